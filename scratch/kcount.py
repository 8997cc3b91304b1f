#!/usr/bin/env python3
"""Static instruction counts per kernel from device assembly, next to the compiler's resource remarks.
usage: hipcc <the library's flags> --cuda-device-only -S csrc/tfrt_trace3d.hip -o X.s -Rpass-analysis=kernel-resource-usage 2> X.res
       python scratch/kcount.py X.s X.res [name-filter] [--loads KERNEL-SUBSTRING]
v_ / s_: vector / scalar instructions, lane: v_readlane + v_writelane among the vector ones,
f64: v_{add,mul,fma,div*,rcp,rsq,sqrt}_f64 (profiles/r06_backward_resources.txt), *_f64: every mnemonic ending in _f64.
--loads: the global_load* / s_waitcnt vmcnt sequence of the blocks of that kernel's first outermost loop with six global loads or more."""
import argparse, re, subprocess

ap = argparse.ArgumentParser()
ap.add_argument("asm"); ap.add_argument("res"); ap.add_argument("filt", nargs="?", default="")
ap.add_argument("--loads", default=None)
a = ap.parse_args()
asm, res, filt, loads = a.asm, a.res, a.filt, a.loads

remarks, cur = {}, None
for line in open(res):
    m = re.search(r"remark: +(.*?) \[-Rpass", line)
    if not m:
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = remarks.setdefault(t.split(":", 1)[1].strip(), {})
    elif cur is not None and ":" in t:
        k, v = t.split(":", 1)
        cur[k.strip()] = v.strip()

kernels, name = {}, None
for line in open(asm):
    m = re.match(r"^(_Z\w+):", line)
    if m and m.group(1) in remarks:
        name = m.group(1)
        kernels[name] = []
        continue
    if name is not None:
        t = line.strip()
        if t and not t.startswith((";", ".")) or re.match(r"^\.LBB", t):
            kernels[name].append(t)
        if t.startswith("s_endpgm"):
            name = None

names = list(kernels)
dem = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE).stdout.decode().splitlines()
F64 = re.compile(r"^v_(add|mul|fma|div\w*|rcp|rsq|sqrt)_f64")
print(f"{'kernel':52s} {'SGPR':>4s} {'VGPR':>4s} {'sspill':>6s} {'vsp':>3s} {'scr':>4s} {'occ':>3s} {'LDS':>6s} {'v_':>5s} {'s_':>5s} {'lane':>4s} {'f64':>4s} {'*_f64':>5s}")
for n, d in zip(names, dem):
    d = re.sub(r"\(.*", "", d).replace("void tfrt::", "").replace("tfrt::", "")
    if filt and filt not in d:
        continue
    ins = [t.split()[0] for t in kernels[n] if not t.endswith(":") and not t.startswith(".LBB")]
    r = remarks[n]
    v = sum(i.startswith("v_") for i in ins)
    s = sum(i.startswith("s_") for i in ins)
    lane = sum(i.startswith(("v_readlane", "v_writelane")) for i in ins)
    f64 = sum(bool(F64.match(i)) for i in ins)
    any64 = sum(bool(re.search(r"_f64(_e32|_e64)?$", i)) for i in ins)
    print(f"{d[:52]:52s} {r.get('TotalSGPRs', '?'):>4s} {r.get('VGPRs', '?'):>4s} {r.get('SGPRs Spill', '?'):>6s} "
          f"{r.get('VGPRs Spill', '?'):>3s} {r.get('ScratchSize [bytes/lane]', '?'):>4s} {r.get('Occupancy [waves/SIMD]', '?'):>3s} "
          f"{r.get('LDS Size [bytes/block]', '?'):>6s} {v:5d} {s:5d} {lane:4d} {f64:4d} {any64:5d}")

if loads:
    for n, d in zip(names, dem):
        if loads not in d:
            continue
        body = kernels[n]
        # the pass loop: from the first loop header after the forward walk to the branch back to it
        heads = [i for i, t in enumerate(body) if re.match(r"^\.LBB\d+_\d+:.*Loop Header: Depth=1", t)]
        for h in heads:
            label = body[h].split(":")[0]
            tag = label[1:]                       # ".LBB47_17" -> "LBB47_17" as the block comments name it
            tag = tag[1:] if tag.startswith("L") else tag
            seg, inside = [], False
            for t in body[h:]:
                if re.match(r"^\.LBB\d+_\d+:", t):   # a block label says which loop it lies in
                    inside = t.startswith(label + ":") or ("Header=" + tag) in t or ("Parent Loop " + tag) in t
                elif inside:
                    seg.append(t)
            if sum("global_load" in t for t in seg) >= 6:
                print(f"\n{d[:70]}: global loads and waits for them in the pass loop ({label}), in layout order")
                for t in seg:
                    if t.startswith("global_load") or (t.startswith("s_waitcnt") and "vmcnt" in t):
                        print("   ", t.split(";")[0].strip())
                break
