"""Timeline of k_trace_inplace's wavefronts in the bench workload's fused optimiser step (needs a
-DTFRT_TUNING -DTFRT_TICKS build: TFRT_LIB_PATH=scratch/variants_live/lib_ticks.so; the stage clocks
of that build lengthen every life).  Usage: inplace_wave_times.py RAYS off|auto"""
import sys, os, ctypes
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..")); sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np, torch, bench
import tfrt.optimizer as optimizer
from tensorflowraytrace_amd import _lib
N = int(sys.argv[1]); mode = sys.argv[2]
eng, system, params = bench.build_scene(N, 41, 9, torch.float32)
eng.wave_schedule = "auto" if mode == "auto" else False
opt = optimizer.SGD_Optimizer(eng, params, bench.make_error_function(), trace_depth=3, learning_rate=1e-6,
                              grad_clip=1e-3, fused="auto", graph=False)
opt.suppress_warnings = True
for _ in range(12): opt.single_step(None)
torch.cuda.synchronize()
fs = opt._fused_step; st = fs._state
assert fs.in_place and fs.folded_backward
G = (N + 63) // 64
sched = st.sched.cpu().numpy() if (mode == "auto" and st.sched is not None) else np.arange(G)
place = np.empty(G, dtype=np.int64); place[sched] = np.arange(G)      # wavefront -> dispatch position
h = ctypes.CDLL(_lib.LIB_PATH)
t0 = np.zeros(65536, dtype=np.uint64); t1 = np.zeros(65536, dtype=np.uint64); info = np.zeros(65536, dtype=np.uint64)
h.tfrt_debug_wave_times(t0.ctypes.data_as(ctypes.c_void_p), t1.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p))
W = min(G, 65536)
a = t0[:W].astype(np.int64); b = t1[:W].astype(np.int64)
base = a.min(); a -= base; b -= base
life = (b - a) / 100.0
print(f"N={N} schedule {mode} ({'built' if mode == 'auto' and st.sched is not None else 'index order'}): {W} wavefronts, "
      f"launch span {b.max() / 100:.1f} us; life us: mean {life.mean():.2f} p50 {np.percentile(life, 50):.2f} "
      f"p90 {np.percentile(life, 90):.2f} p99 {np.percentile(life, 99):.2f} max {life.max():.2f}; "
      f"sum of lives / 5120 slots {life.sum() / 5120:.1f} us")
edges = np.linspace(0, b.max(), 21)
mid = (edges[:-1] + edges[1:]) / 2
print("  resident wavefronts at 20 instants:", [int(((a <= m) & (b > m)).sum()) for m in mid])
tail = np.linspace(b.max() - 2000, b.max(), 21)      # the last 20 us, 1 us apart
print("  resident wavefronts in the last 20 us, 1 us apart:", [int(((a <= m) & (b > m)).sum()) for m in tail[:-1]])
for frac in (0.5, 0.25, 0.1):
    t = np.sort(b)[::-1]
    k = int(5120 * frac)
    print(f"  chip below {int(frac * 100)} % of its slots for the last {(b.max() - t[k]) / 100:.1f} us")
rows = None
try:
    from tensorflowraytrace_amd import ops
    rows = ops.wave_rows(st.N, st.M, st.P, st.block.dtype, st.ws).cpu().numpy().view(np.uint32)
    passes = (rows[:st.P] != 0).sum(0); faces = rows[st.P + 1]
    for p in range(1, st.P + 1):
        m = passes[:W] == p
        if m.any(): print(f"  passes entered {p}: {int(m.sum())} wavefronts, mean life {life[m].mean():.1f} us, mean faces {faces[:W][m].mean():.1f}")
except AttributeError:
    pass
slow = np.argsort(-life)[:10]
print("  slowest (index: life us, start us, dispatch position):", [(int(i), round(float(life[i]), 1), round(float(a[i] / 100), 1), int(place[i])) for i in slow])
late = np.argsort(-b)[:10]
print("  last to finish (index: life us, start us, end us, dispatch position):", [(int(i), round(float(life[i]), 1), round(float(a[i] / 100), 1), round(float(b[i] / 100), 1), int(place[i])) for i in late])
last_disp = sched[-8:]
print("  last dispatched (index: life us, start us):", [(int(i), round(float(life[i]), 1), round(float(a[i] / 100), 1)) for i in last_disp])
