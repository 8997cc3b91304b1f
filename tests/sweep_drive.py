"""
Helpers of the reverse-sweep tests that drive the in-place goal step where the optimiser alone would
not: the in-place route for a source whose wavefronts are no narrow bundles, and the sweep's
gradient with respect to the source rays, which a fused step never asks for.
"""
import ctypes

import torch


def force_in_place(monkeypatch, eng):
    """Every trace of `eng` after the first takes the in-place route (tfrt_scene3d.coherent_only and
    in_place), whatever its wavefronts left over -- what tests/test_gpu_inplace_oracle.py sets by
    hand on its scenes; k_trace_inplace handles every wavefront itself.  The engine's own rule (a
    source that left a wavefront to the grouped kernel is not traced in place) is a choice of speed."""
    def note(self, left_over, passes=1):
        self._visit_all_key = getattr(self, "_visit_key", None)
    monkeypatch.setattr(type(eng), "_note_left_over", note)
    eng.coherent = True


def capture_source_gradient(monkeypatch):
    """tfrt_trace3d_backward_goal is handed a (6, n_rays) float64 block for grad_src_rays (the fused
    step passes NULL) -> dict whose "g_src" is the block of the last call, in the trace's ray order."""
    from tensorflowraytrace_amd import _lib
    handle = _lib.lib()
    entry = handle.tfrt_trace3d_backward_goal
    GRAD_SRC = 26              # position of grad_src_rays in the entry's argument list
    box = {}

    def with_source_gradient(*args):
        args = list(args)
        assert args[GRAD_SRC] is None
        g = torch.zeros((6, int(args[2])), dtype=torch.float64, device="cuda")
        box["g_src"] = g
        args[GRAD_SRC] = ctypes.c_void_p(g.data_ptr())
        return entry(*args)
    monkeypatch.setattr(handle, "tfrt_trace3d_backward_goal", with_source_gradient)
    return box


def natural_order(g_src, perm):
    """The captured block with its columns in the source's own order (`perm`: the trace's order)."""
    if perm is None:
        return g_src
    out = torch.zeros_like(g_src)
    out[:, perm.long()] = g_src
    return out
