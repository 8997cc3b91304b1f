"""
torch-facing wrappers of the HIP entry points (tensors are only device-array containers).

Everything here requires HIP tensors; CPU tensors raise ``TfrtError`` -- there is no CPU
fallback of the hot path.

* ``build_faces``            -> tfrt_build_faces_forward/backward  (autograd.Function)
* ``trace3d`` / ``Trace3D``  -> tfrt_trace3d_forward/backward      (autograd.Function)
* ``intersect3d``            -> tfrt_intersect3d                   (seam S1, engine.py:1103)
* ``snell3d`` / ``snell2d``  -> tfrt_snell3d / tfrt_snell2d        (seam S3, geometry.py:671/565)
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import TfrtError, RayOut, Scene3D, check

_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.float16: _lib.F16}


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise TfrtError(
                "tfrt kernels need tensors on a HIP device (got a CPU tensor); the hot path has "
                "no CPU fallback")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    """The current HIP stream of ``t``'s device as a ``void*`` (the raw accessor avoids building
    a ``torch.cuda.Stream`` object per C call: ~8 us each, eight calls per optimiser step)."""
    if _raw_stream is not None:
        idx = t.device.index
        return ctypes.c_void_p(_raw_stream(idx if idx is not None else torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _c(t, dtype=None):
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


# ------------------------------------------------------------------------- build_faces

_corner_cache = {}


def _check_face_indices(faces, n_vertices):
    """Raise TfrtError unless every index of ``faces`` lies in [0, n_vertices).  One device
    read: vertex_corners calls it once per face tensor, never on a cache hit."""
    if faces.numel() == 0:
        return
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).tolist())
    if lo < 0 or hi >= int(n_vertices):
        raise TfrtError(f"faces: vertex indices must lie in [0, {int(n_vertices)}), got "
                        f"{lo} .. {hi}")


def vertex_corners(faces, n_vertices):
    """(corner_start (V+1) i32, corner_list (3F) i32): the face corners ``f*3+c`` sorted by the
    vertex they reference, for the gather form of the reverse kernels (deterministic, no
    atomics).  Built once per face tensor (mesh topology) and cached with it.

    This is also where the host validates the face indices the kernels rely on (TfrtError for
    an index outside [0, V)): where the table is built, so once per face tensor; a cache hit
    costs no launch and no synchronisation.  Building reads the device (the check, bincount), so
    the first call for a face tensor has to come outside any graph capture.  The cache is keyed
    by the tensor itself: a caller whose faces are not int32 and contiguous already hands
    build_faces / param_faces a fresh copy on every call and pays table and check every time --
    keep the converted tensor, as boundaries.py does."""
    key = (faces.data_ptr(), tuple(faces.shape), int(n_vertices), faces._version)
    hit = _corner_cache.get(key)
    if hit is not None and hit[0] is faces:
        return hit[1], hit[2]
    _check_face_indices(faces, n_vertices)
    flat = faces.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=int(n_vertices))[:int(n_vertices)]
    start = torch.zeros(int(n_vertices) + 1, dtype=torch.int32, device=faces.device)
    start[1:] = torch.cumsum(counts, 0).to(torch.int32)
    if len(_corner_cache) > 256:
        _corner_cache.clear()
    _corner_cache[key] = (faces, start.contiguous(), order.to(torch.int32).contiguous())
    return _corner_cache[key][1], _corner_cache[key][2]


class _BuildFaces(torch.autograd.Function):
    """vertices (V,3) f64 -> face_verts (F,9) f64, norm (F,3) f64.

    boundaries.py:890-923; ``update_mask`` (F,3) uint8 is the vertex_update_map
    (0 = stop_gradient for that corner, boundaries.py:900-913)."""

    @staticmethod
    def forward(ctx, vertices, faces, update_mask):
        _need_gpu(vertices, faces, update_mask)
        vertices = _c(vertices, torch.float64)
        F = faces.shape[0]
        # (validates the indices, also when no gradient is wanted; outside any graph capture)
        corners = vertex_corners(faces, vertices.shape[0]) if F > 0 else None
        fv = torch.empty((F, 9), dtype=torch.float64, device=vertices.device)
        norm = torch.empty((F, 3), dtype=torch.float64, device=vertices.device)
        check(_lib.lib().tfrt_build_faces_forward(
            _p(vertices), vertices.shape[0], _p(faces), F, _p(fv), _p(norm), _stream(vertices)),
            "tfrt_build_faces_forward")
        ctx.save_for_backward(fv, faces, update_mask)
        ctx.n_vertices = vertices.shape[0]
        ctx.corners = corners
        # (an output the loss does not touch arrives as None, not as zeros: a zero upstream on the
        # NaN normal of a zero-area face would turn its vertices' gradients into NaN)
        ctx.set_materialize_grads(False)
        return fv, norm

    @staticmethod
    def backward(ctx, g_fv, g_norm):
        fv, faces, update_mask = ctx.saved_tensors
        g_fv = _c(g_fv, torch.float64)
        g_norm = _c(g_norm, torch.float64)
        if (g_fv is None and g_norm is None) or faces.shape[0] == 0:
            return torch.zeros((ctx.n_vertices, 3), dtype=torch.float64, device=fv.device), None, None
        start, lst = ctx.corners
        gv = torch.empty((ctx.n_vertices, 3), dtype=torch.float64, device=fv.device)
        check(_lib.lib().tfrt_build_faces_backward(
            _p(g_fv), _p(g_norm), _p(fv), _p(faces), _p(update_mask), faces.shape[0],
            ctx.n_vertices, _p(start), _p(lst), _p(gv), _stream(fv)), "tfrt_build_faces_backward")
        return gv, None, None


def build_faces(vertices, faces, update_mask=None):
    """faces: (F,3) int32 on the same device; update_mask: (F,3) uint8/bool or None."""
    faces = _c(faces, torch.int32)
    if update_mask is not None:
        update_mask = _c(update_mask, torch.uint8)
    return _BuildFaces.apply(vertices, faces, update_mask)


class _ParamFaces(torch.autograd.Function):
    """parameters (V,) -> face_verts (F,9), norm (F,3) of ``zero + parameters[:,None] * vectors``
    (boundaries.py:1065-1092 + 890-923) in one launch each way; see tfrt_param_faces_*."""

    @staticmethod
    def forward(ctx, parameters, zero_points, vectors, faces, update_mask):
        _need_gpu(parameters, zero_points, vectors, faces, update_mask)
        parameters = _c(parameters, torch.float64).reshape(-1)
        V, F = zero_points.shape[0], faces.shape[0]
        if parameters.shape[0] != V or vectors.shape != zero_points.shape:
            raise TfrtError("param_faces: parameters (V,), zero_points (V,3) and vectors (V,3) "
                            "must describe the same vertices")
        corners = vertex_corners(faces, V) if F > 0 else None      # (validates the indices)
        fv = torch.empty((F, 9), dtype=torch.float64, device=parameters.device)
        norm = torch.empty((F, 3), dtype=torch.float64, device=parameters.device)
        check(_lib.lib().tfrt_param_faces_forward(
            _p(zero_points), _p(vectors), _p(parameters), V, _p(faces), F, _p(fv), _p(norm),
            _stream(parameters)), "tfrt_param_faces_forward")
        ctx.save_for_backward(fv, faces, update_mask, vectors)
        ctx.shape = parameters.shape
        ctx.corners = corners
        ctx.set_materialize_grads(False)
        return fv, norm

    @staticmethod
    def backward(ctx, g_fv, g_norm):
        fv, faces, update_mask, vectors = ctx.saved_tensors
        g_fv = _c(g_fv, torch.float64)
        g_norm = _c(g_norm, torch.float64)
        if (g_fv is None and g_norm is None) or faces.shape[0] == 0:
            return torch.zeros(ctx.shape, dtype=torch.float64, device=fv.device), None, None, None, None
        start, lst = ctx.corners
        gp = torch.empty(ctx.shape, dtype=torch.float64, device=fv.device)
        check(_lib.lib().tfrt_param_faces_backward(
            _p(g_fv), _p(g_norm), _p(fv), _p(faces), _p(update_mask), _p(vectors),
            faces.shape[0], vectors.shape[0], _p(start), _p(lst), _p(gp), _stream(fv)),
            "tfrt_param_faces_backward")
        return gp, None, None, None, None


def param_faces(parameters, zero_points, vectors, faces, update_mask=None):
    """Faces of the parametric surface ``zero_points + parameters[:,None] * vectors``:
    (face_verts (F,9), norm (F,3)), differentiable w.r.t. ``parameters`` only (zero points and
    vectors are constants between reparametrisations, boundaries.py:1084-1085)."""
    faces = _c(faces, torch.int32)
    zero_points = _c(zero_points.detach(), torch.float64)
    vectors = _c(vectors.detach(), torch.float64)
    if update_mask is not None:
        update_mask = _c(update_mask, torch.uint8)
    return _ParamFaces.apply(parameters, zero_points, vectors, faces, update_mask)


class _ParamFacesMulti(torch.autograd.Function):
    """Several parametric surfaces (and the fixed boundaries between them) -> ONE merged
    face_verts block (M,9) and one norm tensor (F,3) per parametric surface, one launch each way
    (tfrt_param_faces_*_multi).  The norms are separate outputs so that a surface whose normals
    the loss does not touch receives no upstream for them (None), as with a function of its own.  ``spec``: list of entries in the order of the merged block,
    ("param", zero_points, vectors, faces, update_mask) taking the next tensor of ``parameters``,
    or ("copy", face_verts (F,9) detached)."""

    @staticmethod
    def forward(ctx, spec, *parameters):
        dev = parameters[0].device if parameters else spec[0][1].device
        rows = [e[3].shape[0] if e[0] == "param" else e[1].shape[0] for e in spec]
        M = int(sum(rows))
        fv = torch.empty((M, 9), dtype=torch.float64, device=dev)
        norms = []
        descs, keep, pars = [], [], []
        at = k = 0
        for e, F in zip(spec, rows):
            d = _lib.FaceSurface()
            d.n_faces = F
            d.face_verts = fv.data_ptr() + at * 72
            if e[0] == "param":
                _, zero, vectors, faces, mask = e
                par = _c(parameters[k], torch.float64).reshape(-1)
                k += 1
                V = zero.shape[0]
                if par.shape[0] != V or vectors.shape != zero.shape:
                    raise TfrtError("param_faces: parameters (V,), zero_points (V,3) and vectors "
                                    "(V,3) must describe the same vertices")
                d.zero_points, d.vectors, d.parameters = _p(zero), _p(vectors), _p(par)
                d.faces, d.n_vertices = _p(faces), V
                norms.append(torch.empty((F, 3), dtype=torch.float64, device=dev))
                d.norm = _p(norms[-1])
                pars.append((at, F, V, faces, mask, vectors, par.shape))
                keep.append(par)
            else:
                d.copy_from = _p(e[1])
            descs.append(d)
            at += F
        stream = _stream(fv)
        for i in range(0, len(descs), _lib.MAX_SURFACES):
            chunk = descs[i:i + _lib.MAX_SURFACES]
            arr = (_lib.FaceSurface * len(chunk))(*chunk)
            check(_lib.lib().tfrt_param_faces_forward_multi(arr, len(chunk), stream),
                  "tfrt_param_faces_forward_multi")
        ctx.pars = pars
        ctx.corners = [vertex_corners(f, V) if F > 0 else None for (_, F, V, f, _, _, _) in pars]
        ctx.save_for_backward(fv)
        ctx.set_materialize_grads(False)
        return (fv, *norms)

    @staticmethod
    def backward(ctx, g_fv, *g_norms):
        (fv,) = ctx.saved_tensors
        g_fv = _c(g_fv, torch.float64)
        out, descs, keep = [], [], []
        for (at, F, V, faces, mask, vectors, shape), corners, g_norm in zip(ctx.pars, ctx.corners,
                                                                            g_norms):
            # (a surface whose normals the loss does not touch has g_norm None and skips the
            # normal's half: a zero upstream would meet the NaN normal of a zero-area face)
            g_norm = _c(g_norm, torch.float64)
            keep.append(g_norm)
            if (g_fv is None and g_norm is None) or F == 0:
                out.append(torch.zeros(shape, dtype=torch.float64, device=fv.device))
                continue
            sink = GradSink._active
            gp = sink.take(shape) if sink is not None else None
            if gp is None:
                gp = torch.empty(shape, dtype=torch.float64, device=fv.device)
            d = _lib.FaceSurfaceGrad()
            if g_fv is not None and FaceSums._active is not None:
                # (the upstream keeps its (M, 9) shape for autograd; the first four doubles of a
                # row are the face's four sums, expanded inside the gather)
                d.grad_face_sums = g_fv.data_ptr() + at * 72
            else:
                d.grad_face_verts = g_fv.data_ptr() + at * 72 if g_fv is not None else None
            d.grad_norm = _p(g_norm)
            d.face_verts = fv.data_ptr() + at * 72
            d.update_mask, d.vectors = _p(mask), _p(vectors)
            d.corner_start, d.corner_list = _p(corners[0]), _p(corners[1])
            d.n_vertices, d.grad_parameters = V, _p(gp)
            descs.append(d)
            out.append(gp)
        stream = _stream(fv)
        for i in range(0, len(descs), _lib.MAX_SURFACES):
            chunk = descs[i:i + _lib.MAX_SURFACES]
            arr = (_lib.FaceSurfaceGrad * len(chunk))(*chunk)
            check(_lib.lib().tfrt_param_faces_backward_multi(arr, len(chunk), stream),
                  "tfrt_param_faces_backward_multi")
        return (None, *out)


_faces_batch = None   # the batch parametric boundaries hand their update to (see ParamFacesBatch)


class GradSink:
    """While active (``with GradSink(flat):``) the parameter gradients of the face updates are
    written into consecutive slices of ``flat`` (a persistent float64 buffer) instead of fresh
    tensors: a sharded optimiser step then all-reduces ``flat`` as it is -- no concatenation
    before the collective, no slicing after it."""

    _active = None

    def __init__(self, flat):
        self.flat, self.at, self.taken = flat, 0, []

    def __enter__(self):
        self._prev, GradSink._active = GradSink._active, self
        return self

    def __exit__(self, *exc):
        GradSink._active = self._prev
        return False

    def take(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        if self.at + n > self.flat.numel():
            return None
        view = self.flat[self.at:self.at + n].view(shape)
        self.at += n
        self.taken.append(view)
        return view

    def holds(self, t):
        """True if ``t`` is one of the slices handed out (same memory, same size)."""
        return any(v.data_ptr() == t.data_ptr() and v.numel() == t.numel() for v in self.taken)


class FaceSums:
    """While active (``with FaceSums():``) the face gradient handed to the merged face update's
    reverse (_ParamFacesMulti) is in the four-sum form of tfrt_scene3d.face_sums: a reverse sweep
    wrote, per face, the four sums its nine vertex gradients are linear in into the first four
    doubles of the face's row of the (M, 9) block, and the gather expands them once per face
    (tfrt_face_surface_grad.grad_face_sums).  Opened by the fused step around its parameter
    gradients, and only when the merged faces come straight from that update."""

    _active = None

    def __enter__(self):
        self._prev, FaceSums._active = FaceSums._active, self
        return self

    def __exit__(self, *exc):
        FaceSums._active = self._prev
        return False


def faces_from_param_update(fv):
    """Whether ``fv`` is the merged face block as _ParamFacesMulti returned it: its gradient then
    reaches that update's reverse untouched by any other node."""
    fn = getattr(fv, "grad_fn", None)
    return fn is not None and getattr(fn, "_forward_cls", None) is _ParamFacesMulti


def current_faces_batch():
    return _faces_batch


class ParamFacesBatch:
    """The face updates of one optical system's update(), collected and run as one launch.

    ``with batch:`` -- inside, ParametricTriangleBoundary._update registers its parameters here
    (``add``) instead of launching; ``flush(order)`` runs everything in ONE launch and hands every
    boundary its rows of the merged block as ``_face_verts`` / ``_norm``.  ``order``: the
    boundaries of the system in the order of its merged face block; boundaries without a request
    whose faces are fixed (no gradient) are copied into place, so the block IS the system's merged
    face tensor (``merged``) and nothing is concatenated afterwards.  A boundary that is asked
    for its faces before that flushes what has been collected so far."""

    def __init__(self):
        self.requests = []      # (boundary, parameters (tap), zero_points, vectors, faces, mask)
        self.merged = None      # (face block, [(boundary, first row, end row)]) after a full flush
        self._outer = None

    def __enter__(self):
        global _faces_batch
        self._outer, _faces_batch = _faces_batch, self
        return self

    def __exit__(self, *exc):
        global _faces_batch
        _faces_batch = self._outer
        return False

    def add(self, boundary, parameters, zero_points, vectors, faces, mask):
        faces = _c(faces, torch.int32)
        zero_points = _c(zero_points.detach(), torch.float64)
        vectors = _c(vectors.detach(), torch.float64)
        if mask is not None:
            mask = _c(mask, torch.uint8)
        _need_gpu(parameters, zero_points, vectors, faces, mask)
        if faces.shape[0] > 0:
            vertex_corners(faces, zero_points.shape[0])     # (validates the indices, cached)
        self.requests.append((boundary, parameters, zero_points, vectors, faces, mask))
        boundary.__dict__["_faces_pending"] = self

    def flush(self, order=None):
        if not self.requests:
            return
        reqs, self.requests = self.requests, []
        by_boundary = {id(r[0]): r for r in reqs}
        layout = None
        if order is not None:
            layout = []
            for b in order:
                r = by_boundary.get(id(b))
                if r is not None:
                    layout.append(("param", r))
                    continue
                fv = b.__dict__.get("_face_verts_value")
                # (a boundary whose xp .. z2 fields were assigned by hand no longer shows its raw
                # vertex block: its face_verts property stacks the fields -- not copyable)
                overridden = any(k in getattr(b, "_fields", {}) for k in
                                 ("xp", "yp", "zp", "x1", "y1", "z1", "x2", "y2", "z2"))
                if (fv is None or overridden or fv.requires_grad or not fv.is_cuda
                        or fv.dtype != torch.float64
                        or not fv.is_contiguous() or fv.dim() != 2 or fv.shape[1] != 9):
                    layout = None   # (something the block cannot hold: faces only, then cat)
                    break
                layout.append(("copy", b, fv))
            if layout is not None and sum(1 for e in layout if e[0] == "param") != len(reqs):
                layout = None
        if layout is None:
            layout = [("param", r) for r in reqs]
        spec = [("param", e[1][2], e[1][3], e[1][4], e[1][5]) if e[0] == "param"
                else ("copy", e[2]) for e in layout]
        pars = [e[1][1] for e in layout if e[0] == "param"]
        fv, *norms = _ParamFacesMulti.apply(spec, *pars)
        at = k = 0
        rows = []
        for e in layout:
            if e[0] == "param":
                b, F = e[1][0], e[1][4].shape[0]
                b.__dict__["_faces_pending"] = None
                b._face_verts = fv[at:at + F]
                b._norm = norms[k]
                rows.append((b, at, at + F))
                k += 1
            else:
                F = e[2].shape[0]
                rows.append((e[1], at, at + F))
            at += F
        if order is not None and len(layout) == len(order):
            self.merged = (fv, rows)


# ------------------------------------------------------------------- pairwise geometry

def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _pairwise(first, second, grid):
    """Common operand handling of the dense geometry functions: returns (n_cols, n_rows,
    first tensors, first strides, second tensors, second strides, output shape).  ``grid``:
    meshgrid form (first set along columns, second along rows); otherwise element-wise."""
    first = [_c(torch.as_tensor(t), torch.float64) for t in first]
    dev = first[0].device
    second = [_c(torch.as_tensor(t, device=dev), torch.float64) for t in second]
    _need_gpu(*first, *second)
    if grid:
        first = [t.reshape(-1) for t in first]
        second = [t.reshape(-1) for t in second]
        n_cols, n_rows = first[0].numel(), second[0].numel()
        if any(t.numel() != n_cols for t in first) or any(t.numel() != n_rows for t in second):
            raise TfrtError("pairwise geometry: operands of one set must have equal lengths")
        return n_cols, n_rows, first, (1, 0), second, (0, 1), (n_rows, n_cols)
    shape = torch.broadcast_shapes(*[t.shape for t in first + second])
    first = [t.expand(shape).contiguous().reshape(-1) for t in first]
    second = [t.expand(shape).contiguous().reshape(-1) for t in second]
    return first[0].numel(), 1, first, (1, 0), second, (1, 0), tuple(shape)


def line_intersect(first, second, epsilion, grid):
    """geometry.py:27-167.  first = (x1s, y1s, x1e, y1e), second = (x2s, y2s, x2e, y2e).
    Returns x, y, valid, u, v."""
    nc, nr, f, fs, s2, ss, shape = _pairwise(first, second, grid)
    dev = f[0].device
    new = lambda: torch.empty(shape, dtype=torch.float64, device=dev)
    x, y, u, v = new(), new(), new(), new()
    valid = torch.empty(shape, dtype=torch.uint8, device=dev)
    fp, keep1 = _ptr_array(f)
    sp, keep2 = _ptr_array(s2)
    check(_lib.lib().tfrt_line_intersect(nc, nr, fp, fs[0], fs[1], sp, ss[0], ss[1],
                                         float(epsilion), _p(x), _p(y), _p(valid), _p(u), _p(v),
                                         _stream(x)), "tfrt_line_intersect")
    return x, y, valid.bool(), u, v


def line_triangle_intersect(rays, triangles, epsilion, grid):
    """geometry.py:191-320.  rays = (rx1..rz2), triangles = (xp..z2).
    Returns x, y, z, valid, ray_u, trig_u, trig_v."""
    nc, nr, f, fs, s2, ss, shape = _pairwise(rays, triangles, grid)
    dev = f[0].device
    new = lambda: torch.empty(shape, dtype=torch.float64, device=dev)
    x, y, z, ru, tu, tv = new(), new(), new(), new(), new(), new()
    valid = torch.empty(shape, dtype=torch.uint8, device=dev)
    fp, keep1 = _ptr_array(f)
    sp, keep2 = _ptr_array(s2)
    check(_lib.lib().tfrt_line_triangle_intersect(
        nc, nr, fp, fs[0], fs[1], sp, ss[0], ss[1], float(epsilion), _p(x), _p(y), _p(z),
        _p(valid), _p(ru), _p(tu), _p(tv), _stream(x)), "tfrt_line_triangle_intersect")
    return x, y, z, valid.bool(), ru, tu, tv


def line_circle_intersect(lines, circles, epsilion, grid):
    """geometry.py:338-547.  lines = (xs, ys, xe, ye), circles = (xc, yc, r).  Returns the
    (plus, minus) dicts with x, y, valid, u, v."""
    nc, nr, f, fs, s2, ss, shape = _pairwise(lines, circles, grid)
    dev = f[0].device
    new = lambda: torch.empty(shape, dtype=torch.float64, device=dev)
    roots = []
    for _ in range(2):
        roots.append(([new(), new(), new(), new()], torch.empty(shape, dtype=torch.uint8, device=dev)))
    fp, keep1 = _ptr_array(f)
    sp, keep2 = _ptr_array(s2)
    pp, keep3 = _ptr_array(roots[0][0])
    mp, keep4 = _ptr_array(roots[1][0])
    check(_lib.lib().tfrt_line_circle_intersect(
        nc, nr, fp, fs[0], fs[1], sp, ss[0], ss[1], float(epsilion), pp, _p(roots[0][1]), mp,
        _p(roots[1][1]), _stream(roots[0][1])), "tfrt_line_circle_intersect")
    out = []
    for (x, y, u, v), valid in roots:
        out.append({"x": x, "y": y, "valid": valid.bool(), "u": u, "v": v})
    return out[0], out[1]


# ------------------------------------------------------------------- parameter update

def sgd_process(grad, scale, clip, param=None, sgd_learning_rate=0.0):
    """optimizer.py:223-247 (+ :316 when ``param`` is given) in one launch: returns
    ``clip(where(isfinite(grad), grad, 0) * scale, -clip, clip)`` and, if ``param`` is given,
    also applies ``param -= sgd_learning_rate * processed`` in place."""
    _need_gpu(grad, param)
    if grad.dtype not in (torch.float32, torch.float64):
        raise TfrtError(f"sgd_process: float32/float64 gradients only, got {grad.dtype}")
    grad = grad.contiguous()
    out = torch.empty_like(grad)
    if param is not None and (param.dtype != grad.dtype or param.shape != grad.shape
                              or not param.is_contiguous()):
        raise TfrtError("sgd_process: param must be contiguous with the gradient's shape and dtype")
    check(_lib.lib().tfrt_sgd_process(
        _p(grad), _p(out), _p(param), grad.numel(), _DT[grad.dtype], float(scale), float(clip),
        float(sgd_learning_rate), _stream(grad)), "tfrt_sgd_process")
    return out


def _update(rule, fn, what, grads, params, states, rows, processed, extras=(), extras_error=None):
    """``rule``'s launch (an _lib.UpdateRule) over any number of float64 tensors, eight at a time.
    ``extras``: (tensor, bytes per tensor) of its trailing device arguments."""
    k = len(grads)
    lists = [grads, params, *states] + ([] if processed is None else [processed])
    if any(len(ts) != k for ts in lists + [rows]):
        raise TfrtError(f"{fn}: one gradient, parameter, {what} and row per tensor")
    if k == 0:
        return
    _need_gpu(*grads, *params, *[t for ts in states for t in ts], *[t for t, _ in extras])
    for per_tensor in zip(*lists):
        if any(t.dtype != torch.float64 or not t.is_contiguous() or t.shape != per_tensor[0].shape
               for t in per_tensor):
            raise TfrtError(f"{fn}: contiguous float64 tensors of one shape per parameter")
    if extras_error is not None:
        raise TfrtError(extras_error)
    hyper = torch.tensor(rows, dtype=torch.float64).to(grads[0].device)
    entry = getattr(_lib.lib(), rule.entry)
    stream = _stream(params[0])
    for lo in range(0, k, 8):
        g, p, *more = [_ptr_array(ts[lo:lo + 8])[1] for ts in lists]
        done = None if processed is None else more.pop()
        n = [t.numel() for t in grads[lo:lo + 8]]
        check(entry(len(n), g, done, p, *more, (ctypes.c_int64 * len(n))(*n),
                    ctypes.c_void_p(hyper.data_ptr() + 8 * rule.width * lo),
                    *[ctypes.c_void_p(t.data_ptr() + stride * lo) for t, stride in extras], stream),
              rule.entry)


def sgd_momentum(grads, params, velocities, rows, processed=None):
    """optimizer.py:223-247 and the Keras SGD momentum apply for float64 tensors, up to eight per
    launch (tfrt_sgd_momentum_multi): ``rows[k] = (scale, clip, sgd_learning_rate, momentum,
    nesterov)``.  Updates ``params`` and ``velocities`` in place (``velocities`` untouched while
    momentum is 0); writes the processed gradients into ``processed`` if given."""
    _update(_lib.MOMENTUM, "sgd_momentum", "velocity", grads, params, [velocities], rows, processed)


def adam(grads, params, ms, vs, rows, state, ticket, processed=None):
    """optimizer.py:223-247 and the Keras Adam apply for float64 tensors, up to eight per launch
    (tfrt_adam_multi): ``rows[k] = (scale, clip, adam_learning_rate, beta1, beta2, epsilon)``,
    ``state`` the (k, 3) float64 {t, p1, p2} of these tensors and ``ticket`` one zeroed int32, both
    on the device.  Updates ``params``, ``ms``, ``vs`` and ``state`` in place; writes the processed
    gradients into ``processed`` if given."""
    ok = (state.dtype == torch.float64 and tuple(state.shape) == (len(grads), 3)
          and state.is_contiguous() and ticket.dtype == torch.int32 and ticket.numel() >= 1)
    # (the launches of one call run one after the other on one stream: one ticket word for all)
    _update(_lib.ADAM, "adam", "m, v", grads, params, [ms, vs], rows, processed,
            extras=((state, _lib.ADAM.extras[0][1]), (ticket, 0)),
            extras_error=None if ok else "adam: state is (n_tensors, 3) float64, ticket one int32")


class CsrMatrix:
    """A square accumulator / smoother matrix held in CSR form on the device
    (optimizer.py:250-255, 277-282 multiply dense (P,P) matrices whose rows hold a few
    non-zeros, mesh_tools.py:221-421)."""

    def __init__(self, matrix, device):
        if isinstance(matrix, torch.Tensor):
            dense = matrix.detach().to_dense() if matrix.layout != torch.strided else matrix.detach()
            dense = dense.to(device="cpu", dtype=torch.float64).numpy()
        else:
            dense = np.asarray(matrix, dtype=np.float64)
        if dense.ndim != 2:
            raise TfrtError("CsrMatrix: need a rank-2 matrix")
        rows, cols = np.nonzero(dense)                      # row-major order = CSR order
        crow = np.zeros(dense.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=dense.shape[0]), out=crow[1:])
        self.shape = tuple(dense.shape)
        self.nnz = int(rows.size)
        self.crow = torch.as_tensor(crow).to(device)
        self.col = torch.as_tensor(cols.astype(np.int64)).to(device)
        self.val = torch.as_tensor(np.ascontiguousarray(dense[rows, cols])).to(device)

    def matvec(self, x):
        """A @ x for a (P,) or (P,1) float64 vector on the matrix's device."""
        _need_gpu(x)
        shape = x.shape
        v = _c(x.reshape(-1), torch.float64)
        if v.shape[0] != self.shape[1]:
            raise TfrtError(f"CsrMatrix.matvec: matrix is {self.shape}, vector has {v.shape[0]}")
        y = torch.empty(self.shape[0], dtype=torch.float64, device=v.device)
        check(_lib.lib().tfrt_csr_matvec(_p(self.crow), _p(self.col), _p(self.val), _p(v), _p(y),
                                         self.shape[0], _stream(v)), "tfrt_csr_matvec")
        return y.reshape(shape).to(x.dtype) if self.shape[0] == self.shape[1] else y


# ----------------------------------------------------------------------------- trace3d

class Scene3DArgs:
    """Device tensors + scalars describing the merged 3-D boundary set (tfrt_scene3d)."""

    def __init__(self, face_verts, catagory, mat_in=None, mat_out=None, n_in=None, n_out=None,
                 n_table=None, intersect_epsilion=1e-10, size_epsilion=1e-10,
                 ray_start_epsilion=1e-10, face_grad_mask=None, cluster_order=None,
                 deterministic=False, coherent_rays=False):
        self.face_verts = face_verts  # (M,9) f64, may require grad
        self.catagory = _c(catagory, torch.int32)
        self.mat_in = _c(mat_in, torch.int32)
        self.mat_out = _c(mat_out, torch.int32)
        self.n_in = _c(n_in, torch.float64)
        self.n_out = _c(n_out, torch.float64)
        # "value" mode: the tensors as handed in (they may require grad: d error / d index)
        self.n_in_arg = n_in if isinstance(n_in, torch.Tensor) else None
        self.n_out_arg = n_out if isinstance(n_out, torch.Tensor) else None
        self.n_table = _c(n_table, torch.float64)  # (n_materials, N)
        # True: `n_table` has ONE column that holds for every ray (one wavelength)
        self.n_table_uniform = False
        self.face_grad_mask = _c(face_grad_mask, torch.uint8)  # (M) or None
        self.cluster_order = _c(cluster_order, torch.int32)    # (M) or None: two-level filter
        self.deterministic = bool(deterministic)               # ordered reverse-sweep sums
        # True: the rays handed to the trace are in a coherent order (see ray_order()): wavefronts
        # share one walk of the hierarchy (k_intersect_beam), the reverse sweep sums per wavefront.
        # May be reassigned between traces (it belongs to the source, not to the boundaries).
        self.coherent_rays = bool(coherent_rays)
        # with coherent_rays: True = launch no grouped kernel behind k_intersect_beam (a source
        # whose earlier traces left no wavefront over: out["left_over"] == 0)
        self.coherent_only = False
        # with coherent_rays: all passes in ONE launch, rays kept in place (tfrt_scene3d.in_place)
        self.in_place = False
        self.eps = (float(intersect_epsilion), float(size_epsilion), float(ray_start_epsilion))

    def struct(self, face_verts):
        M = face_verts.shape[0]
        cached = getattr(self, "_struct_cache", None)
        if cached is not None and cached[0] == M:
            # every other field points at tensors this object owns: only the face pointer moves
            sc = cached[1]
            sc.face_verts = face_verts.data_ptr() if M else None
            sc.coherent_rays = 1 if self.coherent_rays else 0
            sc.coherent_only = 1 if (self.coherent_only and self.coherent_rays) else 0
            sc.n_table_uniform = 1 if self.n_table_uniform else 0
            sc.in_place = 1 if (self.in_place and self.coherent_rays) else 0
            return sc
        sc = Scene3D()
        sc.face_verts = face_verts.data_ptr() if M else None
        sc.catagory = self.catagory.data_ptr() if M else None
        for name in ("mat_in", "mat_out", "n_in", "n_out"):
            t = getattr(self, name)
            setattr(sc, name, t.data_ptr() if (t is not None and M) else None)
        sc.n_faces = M
        if self.n_table is not None and self.n_table.numel():
            sc.n_table = self.n_table.data_ptr()
            sc.n_table_stride = self.n_table.shape[1]
            sc.n_materials = self.n_table.shape[0]
        else:
            sc.n_table, sc.n_table_stride, sc.n_materials = None, 0, 0
        sc.intersect_epsilion, sc.size_epsilion, sc.ray_start_epsilion = self.eps
        g = self.face_grad_mask
        sc.face_grad_mask = g.data_ptr() if (g is not None and M) else None
        co = self.cluster_order
        if co is not None and co.numel() != M:
            raise TfrtError("cluster_order must be a permutation of the M face indices")
        sc.cluster_order = co.data_ptr() if (co is not None and M) else None
        sc.n_table_uniform = 1 if self.n_table_uniform else 0
        sc.deterministic = 1 if self.deterministic else 0
        sc.coherent_rays = 1 if self.coherent_rays else 0
        sc.coherent_only = 1 if (self.coherent_only and self.coherent_rays) else 0
        sc.in_place = 1 if (self.in_place and self.coherent_rays) else 0
        self._struct_cache = (M, sc)
        return sc


class TraceTape:
    """Everything the reverse sweep needs (kept alive by the autograd node)."""
    pass


def _ray_out(rays, ids, faces):
    o = RayOut()
    if rays is None:
        o.rays, o.ray_id, o.face, o.capacity = None, None, None, 0
    else:
        o.rays, o.ray_id, o.face, o.capacity = rays.data_ptr(), ids.data_ptr(), faces.data_ptr(), rays.shape[1]
    return o


class _IntPool:
    """The int32 outputs of one trace (counts + per-class source ids and faces) cut from one
    allocation: one fill instead of one per array when they must start as zeros."""

    def __init__(self, dev, zero_all, n_counts, flags, cap_n, passes):
        caps = ((_lib.COMPILE_FINISHED, cap_n), (_lib.COMPILE_ACTIVE, cap_n * max(passes, 1)),
                (_lib.COMPILE_STOPPED, cap_n), (_lib.COMPILE_DEAD, cap_n))
        pad = self._pad
        total = pad(n_counts) + pad(cap_n) + sum(2 * pad(c) for f, c in caps if flags & f)
        if zero_all:
            self._buf = torch.zeros(total, dtype=torch.int32, device=dev)
        else:
            self._buf = torch.empty(total, dtype=torch.int32, device=dev)
            self._buf[:n_counts].zero_()
        self.counts = self._buf[:n_counts]
        self._at = pad(n_counts)

    @staticmethod
    def _pad(n):          # every array starts on a 256-byte boundary, like its own allocation
        return (n + 63) & ~63

    def take(self, n):
        out = self._buf[self._at:self._at + n]
        self._at += self._pad(n)
        return out


def _with_rows(blocks, present):
    """Outputs of a trace Function: the class blocks followed by the rows of every compiled class
    (views of the same memory).  A consumer that differentiates single fields of a class (``y_end``
    of the finished rays, say) takes the row outputs: autograd then hands backward() that row's
    gradient alone instead of assembling a dense zero-padded block per field it touched
    (select_backward + slice_backward + add over (rows, capacity): ~90 us per step at 1M rays)."""
    rows = []
    for b, p in zip(blocks, present):
        if p:
            rows.extend(b.unbind(0))
    return tuple(blocks) + tuple(rows)


def _split_rows(outs, present, n_rows):
    """(class blocks, {class name: its row outputs}) from the outputs of a trace Function."""
    rows, at = {}, 4
    for name, p in zip(_CLASS_NAMES, present):
        if p:
            rows[name] = outs[at:at + n_rows]
            at += n_rows
    return outs[:4], rows


def _class_grads(ctx_present, caps, n_rows, dev, grads):
    """Float64 (rows, capacity) gradient block per class from the block / row gradients that
    autograd delivered (None where the class took no gradient at all)."""
    blocks, rows = grads[:4], grads[4:]
    out, at = [], 0
    for k, present in enumerate(ctx_present):
        if not present:
            out.append(None)
            continue
        gb, gr = blocks[k], rows[at:at + n_rows]
        at += n_rows
        if gb is None and all(g is None for g in gr):
            out.append(None)
            continue
        if all(g is None for g in gr):
            out.append(_c(gb, torch.float64))
            continue
        if gb is None:
            blk = torch.zeros((n_rows, caps[k]), dtype=torch.float64, device=dev)
        else:
            blk = gb.to(torch.float64, copy=True).contiguous()
        for i, g in enumerate(gr):
            if g is not None:
                if gb is None:
                    blk[i].copy_(g)
                else:
                    blk[i].add_(g)
        out.append(blk)
    return out


class _Trace3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, face_verts, n_in, n_out, scene, opts):
        # (n_in / n_out: the per-face indices of "value" mode when they require grad -- the values
        # are read through `scene`; listing them here gives their gradients a place to go)
        _need_gpu(src, face_verts)
        dev = src.device
        if src.dtype not in _DT:
            raise TfrtError(f"ray state dtype must be float32, float64 or float16, got {src.dtype}")
        src = src.contiguous()
        face_verts = _c(face_verts, torch.float64)
        N = src.shape[1]
        P = int(opts["max_passes"])
        flags = int(opts["flags"])
        dt = _DT[src.dtype]
        L = _lib.lib()
        wsb = L.tfrt_trace3d_workspace_bytes(N, face_verts.shape[0], P, dt)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        # With speculative slicing (predicted counts) rows beyond the true counts may be read
        # before the prediction is verified: the index arrays must then hold valid indices
        # (zeros); the ray blocks may hold anything, a wrong guess is re-evaluated anyway.
        capN = max(N, 1)
        ints = _IntPool(dev, bool(opts.get("zero_init")), _lib.COUNTS_PER_PASS * (P + 1), flags,
                        capN, P)
        counts = ints.counts

        def alloc(flag, cap):
            if not (flags & flag):
                return None, None, None
            return (torch.empty((6, cap), dtype=src.dtype, device=dev), ints.take(cap),
                    ints.take(cap))

        fin = alloc(_lib.COMPILE_FINISHED, capN)
        act = alloc(_lib.COMPILE_ACTIVE, capN * max(P, 1))
        stp = alloc(_lib.COMPILE_STOPPED, capN)
        dead = alloc(_lib.COMPILE_DEAD, capN)
        unf = torch.empty((6, capN), dtype=src.dtype, device=dev)
        unf_id = ints.take(capN)
        sc = scene.struct(face_verts)
        outs = [_ray_out(*o) for o in (fin, act, stp, dead)]
        perm = opts.get("perm")
        # an in-place trace over permuted rays compacts its ray sets in the CALLER's order itself
        # (tfrt_scene3d.ray_slot = the inverse of `perm`): nothing to restore afterwards
        own_order = bool(perm is not None and N
                         and L.tfrt_trace3d_in_place(ctypes.byref(sc), N, P) == 1)
        inv = None
        if own_order:
            inv = opts.get("ray_slot")
            inv = inverse_order(perm) if inv is None else inv
            sc.ray_slot = inv.data_ptr()
        # lazy (trace3d(lazy=True)) over an in-place trace: the forward call is given no room for
        # ray sets -- set-up launch + ONE trace launch --, and the sets are compacted from the tape
        # (tfrt_trace3d_compact into the very tensors returned here) when the caller cuts them
        in_place_now = bool(N and (own_order or (
            perm is None and L.tfrt_trace3d_in_place(ctypes.byref(sc), N, P) == 1)))
        defer = bool(opts.get("lazy") and in_place_now)
        none = [_ray_out(None, None, None) for _ in range(4)] if defer else None
        fo = none if defer else outs
        try:
            check(L.tfrt_trace3d_forward(
                _p(src), src.shape[1], N, ctypes.byref(sc), float(opts["new_ray_length"]),
                float(opts["dead_ray_length"] or 0.0), P, dt, flags,
                ctypes.byref(fo[0]), ctypes.byref(fo[1]), ctypes.byref(fo[2]),
                ctypes.byref(fo[3]), None if defer else _p(unf), None if defer else _p(unf_id),
                _p(counts), _p(ws), wsb, _stream(src)),
                "tfrt_trace3d_forward")
        finally:
            sc.ray_slot = None          # (the struct is cached on the scene)
        if defer:
            M = face_verts.shape[0]
            dead_len = float(opts["dead_ray_length"] or 0.0)

            def compact(src=src, outs=outs, unf=unf, unf_id=unf_id, counts=counts, ws=ws, inv=inv):
                check(L.tfrt_trace3d_compact(
                    _p(src), src.shape[1], N, dead_len, P, dt, flags, ctypes.byref(outs[0]),
                    ctypes.byref(outs[1]), ctypes.byref(outs[2]), ctypes.byref(outs[3]), _p(unf),
                    _p(unf_id), _p(counts), M, _p(inv), _p(ws), wsb, _stream(src)),
                    "tfrt_trace3d_compact")
            opts["_compact"] = compact
        tape = TraceTape()
        tape.src, tape.face_verts, tape.scene, tape.opts = src, face_verts, scene, dict(opts)
        tape.ws, tape.wsb, tape.counts, tape.dt = ws, wsb, counts, dt
        tape.caps = [o[0].shape[1] if o[0] is not None else 0 for o in (fin, act, stp, dead)]
        tape.dest = None
        if perm is not None and N and not own_order:
            # `src` is a permuted source (src = natural[:, perm], e.g. perm = ray_order(natural)):
            # hand every class back in the reference's order, ids in the natural numbering; the
            # reverse sweep takes the gradients back through `dest`
            tape.dest = []
            restored = []
            zero = bool(opts.get("zero_init"))
            for o, col in zip((fin, act, stp, dead),
                              (_lib.CLS_FINISHED, _lib.CLS_ACTIVE, _lib.CLS_STOPPED, _lib.CLS_DEAD)):
                if o[0] is None:
                    tape.dest.append(None)
                    restored.append(o)
                    continue
                at = _lib.COUNTS_PER_PASS * P + col
                total = counts[at:at + 1]
                inv, dest, ids_o = restore_plan(o[1], counts, P, col, perm, N, o[0].shape[1],
                                                zero=zero)
                face = torch.zeros_like(o[2]) if zero else None
                restored.append((gather_rows(o[0], inv, total), ids_o,
                                 gather_rows(o[2], inv, total, out=face)))
                tape.dest.append((dest, total))
            fin, act, stp, dead = restored
            if P > 0:
                at = _lib.COUNTS_PER_PASS * (P - 1) + _lib.CLS_ACTIVE
                total = counts[at:at + 1]
                inv, _, ids_o = restore_plan(unf_id, None, 0, None, perm, N, capN, total, zero=zero)
                unf, unf_id = gather_rows(unf, inv, total), ids_o
        ctx.tape = tape
        aux = {
            "counts": counts, "unfinished": unf, "unfinished_id": unf_id,
            "finished_id": fin[1], "finished_face": fin[2],
            "active_id": act[1], "active_face": act[2],
            "stopped_id": stp[1], "stopped_face": stp[2],
            "dead_id": dead[1], "dead_face": dead[2],
        }
        opts["_aux"] = aux
        empty = torch.empty((6, 0), dtype=src.dtype, device=dev)
        rays = [o[0] if o[0] is not None else empty for o in (fin, act, stp, dead)]
        ctx.present = [o[0] is not None for o in (fin, act, stp, dead)]
        ctx.set_materialize_grads(False)
        return _with_rows(rays, ctx.present)

    @staticmethod
    def backward(ctx, *grads):
        t = ctx.tape
        dev = t.src.device
        M = t.face_verts.shape[0]
        g_fv = torch.zeros((M, 9), dtype=torch.float64, device=dev)
        need_src = ctx.needs_input_grad[0]
        g_src = torch.zeros((6, t.src.shape[1]), dtype=torch.float64, device=dev) if need_src else None
        if t.dest is None:
            gs = _class_grads(ctx.present, t.caps, 6, dev, grads)
        else:
            # restored classes: the gradients go back into the trace's row order, row by row --
            # an error function usually touches one or two of a class's six rows (y_end, z_end),
            # and a random gather of a million float64 costs 15 us per row
            gs, at = [], 4
            for k, present in enumerate(ctx.present):
                if not present:
                    gs.append(None)
                    continue
                gb, gr = grads[k], grads[at:at + 6]
                at += 6
                d = t.dest[k]
                if gb is None and all(g is None for g in gr):
                    gs.append(None)
                    continue
                blk = torch.zeros((6, t.caps[k]), dtype=torch.float64, device=dev)
                if gb is not None:
                    gather_rows(_c(gb, torch.float64), d[0], d[1], out=blk)
                for i, g in enumerate(gr):
                    if g is None:
                        continue
                    row = gather_rows(_c(g, torch.float64), d[0], d[1],
                                      out=blk[i] if gb is None else None)
                    if gb is not None:
                        blk[i].add_(row)
                gs.append(blk)
        sc = t.scene.struct(t.face_verts)
        want_n = (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]) and M > 0
        g_n = torch.zeros((2, M), dtype=torch.float64, device=dev) if want_n else None
        if want_n:
            sc.grad_n_in, sc.grad_n_out = g_n[0].data_ptr(), g_n[1].data_ptr()
        try:
            check(_lib.lib().tfrt_trace3d_backward(
                _p(t.src), t.src.shape[1], t.src.shape[1], ctypes.byref(sc),
                float(t.opts["new_ray_length"]), float(t.opts["dead_ray_length"] or 0.0),
                int(t.opts["max_passes"]), t.dt,
                _p(gs[0]), t.caps[0], _p(gs[1]), t.caps[1], _p(gs[2]), t.caps[2], _p(gs[3]),
                t.caps[3], _p(g_fv), _p(g_src), _p(t.counts), _p(t.ws), t.wsb, _stream(t.src)),
                "tfrt_trace3d_backward")
        finally:
            sc.grad_n_in = sc.grad_n_out = None       # (the struct is cached on the scene)
        if g_src is not None:
            g_src = g_src.to(t.src.dtype)
        g_in = g_n[0] if (want_n and ctx.needs_input_grad[2]) else None
        g_out = g_n[1] if (want_n and ctx.needs_input_grad[3]) else None
        return g_src, g_fv, g_in, g_out, None, None


_CLASS_NAMES = ("finished", "active", "stopped", "dead")
_CLASS_NAMES_BY_COUNT_COLUMN = ("active", "finished", "stopped", "dead")   # counts[:, CLS_*]


class _LazyRows:
    """``rows[i]`` = the first n entries of row i of a class block, cut on first use."""

    def __init__(self, rows, n):
        self._rows, self._n, self._cut = rows, n, {}

    def __len__(self):
        return len(self._rows)

    def __getitem__(self, i):
        r = self._cut.get(i)
        if r is None:
            r = self._cut[i] = self._rows[i][:self._n]
        return r


def _slice_outputs(full, aux, counts, P, ncols_prefix=None):
    """Cut the full-capacity class outputs down to the per-class totals in ``counts``."""
    tail = counts[P * 8:]
    if tail[6] != 0:
        raise TfrtError("trace forward: output capacity exceeded (internal error)")
    out = {
        "counts": counts[:P * 8].reshape(P, 8).copy(),
        "counts_dev": aux["counts"],
        "n_tests": int(np.uint32(tail[4])) | (int(np.uint32(tail[5])) << 32),
        # visiting-order traces: wavefronts that were no narrow bundles (done by the grouped kernel)
        "left_over": int(tail[7]),
    }
    totals = {"active": int(tail[0]), "finished": int(tail[1]), "stopped": int(tail[2]),
              "dead": int(tail[3])}
    for name, rays in full.items():
        if aux[name + "_id"] is None:
            continue
        n = min(totals[name], rays.shape[1])
        out[name] = rays[:, :n]
        if name + "_rows" in aux:   # the same rows as separate autograd outputs (see _with_rows)
            out[name + "_rows"] = _LazyRows(aux[name + "_rows"], n)
        out[name + "_id"] = aux[name + "_id"][:n]
        out[name + "_face"] = aux[name + "_face"][:n]
    n_unf = int(out["counts"][P - 1, 0]) if P > 0 else 0
    out["unfinished"] = aux["unfinished"][:, :n_unf]
    out["unfinished_id"] = aux["unfinished_id"][:n_unf]
    return out


class PendingCounts:
    """Counts of a trace whose device->host copy is still in flight (speculative slicing)."""

    def __init__(self, host, event, full, aux, P, predicted):
        self.host, self.event, self.full, self.aux, self.P = host, event, full, aux, P
        self.predicted = predicted

    def resolve(self):
        """Wait for the copy.  Returns (prediction_was_right, outputs sliced by the true counts)."""
        self.event.synchronize()
        actual = self.host.numpy().copy()
        ok = self.predicted is not None and np.array_equal(actual, self.predicted)
        return ok, actual, _slice_outputs(self.full, self.aux, actual, self.P)


def _finish_trace(full, aux, P, predicted_counts):
    """Bring the per-class counts to the host.  Without a prediction this is the trace's one
    host sync; with a prediction (the previous step's counts) the copy is left in flight, the
    outputs are cut with the predicted sizes and ``out["pending"].resolve()`` verifies later."""
    dev_counts = aux["counts"]
    host = torch.empty(dev_counts.shape, dtype=dev_counts.dtype, pin_memory=True)
    host.copy_(dev_counts, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev_counts.device))
    pending = PendingCounts(host, ev, full, aux, P, predicted_counts)
    if predicted_counts is None:
        _, actual, out = pending.resolve()
        out["raw_counts"] = actual
        return out
    out = _slice_outputs(full, aux, predicted_counts, P)
    out["raw_counts"] = predicted_counts
    out["pending"] = pending
    return out


def trace3d(src, face_verts, scene, max_passes, new_ray_length=1.0, dead_ray_length=None,
            flags=_lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED, predicted_counts=None, perm=None,
            ray_slot=None, lazy=False):
    """Run the whole 3-D trace.  ``src`` is a (6,N) ray block (f32 or f64) on the GPU.

    Returns a dict: for each class c in finished/active/stopped/dead (when compiled) the ray
    block ``c`` (6, n_c) (differentiable w.r.t. ``face_verts`` and ``src``), ``c_id`` (source
    ray index per row) and ``c_face`` (merged face hit); ``unfinished``/``unfinished_id``;
    ``counts`` (host numpy, per pass) and ``n_tests``.  One host sync (to read the counts),
    unless ``predicted_counts`` (the ``raw_counts`` of an earlier, identical-shape trace) is
    given: then nothing blocks and ``out["pending"].resolve()`` checks the prediction.

    ``perm`` (int32, N): ``src`` is ``natural[:, perm]`` -- a source handed over in a coherent
    order (``ray_order`` / ``permute_rays``; set ``scene.coherent_rays``).  Every output then comes
    back as the trace of ``natural`` itself gives it: ids in the natural numbering, every class in
    the reference's order (restored on the device inside the autograd node, gradients included;
    an in-place trace -- ``scene.in_place`` -- compacts them in that order directly, through
    ``ray_slot`` = ``inverse_order(perm)``, computed here when not handed in).

    ``lazy``: do not wait for the counts; returns ``{"finish": callable}`` instead.
    """
    opts = dict(max_passes=max_passes, new_ray_length=new_ray_length,
                dead_ray_length=dead_ray_length, flags=flags,
                zero_init=predicted_counts is not None, perm=perm, ray_slot=ray_slot, lazy=lazy)
    grad_n = lambda t: t if (isinstance(t, torch.Tensor) and t.requires_grad) else None
    outs = _Trace3D.apply(src, face_verts, grad_n(scene.n_in_arg), grad_n(scene.n_out_arg),
                          scene, opts)
    aux = opts.pop("_aux")
    compact = opts.pop("_compact", None)
    blocks, rows = _split_rows(outs, [aux[name + "_id"] is not None for name in _CLASS_NAMES], 6)
    full = dict(zip(_CLASS_NAMES, blocks))
    for name, r in rows.items():
        aux[name + "_rows"] = r
    if lazy:
        # nothing is read back here: the caller cuts the sets (one host read of the counts) when
        # somebody asks for them -- ``out["finish"]()`` returns the dict this function returns
        P = int(max_passes)

        def finish():
            if compact is not None:     # (an in-place trace that has not compacted its sets yet)
                compact()
            return _finish_trace(full, aux, P, None)
        return {"finish": finish}
    return _finish_trace(full, aux, int(max_passes), predicted_counts)


# -------------------------------------------------------------------------------- seams

def intersect3d(rays, face_verts, intersect_epsilion=1e-10, size_epsilion=1e-10,
                ray_start_epsilion=1e-10):
    """OpticalSystem3D._intersection (engine.py:1103-1166).  rays: (6,N) block."""
    _need_gpu(rays, face_verts)
    rays = rays.contiguous()
    face_verts = _c(face_verts, torch.float64)
    N, M = rays.shape[1], face_verts.shape[0]
    dev = rays.device
    L = _lib.lib()
    wsb = L.tfrt_intersect3d_workspace_bytes(N, M)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    f = lambda: torch.empty(N, dtype=torch.float64, device=dev)
    x, y, z, ray_u, trig_u, trig_v = f(), f(), f(), f(), f(), f()
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    gather = torch.empty(N, dtype=torch.int32, device=dev)
    check(L.tfrt_intersect3d(
        _p(rays), rays.shape[1], N, _DT[rays.dtype], _p(face_verts) if M else None, M,
        float(intersect_epsilion), float(size_epsilion), float(ray_start_epsilion),
        _p(x), _p(y), _p(z), _p(valid), _p(ray_u), _p(trig_u), _p(trig_v), _p(gather),
        _p(ws), wsb, _stream(rays)), "tfrt_intersect3d")
    return x, y, z, valid.bool(), ray_u, trig_u, trig_v, gather


def ray_order(rays, face_verts=None, axis=None, return_keys=False, out=None):
    """A coherent visiting order of the rays of a (6, N) block: int32 permutation in which rays
    whose lines run close together are neighbours, so that 64 consecutive entries form a narrow
    bundle (tfrt_ray_order: Hilbert keys + a stable radix sort on the device, no host sync,
    capturable).  Trace ``permute_rays(rays, order)`` (and per-ray tables in the same order) with
    ``Scene3DArgs.coherent_rays`` / ``tfrt_scene3d.coherent_rays`` set: coherent wavefronts share
    one walk of the face hierarchy (k_intersect_beam); ``restore_order(out, order)`` gives the ray
    sets of ``rays`` itself.

    Rays that mostly share a direction are ordered along a Hilbert curve through the points where
    their lines pass the middle of the scene (``face_verts`` (M, 9): the mean centroid of 64
    sampled faces; None: the mean end point of 256 sampled rays), in the plane perpendicular to
    ``axis`` (3 numbers; None: the mean direction of the sampled rays); rays without a common
    direction (an isotropic point source) along a Hilbert curve over the octahedral map of their
    directions.  ``return_keys``: also the uint32 keys (natural order, as int32 bits); the order
    equals ``argsort(keys, stable=True)``.  ``out``: an int32 tensor of N entries to write into."""
    _need_gpu(rays, face_verts)
    if rays.dtype not in _DT:
        raise TfrtError(f"ray state dtype must be float32, float64 or float16, got {rays.dtype}")
    rays = rays.detach()
    if rays.stride(1) != 1:
        rays = rays.contiguous()
    N = rays.shape[1]
    dev = rays.device
    L = _lib.lib()
    perm = out if out is not None else torch.empty(N, dtype=torch.int32, device=dev)
    if perm.dtype != torch.int32 or perm.numel() != N or not perm.is_contiguous():
        raise TfrtError("ray_order: `out` must be a contiguous int32 tensor of N entries")
    keys = torch.empty(N, dtype=torch.int32, device=dev) if return_keys else None
    if N:
        fv = None if face_verts is None else _c(face_verts.detach(), torch.float64)
        wsb = L.tfrt_ray_order_workspace_bytes(N)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        ax = None if axis is None else (ctypes.c_double * 3)(*[float(v) for v in axis])
        check(L.tfrt_ray_order(_p(rays), rays.stride(0), N, _DT[rays.dtype], _p(fv),
                               0 if fv is None else fv.shape[0], ax, _p(perm), _p(keys), _p(ws),
                               wsb, _stream(rays)), "tfrt_ray_order")
    return (perm, keys) if return_keys else perm


def inverse_order(perm):
    """``inv`` with ``inv[perm[j]] = j`` (int32): where the caller's ray r sits in a block that was
    permuted with ``perm`` -- tfrt_scene3d.ray_slot.  (Not cached here: an order tensor is
    re-written in place by tfrt_ray_order / tfrt_source3d_order without a version bump; the
    engine keeps the inverse next to the order it belongs to.)"""
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
    return inv


def wave_groups(n_rays):
    """Entries of a wavefront schedule for ``n_rays`` rays: the groups of 64 consecutive rays."""
    return (int(n_rays) + 63) // 64


def wave_schedule(n_rays, n_faces, max_passes, state_dtype, workspace, out=None):
    """The wavefront schedule for the next in-place traces of the rays whose trace left its tape in
    ``workspace`` (tfrt_trace3d_wave_schedule; tfrt_scene3d.wave_schedule): int32, the groups of 64
    rays by cost class, the heaviest class first.  ``state_dtype``: the ray block's torch dtype;
    ``out``: an int32 tensor of ``wave_groups(n_rays)`` entries to write into."""
    _need_gpu(workspace, out)
    G = wave_groups(n_rays)
    if out is None:
        out = torch.empty(G, dtype=torch.int32, device=workspace.device)
    if out.dtype != torch.int32 or out.numel() != G or not out.is_contiguous():
        raise TfrtError("wave_schedule: `out` must be a contiguous int32 tensor of ceil(N / 64) entries")
    check(_lib.lib().tfrt_trace3d_wave_schedule(
        n_rays, n_faces, max_passes, _DT[state_dtype], _p(workspace), workspace.numel(), _p(out),
        _stream(workspace)), "tfrt_trace3d_wave_schedule")
    return out


def wave_rows(n_rays, n_faces, max_passes, state_dtype, workspace):
    """The per-wavefront count rows ``wave_schedule`` reads (tfrt_trace3d_wave_rows): int32 tensor
    (max_passes + 2, W) of uint32 bits, W the wavefronts of the trace."""
    _need_gpu(workspace)
    L = _lib.lib()
    args = (n_rays, n_faces, max_passes, _DT[state_dtype], _p(workspace), workspace.numel())
    W = L.tfrt_trace3d_wave_rows(*args, None, None)
    if W < 0:
        check(W, "tfrt_trace3d_wave_rows")
    rows = torch.empty((max_passes + 2, W), dtype=torch.int32, device=workspace.device)
    code = L.tfrt_trace3d_wave_rows(*args, _p(rows), _stream(workspace))
    if code < 0:
        check(code, "tfrt_trace3d_wave_rows")
    return rows


def check_wave_schedule(schedule, n_rays):
    """Refuses a caller's wavefront schedule unless it is a contiguous int32 device tensor holding a
    permutation of ``range(wave_groups(n_rays))`` -- a group that is missing would not be traced.
    Checked by sorting (one host read), before anything is launched with it."""
    G = wave_groups(n_rays)
    if not isinstance(schedule, torch.Tensor) or schedule.dtype != torch.int32:
        raise TfrtError("wave_schedule must be an int32 tensor")
    _need_gpu(schedule)
    if schedule.dim() != 1 or schedule.numel() != G or not schedule.is_contiguous():
        raise TfrtError(f"wave_schedule must hold {G} entries (one per 64 rays), "
                        f"got shape {tuple(schedule.shape)}")
    want = torch.arange(G, dtype=torch.int32, device=schedule.device)
    if not torch.equal(torch.sort(schedule).values, want):
        raise TfrtError(f"wave_schedule must be a permutation of range({G})")
    return schedule


def permute_rays(rays, index, out=None):
    """``rays[:, index]`` of a (6, N) ray block (tfrt_permute_rays)."""
    _need_gpu(rays, index)
    rays = rays.detach()
    if rays.stride(1) != 1:
        rays = rays.contiguous()
    N = rays.shape[1]
    if index.dtype != torch.int32 or index.numel() != N:
        raise TfrtError("permute_rays: index must be an int32 permutation of the N rays")
    if out is None:
        out = torch.empty((6, N), dtype=rays.dtype, device=rays.device)
    if N:
        L = _lib.lib()
        wsb = L.tfrt_permute_rays_workspace_bytes(N, _DT[rays.dtype])
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=rays.device)
        check(L.tfrt_permute_rays(_p(rays), rays.stride(0), N, _DT[rays.dtype], _p(index), _p(out),
                                  out.stride(0), _p(ws), wsb, _stream(rays)), "tfrt_permute_rays")
    return out


def gather_rows(src, index, n_valid=None, out=None):
    """``src[..., index]`` for a (k, n) or (n,) tensor of 1/2/4/8-byte elements through an int32
    index (tfrt_gather_rows); ``n_valid``: int32 device scalar, entries beyond it are left alone."""
    _need_gpu(src, index)
    src = src.detach()
    one = src.dim() == 1
    s2 = src.reshape(1, -1) if one else src
    if s2.stride(1) != 1:
        s2 = s2.contiguous()
    k, n = s2.shape[0], index.numel()
    if out is None:
        out = torch.empty((k, n), dtype=src.dtype, device=src.device)
    o2 = out.reshape(1, -1) if out.dim() == 1 else out
    if n and k:
        check(_lib.lib().tfrt_gather_rows(_p(s2), s2.stride(0), k, s2.element_size(), _p(index), n,
                                          _p(n_valid), _p(o2), o2.stride(0), _stream(src)),
              "tfrt_gather_rows")
    return out.reshape(-1) if (one and out.dim() == 2) else out


def _check_field_codes(what, rows, row_x, row_y, dimension):
    """``dimension`` None: ``row_x`` / ``row_y`` are rows of the (k, n) block ``rows``; given:
    ``rows`` is the (2 * dimension, n) geometry block and they are field codes
    (tfrt_density_error_fields).  The C entries bound a code by a constant, not by the block."""
    top, noun = rows.shape[0], "rows"
    if dimension is not None:
        if dimension not in (2, 3):
            raise ValueError(f"{what}: dimension must be None, 2 or 3, got {dimension!r}")
        if rows.shape[0] != 2 * dimension:
            raise ValueError(f"{what}: a {dimension}-D geometry block has {2 * dimension} rows, "
                             f"got {rows.shape[0]}")
        top, noun = 3 * dimension, "field codes"
    if not (0 <= row_x < top and -1 <= row_y < top and row_x != row_y):
        raise ValueError(f"{what}: {noun} must be distinct and lie in [0, {top}), got "
                         f"{row_x}, {row_y}")


def _column_buffers(what, rows, grad, err, mask=None, perm=None):
    """What the column errors (density_error, spot_error, transport_error, goal_error_columns)
    ask of their per-column arguments, for the (k, n) block ``rows``: ``mask`` and ``perm``, where
    given, contiguous int32 with at least n entries; ``grad`` float64 (k, at least n), zeros made
    here by default; ``err`` three float64.  Returns (grad, err)."""
    k, n = rows.shape
    for name, index in (("mask", mask), ("perm", perm)):
        if index is not None and (index.dtype != torch.int32 or index.numel() < n
                                  or not index.is_contiguous()):
            raise ValueError(f"{what}: {name} must be contiguous int32, one entry per column")
    if grad is None:
        grad = torch.zeros((k, n), dtype=torch.float64, device=rows.device)
    elif grad.dtype != torch.float64 or grad.dim() != 2 or grad.shape[0] != k or grad.shape[1] < n:
        raise ValueError(f"{what}: grad must be float64 ({k}, {n})")
    if err is None:
        err = torch.empty(3, dtype=torch.float64, device=rows.device)
    return grad, err


def _column_workspace(what, rows, grad, workspace, workspace_bytes, *tensors):
    """The GPU path's share of the same: every tensor on the device, ``rows`` and ``grad`` with
    contiguous columns, and the ``workspace`` given or one of ``workspace_bytes()`` bytes."""
    _need_gpu(rows, grad, *tensors)
    if (rows.shape[1] > 0 and rows.stride(1) != 1) or (grad.shape[1] > 0 and grad.stride(1) != 1):
        raise ValueError(f"{what}: rows and grad must have contiguous columns")
    if workspace is None:
        workspace = torch.empty(max(workspace_bytes(), 1), dtype=torch.uint8, device=rows.device)
    return workspace


def _link_torch(rows, dim):
    """(start, end, d, L, ok) of the columns' last links, the operations of
    tfrt_density_error_fields one by one."""
    s, e = rows[:dim].double(), rows[dim:2 * dim].double()
    v = e - s
    q = v[0] * v[0] + v[1] * v[1]
    if dim == 3:
        q = q + v[2] * v[2]
    # (numpy's sqrt on the CPU, as tests/direction_fields_reference.py uses: torch 2.10's CPU sqrt
    # differed from it in the last bit of 11 of the 1,000 lengths of that file's ``rays(1000)``,
    # and L has to agree with the kernels' bit for bit)
    L = torch.sqrt(q) if q.is_cuda else torch.from_numpy(np.sqrt(q.numpy()))
    ok = torch.isfinite(s).all(dim=0) & torch.isfinite(e).all(dim=0) & torch.isfinite(L) & (L > 0)
    return s, e, v / L, L, ok


def _link_field_torch(link, code, dim):
    s, e, d, _, ok = link
    v = s[code] if code < dim else (e[code - dim] if code < 2 * dim else d[code - 2 * dim])
    return torch.where(ok, v, torch.full((), float("nan"), dtype=torch.float64))


def _chain_cpu(grad, n, dim, row_x, row_y, gx, gy, link, counts):
    """All 2 * dim rows of ``grad`` from gx, gy (the chain rule of tfrt_density_error_fields, in
    its operation order); zeros where ``counts`` is false."""
    _, _, d, L, _ = link
    two = row_y >= 0
    ax, ay = row_x - 2 * dim, (row_y - 2 * dim if two else -1)
    t = gx * d[ax] if ax >= 0 else None
    if ay >= 0:
        t = gy * d[ay] if t is None else t + gy * d[ay]
    zero = torch.zeros((), dtype=torch.float64)
    for b in range(dim):
        gvb = gx if ax == b else (gy if ay == b else torch.zeros_like(gx))
        G = (gvb - t * d[b]) / L
        start, end = -G, G
        if row_x == b:
            start = start + gx
        if two and row_y == b:
            start = start + gy
        if row_x == dim + b:
            end = end + gx
        if two and row_y == dim + b:
            end = end + gy
        grad[b, :n] = torch.where(counts, start, zero)
        grad[dim + b, :n] = torch.where(counts, end, zero)


def _fields_cpu(rows, row_x, row_y, dimension):
    """(x, y, link) of the columns on the CPU: the float64 fields (y: zeros with one field) and,
    with a direction field, the ``_link_torch`` of the block that ``_chain_cpu`` needs (else None:
    plain rows)."""
    two = row_y >= 0
    if dimension is not None and max(row_x, row_y) >= 2 * dimension:
        link = _link_torch(rows, dimension)
        x = _link_field_torch(link, row_x, dimension)
        y = _link_field_torch(link, row_y, dimension) if two else torch.zeros_like(x)
        return x, y, link
    x = rows[row_x].double()
    return x, (rows[row_y].double() if two else torch.zeros_like(x)), None


def _outside_cpu(x, y, two, grid, oob, counts, w):
    """The columns of ``counts`` outside the closed domain of ``grid``: returns (inside, pen, gx,
    gy) -- the mask of the columns inside, the sum of the penalties ``oob * (ex**2 + ey**2)`` with
    ``ex = max(x0 - x, 0) + max(x - x1, 0)``, and their derivatives, zero where a column is not
    outside (gy: None with one field).  ``w``: a weight per column or None; penalty and derivative
    are multiplied by it last."""
    x0, x1, _, y0, y1, _ = grid
    out = (x < x0) | (x > x1)
    if two:
        out |= (y < y0) | (y > y1)
    inside, outside = counts & ~out, counts & out
    zero = torch.zeros((), dtype=torch.float64)
    ex = torch.maximum(x0 - x, zero) + torch.maximum(x - x1, zero)
    ey = (torch.maximum(y0 - y, zero) + torch.maximum(y - y1, zero)) if two else torch.zeros_like(x)
    pens = oob * (ex * ex + ey * ey)
    gx = oob * (2.0 * ex) * ((x > x1).double() - (x < x0).double())
    gy = oob * (2.0 * ey) * ((y > y1).double() - (y < y0).double()) if two else None
    if w is not None:
        pens, gx = pens * w, gx * w
        gy = gy * w if two else None
    pen = pens[outside].sum()
    gx = torch.where(outside, gx, zero)
    gy = torch.where(outside, gy, zero) if two else None
    return inside, pen, gx, gy


def _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, counts):
    """The gradient rows from gx, gy: the chain rule onto all 2 * dimension rows with a direction
    field (``link`` given; zeros where ``counts`` is false), else the fields' own rows."""
    if link is not None:
        _chain_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, counts)
    else:
        grad[row_x, :n] = gx
        if row_y >= 0:
            grad[row_y, :n] = gy


DENSITY_FIXED_ONE = 4294967296.0      # 2^32: one ray's total weight in the int64 histogram
DENSITY_MAX_BINS = 65536


def density_grid(domain, nx, ny=None):
    """The domain constants tfrt_density_error takes, (x0, x1, sx, y0, y1, sy) in float64 with
    sx = nx / (x1 - x0) computed once here; one axis: the y constants are 0."""
    (x0, x1) = (float(v) for v in domain[0])
    sx = float(np.float64(nx) / (np.float64(x1) - np.float64(x0)))
    if ny is None:
        return (x0, x1, sx, 0.0, 0.0, 0.0)
    (y0, y1) = (float(v) for v in domain[1])
    return (x0, x1, sx, y0, y1, float(np.float64(ny) / (np.float64(y1) - np.float64(y0))))


def _check_weights(what, weights):
    """``weights``: contiguous float64, one per SOURCE ray."""
    if weights.dtype != torch.float64 or weights.dim() != 1 or not weights.is_contiguous():
        raise ValueError(f"{what}: weights must be a contiguous float64 vector, one weight per "
                         "source ray")


def _source_weights(weights, perm, n):
    """(w, ok) per column on the CPU: the weight of column i's source ray ``perm[i]`` (``i``
    without perm) and whether it counts -- the source ray exists, w is finite and in [0, 1]."""
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < weights.numel())
    w = torch.zeros(n, dtype=torch.float64)
    w[s_ok] = weights[s[s_ok]]
    return w, s_ok & (w >= 0.0) & (w <= 1.0)


def density_error(rows, row_x, row_y, goal, grid, oob_weight=0.0, mask=None, grad=None, err=None,
                  hq=None, workspace=None, variant=0, dimension=None, weights=None, perm=None,
                  n_source=None):
    """tfrt_density_error: the DensityError of the columns of ``rows`` (k, n), x in row ``row_x``
    and y in row ``row_y`` (-1: one field), against the L2-normalised float64 ``goal`` (ny, nx) or
    (nx,); ``grid`` from ``density_grid``; ``mask``: optional int32, column i counts if
    mask[i] >= 0.  Returns (err {sum, 1, mean}, grad (k, n) float64, hq int64 of the goal's
    shape): rows ``row_x`` / ``row_y`` of ``grad`` are written for every column, other rows only
    when ``grad`` is made here (zeros).  ``grad``, ``err``, ``hq``, ``workspace`` (uint8): buffers
    to reuse -- with all four given a CUDA call allocates nothing.  ``row_x`` / ``row_y`` must be
    distinct rows of the block; a ValueError otherwise, before anything is launched.

    ``dimension`` 2 or 3 (tfrt_density_error_fields): ``rows`` is the (2 * dimension, n) geometry
    block of the finished rays (start rows, then end rows) and ``row_x`` / ``row_y`` are FIELD
    CODES: below 2 * dimension a row of the block, from there on the direction cosines of the last
    link (3-D: x_dir, y_dir, z_dir = 6, 7, 8; 2-D: x_dir, y_dir = 4, 5).  With a direction field
    all 2 * dimension rows of ``grad`` are written (the chain rule back onto start and end).

    ``weights`` (tfrt_density_error_weighted): contiguous float64, one radiant power in [0, 1] per
    SOURCE ray (``n_source`` of them, default all); ``perm``: optional int32 (n,), the source ray
    of column i (None: column i is source ray i).  A column without a source ray, or whose weight
    is not finite or not in [0, 1], does not count; every bilinear weight, the gradient and the
    penalty are multiplied by the ray's weight last.  On return the first nx * ny float64 of a
    ``workspace`` given hold the pulls D (on the CPU path too).

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64
    fixed-point histogram and the same operation order per ray (``hq`` and the per-ray quantities
    agree bit for bit; the sums over bins are torch's and agree to rounding)."""
    two = row_y >= 0
    nx = goal.shape[-1]
    ny = goal.shape[0] if goal.dim() == 2 else 1
    if goal.dtype != torch.float64 or not goal.is_contiguous() or goal.dim() != (2 if two else 1):
        raise ValueError("density_error: goal must be contiguous float64, (ny, nx) for two fields "
                         "and (nx,) for one")
    if nx * ny > DENSITY_MAX_BINS:
        raise ValueError(f"density_error: more than {DENSITY_MAX_BINS} bins")
    n = rows.shape[1]
    _check_field_codes("density_error", rows, row_x, row_y, dimension)
    if weights is not None:
        _check_weights("density_error", weights)
        n_source = weights.numel() if n_source is None else int(n_source)
        if not 0 <= n_source <= weights.numel():
            raise ValueError("density_error: n_source exceeds the weights given")
    # (the source ray of a column is looked up for its weight only)
    grad, err = _column_buffers("density_error", rows, grad, err, mask,
                                perm if weights is not None else None)
    if hq is None:
        hq = torch.empty(goal.shape, dtype=torch.int64, device=rows.device)
    x0, x1, sx, y0, y1, sy = grid
    if not rows.is_cuda:
        _density_error_cpu(rows, row_x, row_y, goal, grid, float(oob_weight), mask, grad, err, hq,
                           dimension, None if weights is None else weights[:n_source], perm,
                           None if workspace is None
                           else workspace[:8 * nx * ny].view(torch.float64))
        return err, grad, hq
    L = _lib.lib()
    workspace = _column_workspace(
        "density_error", rows, grad, workspace,
        lambda: L.tfrt_density_error_workspace_bytes(n, nx, ny), goal, mask, err, hq, weights, perm)
    if weights is not None:
        # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
        check(L.tfrt_density_error_weighted(
            _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
            _p(mask), row_x, row_y, _p(goal), _p(weights), n_source, _p(perm), nx, ny, x0, x1, sx,
            y0, y1, sy, float(oob_weight), _p(grad), grad.stride(0), _p(err), _p(hq), int(variant),
            _p(workspace), workspace.numel(), _stream(rows)), "tfrt_density_error_weighted")
        return err, grad, hq
    if dimension is not None:
        check(L.tfrt_density_error_fields(
            _p(rows), rows.stride(0), n, _DT[rows.dtype], int(dimension), _p(mask), row_x, row_y,
            _p(goal), nx, ny, x0, x1, sx, y0, y1, sy, float(oob_weight), _p(grad), grad.stride(0),
            _p(err), _p(hq), int(variant), _p(workspace), workspace.numel(), _stream(rows)),
            "tfrt_density_error_fields")
        return err, grad, hq
    check(L.tfrt_density_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], _p(mask), row_x, row_y, _p(goal), nx, ny,
        x0, x1, sx, y0, y1, sy, float(oob_weight), _p(grad), grad.stride(0), _p(err), _p(hq),
        int(variant), _p(workspace), workspace.numel(), _stream(rows)), "tfrt_density_error")
    return err, grad, hq


def _density_axis(v, lo, scale, nb):
    u = (v - lo) * scale - 0.5
    f = torch.floor(u)
    i0 = f.long()
    return i0.clamp(0, nb - 1), (i0 + 1).clamp(0, nb - 1), u - f


def _density_error_cpu(rows, row_x, row_y, goal, grid, oob, mask, grad, err, hq, dimension=None,
                       weights=None, perm=None, pull=None):
    """The CPU path of ``density_error`` (every torch op rounds on its own, as the kernels do);
    ``pull``: nx * ny float64 that receive the pulls D."""
    x0, x1, sx, y0, y1, sy = grid
    two = row_y >= 0
    nx = goal.shape[-1]
    n = rows.shape[1]
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counts = torch.isfinite(x) & torch.isfinite(y)
    if mask is not None:
        counts &= mask[:n] >= 0
    w = None
    if weights is not None:
        w, w_ok = _source_weights(weights, perm, n)
        counts &= w_ok
    # outside: the penalty and its derivative (weighted: each times w last)
    inside, pen, gx, gy = _outside_cpu(x, y, two, grid, oob, counts, w)
    # inside: the fixed-point histogram
    xi, yi = x[inside], y[inside]
    wi = w[inside] if w is not None else None
    ia, ib, tx = _density_axis(xi, x0, sx, nx)
    flat = hq.view(-1)
    flat.zero_()

    def splat(index, b):
        if wi is not None:
            b = b * wi
        flat.index_add_(0, index, torch.round(b * DENSITY_FIXED_ONE).long())
    if two:
        ja, jb, ty = _density_axis(yi, y0, sy, goal.shape[0])
        wx0, wx1, wy0, wy1 = 1.0 - tx, tx, 1.0 - ty, ty
        splat(ja * nx + ia, wy0 * wx0)
        splat(ja * nx + ib, wy0 * wx1)
        splat(jb * nx + ia, wy1 * wx0)
        splat(jb * nx + ib, wy1 * wx1)
    else:
        splat(ia, 1.0 - tx)
        splat(ib, tx)
    H = flat.double() / DENSITY_FIXED_ONE
    g = goal.reshape(-1)
    s = torch.sqrt((H * H).sum())
    if float(s) == 0.0:
        e_hist, D = (g * g).sum(), torch.zeros_like(H)
    else:
        h = H / s
        r = h - g
        e_hist = (r * r).sum()
        D = (2.0 / s) * (r - h * (h * r).sum())
    if pull is not None:
        pull.copy_(D)
    if two:
        d00, d01, d10, d11 = D[ja * nx + ia], D[ja * nx + ib], D[jb * nx + ia], D[jb * nx + ib]
        gxi = sx * ((1.0 - ty) * (d01 - d00) + ty * (d11 - d10))
        gyi = sy * ((1.0 - tx) * (d10 - d00) + tx * (d11 - d01))
        gy[inside] = gyi if wi is None else gyi * wi
    else:
        gxi = sx * (D[ib] - D[ia])
    gx[inside] = gxi if wi is None else gxi * wi
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, counts)
    e = e_hist + pen
    err[0], err[1], err[2] = e, 1.0, e


TRANSPORT_KEY_BITS = 26               # transport_math.h: two 13-bit digits of the radix sort
TRANSPORT_KEY_INVALID = (1 << TRANSPORT_KEY_BITS) - 1
TRANSPORT_MAX_DIRECTIONS = 64
TRANSPORT_MAX_KNOTS = 65536
TRANSPORT_SUBCELLS = 4                # sub-points per goal bin and axis of the quantile tables


def transport_directions(directions, n_fields=2):
    """The (K, 2) float64 array of (cos, sin) of a TransportError's projection angles, computed
    once here: an int K means the angles pi * k / K, k = 0 .. K-1; an array gives them.  One field:
    the single direction (1, 0)."""
    if n_fields == 1:
        return np.array([[1.0, 0.0]], dtype=np.float64)
    if np.ndim(directions) == 0:
        if isinstance(directions, (bool, np.bool_)) or int(directions) != directions:
            raise ValueError(f"transport_directions: a direction count must be an integer, got "
                             f"{directions!r}")
        k = int(directions)
        if not 1 <= k <= TRANSPORT_MAX_DIRECTIONS:
            raise ValueError(f"transport_directions: 1 .. {TRANSPORT_MAX_DIRECTIONS} directions, "
                             f"got {k}")
        theta = np.pi * np.arange(k, dtype=np.float64) / np.float64(k)
    else:
        theta = np.asarray(directions, dtype=np.float64)
        if theta.ndim != 1 or not 1 <= theta.size <= TRANSPORT_MAX_DIRECTIONS \
                or not np.isfinite(theta).all():
            raise ValueError(f"transport_directions: 1 .. {TRANSPORT_MAX_DIRECTIONS} finite "
                             f"angles, got {directions!r}")
    return np.stack([np.cos(theta), np.sin(theta)], axis=1)


def transport_tables(goal, domain, angles, knots):
    """The quantile tables of a TransportError, (K, Q + 1) numpy float64, in the normalised
    coordinates of ``domain`` (whose extents therefore do not enter: only one (lo, hi) per field
    is asked for).  ``goal``: non-negative (ny, nx) or (nx,); ``angles``: the (K, 2) (cos, sin) of
    ``transport_directions``; ``knots``: Q.  Every bin is split into 4 x 4 sub-points (4 with one
    field) at the sub-cells' centres, each with the bin's mass; empty ones are dropped; per
    direction the projections ``p = c * xi + s * eta`` (one field: ``xi``) are sorted stably,
    ``cm = (cumsum(w) - w / 2) / sum(w)``, and ``T = np.interp(arange(Q + 1) / Q, cm, p_sorted)``:
    non-decreasing by construction."""
    g = np.asarray(goal, dtype=np.float64)
    cs = np.asarray(angles, dtype=np.float64).reshape(-1, 2)
    q = int(knots)
    if g.ndim not in (1, 2) or g.ndim != len(domain):
        raise ValueError("transport_tables: goal must be (ny, nx) with two domain axes or (nx,) "
                         "with one")
    if not 2 <= q <= TRANSPORT_MAX_KNOTS:
        raise ValueError(f"transport_tables: 2 .. {TRANSPORT_MAX_KNOTS} knots, got {knots!r}")
    if not np.isfinite(g).all() or (g < 0).any() or not (g > 0).any():
        raise ValueError("transport_tables: goal must be finite, non-negative and not all zero")
    sub = TRANSPORT_SUBCELLS
    nx = g.shape[-1]
    xi = (np.arange(nx * sub, dtype=np.float64) + 0.5) / np.float64(nx * sub)
    if g.ndim == 2:
        ny = g.shape[0]
        eta = (np.arange(ny * sub, dtype=np.float64) + 0.5) / np.float64(ny * sub)
        w = np.repeat(np.repeat(g, sub, axis=0), sub, axis=1).reshape(-1)
        xi, eta = np.tile(xi, ny * sub), np.repeat(eta, nx * sub)
    else:
        w = np.repeat(g, sub)
        eta = np.zeros_like(xi)
        cs = np.array([[1.0, 0.0]])
    keep = w > 0
    xi, eta, w = xi[keep], eta[keep], w[keep]
    at = np.arange(q + 1, dtype=np.float64) / np.float64(q)
    tables = np.empty((cs.shape[0], q + 1), dtype=np.float64)
    for k, (c, s) in enumerate(cs):
        p = c * xi + s * eta if g.ndim == 2 else xi
        order = np.argsort(p, kind="stable")
        ws = w[order]
        cm = (np.cumsum(ws) - ws / 2.0) / ws.sum()
        tables[k] = np.interp(at, cm, p[order])
    return tables


def transport_grid(domain):
    """The domain constants tfrt_transport_error takes, (x0, ix, y0, iy) in float64 with
    ix = 1 / (x1 - x0) computed once here; one axis: the y constants are 0."""
    (x0, x1) = (float(v) for v in domain[0])
    ix = float(np.float64(1.0) / (np.float64(x1) - np.float64(x0)))
    if len(domain) == 1:
        return (x0, ix, 0.0, 0.0)
    (y0, y1) = (float(v) for v in domain[1])
    return (x0, ix, y0, float(np.float64(1.0) / (np.float64(y1) - np.float64(y0))))


def transport_error(rows, row_x, row_y, tables, grid, angles, mask=None, dimension=None,
                    grad=None, err=None, rank2=None, workspace=None):
    """tfrt_transport_error: the TransportError of the columns of ``rows`` (k, n), x in row
    ``row_x`` and y in row ``row_y`` (-1: one field, one direction).  ``tables``: contiguous
    float64 (K, Q + 1) from ``transport_tables``; ``grid`` from ``transport_grid``; ``angles``:
    contiguous float64 (K, 2), the (cos, sin) of ``transport_directions``; both on the device of
    ``rows``.  ``mask``: optional int32, column i counts if mask[i] >= 0.  ``dimension`` 2 or 3:
    ``rows`` is the (2 * dimension, n) geometry block (position rows only); None: any block of up
    to six rows.  Returns (err {sum, K * n_valid, mean}, grad (k, n) float64, rank2 (K, n) int32:
    2 * first + count of every column, -1 where it does not count): rows ``row_x`` / ``row_y`` of
    ``grad`` are written for every column, other rows only when ``grad`` is made here (zeros).
    ``grad``, ``err``, ``rank2``, ``workspace`` (uint8): buffers to reuse -- with all four given a
    CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same keys, the
    same ranks and the same operation order per ray (``rank2`` and the gradient agree bit for
    bit; the error sum is torch's and agrees to rounding)."""
    two = row_y >= 0
    if tables.dtype != torch.float64 or tables.dim() != 2 or not tables.is_contiguous() \
            or angles.dtype != torch.float64 or tuple(angles.shape) != (tables.shape[0], 2) \
            or not angles.is_contiguous():
        raise ValueError("transport_error: tables must be contiguous float64 (K, Q + 1) and "
                         "angles contiguous float64 (K, 2)")
    K, Q = tables.shape[0], tables.shape[1] - 1
    if not (1 <= K <= TRANSPORT_MAX_DIRECTIONS and 2 <= Q <= TRANSPORT_MAX_KNOTS) \
            or (not two and K != 1):
        raise ValueError(f"transport_error: 1 .. {TRANSPORT_MAX_DIRECTIONS} directions (one with "
                         f"one field) and 2 .. {TRANSPORT_MAX_KNOTS} knots, got {K} and {Q}")
    k, n = rows.shape
    top = k if dimension is None else 2 * dimension
    if dimension is not None and (dimension not in (2, 3) or k != 2 * dimension):
        raise ValueError(f"transport_error: dimension must be None, 2 or 3 with a block of "
                         f"2 * dimension rows, got {dimension!r} and {k} rows")
    if k > 6 or not (0 <= row_x < top and -1 <= row_y < top and row_x != row_y):
        raise ValueError(f"transport_error: rows must be distinct position rows in [0, {top}), "
                         f"got {row_x}, {row_y}")
    grad, err = _column_buffers("transport_error", rows, grad, err, mask)
    if rank2 is None:
        rank2 = torch.empty((K, n), dtype=torch.int32, device=rows.device)
    if rank2.dtype != torch.int32 or tuple(rank2.shape) != (K, n) or not rank2.is_contiguous():
        raise ValueError(f"transport_error: rank2 must be contiguous int32 ({K}, {n})")
    if not rows.is_cuda:
        _transport_error_cpu(rows, row_x, row_y, tables, grid, angles, mask, grad, err, rank2)
        return err, grad, rank2
    L = _lib.lib()
    workspace = _column_workspace(
        "transport_error", rows, grad, workspace,
        lambda: L.tfrt_transport_error_workspace_bytes(n, K), tables, angles, mask, err, rank2)
    x0, ix, y0, iy = grid
    check(L.tfrt_transport_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
        _p(mask), row_x, row_y, x0, ix, y0, iy, _p(angles), _p(tables), Q, K, _p(grad),
        grad.stride(0), _p(err), _p(rank2), _p(workspace), workspace.numel(), _stream(rows)),
        "tfrt_transport_error")
    return err, grad, rank2


def _transport_error_cpu(rows, row_x, row_y, tables, grid, angles, mask, grad, err, rank2):
    """The CPU path of ``transport_error`` (every torch op rounds on its own, as the kernels
    do)."""
    x0, ix, y0, iy = grid
    two = row_y >= 0
    n = rows.shape[1]
    K, Q = tables.shape[0], tables.shape[1] - 1
    x = rows[row_x].double()
    y = rows[row_y].double() if two else torch.zeros_like(x)
    counts = torch.isfinite(x) & torch.isfinite(y)
    if mask is not None:
        counts &= mask[:n] >= 0
    nv = int(counts.sum())
    xi = (x - x0) * ix
    eta = (y - y0) * iy if two else torch.zeros_like(x)
    zero = torch.zeros((), dtype=torch.float64)
    top = float(TRANSPORT_KEY_INVALID - 1)
    gx, gy = torch.zeros_like(x), torch.zeros_like(x)
    total = torch.zeros((), dtype=torch.float64)
    for k in range(K):
        c, s = (float(v) for v in angles[k]) if two else (1.0, 0.0)
        a, b = min(0.0, c) + min(0.0, s), max(0.0, c) + max(0.0, s)
        lo = a - (b - a)
        scale = float(1 << TRANSPORT_KEY_BITS) / (3.0 * (b - a))
        p = c * xi + s * eta if two else xi
        v = torch.floor((p - lo) * scale)
        key = torch.where(v >= 0.0, torch.clamp(v, max=top), zero).long()
        key = torch.where(counts, key, torch.full_like(key, TRANSPORT_KEY_INVALID))
        sk = torch.sort(key).values
        first = torch.searchsorted(sk, key, right=False)
        last = torch.searchsorted(sk, key, right=True)
        r2 = torch.where(counts, first + last, torch.full_like(first, -1))
        rank2[k] = r2.to(torch.int32)
        if nv == 0:
            continue
        u = (r2.double() * 0.5) / float(nv)
        z = u * float(Q)
        fm = torch.clamp(torch.floor(z), min=0.0, max=float(Q - 1))
        m = fm.long()
        f = z - fm
        T = tables[k]
        t0 = T[m]
        t = t0 + f * (T[m + 1] - t0)
        d = torch.where(counts, p - t, zero)
        total = total + (d * d).sum()
        gx = gx + ((2.0 * d) * c) * ix
        gy = gy + ((2.0 * d) * s) * iy
    grad[row_x, :n] = gx
    if two:
        grad[row_y, :n] = gy
    terms = float(K * nv)
    err[0], err[1] = total, terms
    err[2] = total / terms if terms > 0 else float("nan")


SPOT_MAX_GROUPS = 1 << 20
SPOT_LDS_GROUPS = 1024
SPOT_MAX_GRID = 512                # workgroups of the accumulate launch (spot_records.h) ...
SPOT_RAYS_PER_BLOCK = 4 * 256      # ... one per that many columns
DISTORTION_SEED_MAX_GRID = 2048    # workgroups of 256 lanes of k_distortion_seed (residual_seed.h)
SPOT_WEIGHTED_LDS_GROUPS = 512     # tfrt_spot_error_weighted: six planes, the same 24 KiB
SPOT_MAX_WBITS = 20


def spot_qbits(n_source):
    """Fraction bits of tfrt_spot_error's fixed point for a source of ``n_source`` rays:
    n_source * 2^qbits < 2^62, at most 52."""
    return min(52, 62 - int(n_source).bit_length())


def spot_wbits(n_source):
    """Fraction bits of tfrt_spot_error_weighted's quantised weight for a source of ``n_source``
    rays: n_source * 2^wbits * 2^ceil(qbits / 2) < 2^62 with ``qbits = spot_qbits(n_source)``, at
    most 20."""
    qbits = spot_qbits(n_source)
    return min(SPOT_MAX_WBITS, 62 - int(n_source).bit_length() - (qbits + 1) // 2)


def spot_grid(domain, qbits):
    """The domain constants tfrt_spot_error takes, (x0, x1, qsx, y0, y1, qsy) in float64 with
    qsx = 2^qbits / (x1 - x0) computed once here; one axis: the y constants are 0."""
    one = float(np.ldexp(1.0, int(qbits)))
    (x0, x1) = (float(v) for v in domain[0])
    qsx = float(np.float64(one) / (np.float64(x1) - np.float64(x0)))
    if len(domain) == 1:
        return (x0, x1, qsx, 0.0, 0.0, 0.0)
    (y0, y1) = (float(v) for v in domain[1])
    return (x0, x1, qsx, y0, y1, float(np.float64(one) / (np.float64(y1) - np.float64(y0))))


def spot_error(rows, row_x, row_y, group, n_groups, grid, oob_weight=0.0, mask=None, perm=None,
               grad=None, err=None, acc=None, variant=0, workspace=None, qbits=None,
               dimension=None, weights=None, wbits=None):
    """tfrt_spot_error: the SpotError of the columns of ``rows`` (k, n), x in row ``row_x`` and y
    in row ``row_y`` (-1: one field).  ``group``: contiguous int32 labels, one per SOURCE ray;
    ``perm``: optional int32 (n,), the source ray of column i (None: column i is source ray i);
    ``n_groups``: G, labels outside [0, G) belong to no spot; ``grid`` from ``spot_grid`` with the
    same ``qbits`` (None: ``spot_qbits(group.numel())``); ``mask``: optional int32, column i
    counts if mask[i] >= 0.  Returns (err {sum, terms, mean}, grad (k, n) float64, acc (G, 4)
    int64 {count, Sx, Sy, 0}): rows ``row_x`` / ``row_y`` of ``grad`` are written for every column,
    other rows only when ``grad`` is made here (zeros).  ``grad``, ``err``, ``acc``, ``workspace``
    (uint8): buffers to reuse -- with all four given a CUDA call allocates nothing.

    ``dimension`` 2 or 3 (tfrt_spot_error_fields): ``rows`` is the (2 * dimension, n) geometry
    block and ``row_x`` / ``row_y`` are FIELD CODES, as for ``density_error``; with a direction
    field all 2 * dimension rows of ``grad`` are written and the centroids are mean direction
    cosines.

    ``weights`` (tfrt_spot_error_weighted): contiguous float64, one radiant power in [0, 1] per
    SOURCE ray, as many as labels; ``wbits``: the fraction bits of the quantised weight
    ``wq = rint(w * 2**wbits)`` (None: ``spot_wbits(group.numel())``).  ``acc`` is then (G, 8)
    int64 ``{W, Xhi, Xlo, Yhi, Ylo, count, 0, 0}``, the centroids are weighted means, and terms,
    gradient and penalty carry ``wr = wq * 2**-wbits``.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64 fixed
    point and the same operations per ray, each rounded on its own (``acc`` and the gradient rows
    agree bit for bit; the error sums are torch's and agree to rounding)."""
    n_groups = int(n_groups)
    if group.dtype != torch.int32 or group.dim() != 1 or not group.is_contiguous():
        raise ValueError("spot_error: group must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= SPOT_MAX_GROUPS:
        raise ValueError(f"spot_error: n_groups must lie in 1 .. {SPOT_MAX_GROUPS}")
    n = rows.shape[1]
    _check_field_codes("spot_error", rows, row_x, row_y, dimension)
    if qbits is None:
        qbits = spot_qbits(group.numel())
    record = 4
    if weights is not None:
        _check_weights("spot_error", weights)
        if weights.numel() != group.numel():
            raise ValueError("spot_error: one weight per label")
        if wbits is None:
            wbits = spot_wbits(group.numel())
        record = 8
    grad, err = _column_buffers("spot_error", rows, grad, err, mask, perm)
    if acc is None:
        acc = torch.empty((n_groups, record), dtype=torch.int64, device=rows.device)
    if tuple(acc.shape) != (n_groups, record) or acc.dtype != torch.int64 \
            or not acc.is_contiguous():
        raise ValueError(f"spot_error: acc must be contiguous int64 of shape (n_groups, {record})")
    x0, x1, qsx, y0, y1, qsy = grid
    if not rows.is_cuda:
        if weights is not None:
            if not 1 <= qbits <= 52 or not 1 <= wbits <= SPOT_MAX_WBITS \
                    or n >= 1 << (62 - wbits - (qbits + 1) // 2):
                raise ValueError("spot_error: qbits must lie in 1 .. 52 and wbits in 1 .. 20 with "
                                 "n < 2^(62 - wbits - ceil(qbits / 2))")
        elif not 1 <= qbits <= 52 or n >= 1 << (62 - qbits):
            raise ValueError("spot_error: qbits must lie in 1 .. 52 with n < 2^(62 - qbits)")
        _spot_error_cpu(rows, row_x, row_y, group, n_groups, grid, float(oob_weight), mask, perm,
                        grad, err, acc, int(qbits), dimension, weights,
                        None if wbits is None else int(wbits))
        return err, grad, acc
    L = _lib.lib()
    workspace = _column_workspace(
        "spot_error", rows, grad, workspace,
        lambda: L.tfrt_spot_error_workspace_bytes(n, n_groups), group, mask, perm, err, acc,
        weights)
    if weights is not None:
        # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
        check(L.tfrt_spot_error_weighted(
            _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
            _p(mask), row_x, row_y, _p(group), _p(weights), int(wbits), group.numel(), _p(perm),
            n_groups, x0, x1, qsx, y0, y1, qsy, int(qbits), float(oob_weight), _p(grad),
            grad.stride(0), _p(err), _p(acc), int(variant), _p(workspace), workspace.numel(),
            _stream(rows)), "tfrt_spot_error_weighted")
        return err, grad, acc
    if dimension is not None:
        check(L.tfrt_spot_error_fields(
            _p(rows), rows.stride(0), n, _DT[rows.dtype], int(dimension), _p(mask), row_x, row_y,
            _p(group), group.numel(), _p(perm), n_groups, x0, x1, qsx, y0, y1, qsy, int(qbits),
            float(oob_weight), _p(grad), grad.stride(0), _p(err), _p(acc), int(variant),
            _p(workspace), workspace.numel(), _stream(rows)), "tfrt_spot_error_fields")
        return err, grad, acc
    check(L.tfrt_spot_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], _p(mask), row_x, row_y, _p(group),
        group.numel(), _p(perm), n_groups, x0, x1, qsx, y0, y1, qsy, int(qbits),
        float(oob_weight), _p(grad), grad.stride(0), _p(err), _p(acc), int(variant),
        _p(workspace), workspace.numel(), _stream(rows)), "tfrt_spot_error")
    return err, grad, acc


def spot_centroids(acc, grid, fields=2, qbits=None):
    """The (G, fields) float64 centroids of a tfrt_spot_error record table:
    ``x0 + (Sx / count) / qsx``, NaN for a group without rays.  A table of eight-slot records
    (tfrt_spot_error_weighted; it needs the ``qbits`` of the evaluation for ``h = qbits // 2``):
    ``x0 + ((ldexp(Xhi, h) + Xlo) / W) / qsx``, NaN for a group without weight."""
    x0, _, qsx, y0, _, qsy = grid
    if acc.shape[1] == 8:
        if qbits is None:
            raise ValueError("spot_centroids: eight-slot records need qbits")
        lift = float(np.ldexp(1.0, int(qbits) // 2))       # (times 2^h: exact)
        W = acc[:, 0].double()
        W = torch.where(W > 0, W, torch.full_like(W, float("nan")))
        cols = [x0 + ((acc[:, 1].double() * lift + acc[:, 2].double()) / W) / qsx]
        if fields == 2:
            cols.append(y0 + ((acc[:, 3].double() * lift + acc[:, 4].double()) / W) / qsy)
        return torch.stack(cols, dim=1)
    cnt = acc[:, 0].double()
    cnt = torch.where(cnt > 0, cnt, torch.full_like(cnt, float("nan")))
    cols = [x0 + (acc[:, 1].double() / cnt) / qsx]
    if fields == 2:
        cols.append(y0 + (acc[:, 2].double() / cnt) / qsy)
    return torch.stack(cols, dim=1)


def _spot_error_cpu(rows, row_x, row_y, group, n_groups, grid, oob, mask, perm, grad, err, acc,
                    qbits, dimension=None, weights=None, wbits=None):
    """The CPU path of ``spot_error`` (every torch op rounds on its own, as the kernels do)."""
    x0, x1, qsx, y0, y1, qsy = grid
    two = row_y >= 0
    n = rows.shape[1]
    qmax = float(np.ldexp(1.0, qbits))
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counting = torch.ones(n, dtype=torch.bool) if mask is None else (mask[:n] >= 0)
    finite = torch.isfinite(x) & torch.isfinite(y)
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64)
    label[s_ok] = group[s[s_ok]].long()
    spot = counting & finite & s_ok & (label >= 0) & (label < n_groups)
    wq = wr = None
    if weights is not None:
        # wq = rint(w * 2^wbits), half to even; wr = wq * 2^-wbits is the weight everywhere
        w, w_ok = _source_weights(weights, perm, n)
        wq = torch.where(w_ok, torch.round(w * float(np.ldexp(1.0, wbits))), torch.zeros_like(w))
        wr = wq * float(np.ldexp(1.0, -wbits))
        spot &= wq > 0
    # outside: the penalty and its derivative (weighted: each times wr last)
    inside, pen, gx, gy = _outside_cpu(x, y, two, grid, oob, spot, wr)
    # inside: the fixed-point records, one list of slots per layout
    xi, yi, li = x[inside], y[inside], label[inside]
    acc.zero_()
    qxi = torch.round((xi - x0) * qsx).clamp(0.0, qmax).long()
    qyi = torch.round((yi - y0) * qsy).clamp(0.0, qmax).long() if two else None
    ones = torch.ones_like(li)
    if wr is None:
        slots = [ones, qxi, qyi]                       # {count, Sx, Sy, 0}
    else:
        # {W, Xhi, Xlo, Yhi, Ylo, count, 0, 0}: wq * q in two limbs of h and qbits - h bits
        h = qbits // 2
        low = (1 << h) - 1
        wqi = wq[inside].long()
        slots = [wqi, wqi * (qxi >> h), wqi * (qxi & low)]
        slots += [wqi * (qyi >> h), wqi * (qyi & low)] if two else [None, None]
        slots.append(ones)
    for p, v in enumerate(slots):
        if v is not None:
            acc[:, p].index_add_(0, li, v)
    # (spot_centroids reads both layouts, group by group in the kernels' operation order)
    centre = spot_centroids(acc, grid, 2 if two else 1, qbits)[li]
    wri = None if wr is None else wr[inside]
    terms = None
    for k, (vi, g) in enumerate(((xi, gx), (yi, gy))[:2 if two else 1]):
        d = vi - centre[:, k]
        g[inside] = 2.0 * d if wri is None else (2.0 * d) * wri
        t = d * d if wri is None else wri * (d * d)
        terms = t if terms is None else terms + t
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, spot)
    e = terms.sum() + pen
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    err[0], err[1] = e, n_terms
    err[2] = e / n_terms if n_terms > 0 else float("nan")


# ------------------------------------------- group centroids as a scaled copy of the object
DISTORTION_FITS = {"scale": 0, "affine": 1}
DISTORTION_BLOCK = 1024            # k_distortion_fit: one workgroup of 16 waves


def distortion_group_sum(values, used):
    """The sum of ``values[used]`` over the groups in the fixed shape and order of
    k_distortion_fit, as float64 torch ops on the CPU: thread j takes the groups j, j + 1024, ...
    in ascending order from 0.0 (unused groups skipped), the 64 lanes of a wave are combined by
    ``v += v[lane ^ d]`` for d = 32 .. 1, then the 16 waves in index order from 0.0."""
    B = DISTORTION_BLOCK
    G = values.numel()
    trips = max((G + B - 1) // B, 1)
    v = torch.zeros(trips * B, dtype=torch.float64)
    u = torch.zeros(trips * B, dtype=torch.bool)
    v[:G], u[:G] = values.double().cpu(), used.cpu()
    s = torch.zeros(B, dtype=torch.float64)
    for vt, ut in zip(v.view(trips, B), u.view(trips, B)):
        s = torch.where(ut, s + vt, s)
    w = s.view(B // 64, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :d] + w[:, d:2 * d]
    total = torch.zeros((), dtype=torch.float64)
    for wave in w[:, 0]:
        total = total + wave
    return total


def _distortion_fit_cpu(acc, points, grid, two, fit_kind, min_cond):
    """(fit_out (8,), residual (G, 2)) of a record table: distortion_math.h, operation by
    operation, over all groups at once (CPU float64 tensors)."""
    x0, _, qsx, y0, _, qsy = grid
    G = acc.shape[0]
    cnt = acc[:, 0]
    used = cnt > 0
    w = cnt.double()
    zeros = torch.zeros(G, dtype=torch.float64)
    safe = torch.where(used, w, torch.ones_like(w))
    cx = x0 + (acc[:, 1].double() / safe) / qsx
    cy = y0 + (acc[:, 2].double() / safe) / qsy if two else zeros
    px = points[:, 0].double()
    py = points[:, 1].double() if two else zeros
    gsum = lambda v: distortion_group_sum(v, used)          # noqa: E731
    W = gsum(w)
    pmx, pmy, cmx, cmy = (gsum(w * v) / W for v in (px, py, cx, cy))
    n_used = int(used.sum())
    dpx, dpy, dcx, dcy = px - pmx, py - pmy, cx - cmx, cy - cmy
    Sxx, Sxy, Syy = gsum(w * (dpx * dpx)), gsum(w * (dpx * dpy)), gsum(w * (dpy * dpy))
    Cxx, Cxy = gsum(w * (dcx * dpx)), gsum(w * (dcx * dpy))
    Cyx, Cyy = gsum(w * (dcy * dpx)), gsum(w * (dcy * dpy))
    trp = Sxx + Syy
    nan = float("nan")
    fit = torch.full((8,), nan, dtype=torch.float64)
    if fit_kind == 1 and two:
        det = Sxx * Syy - Sxy * Sxy
        h = trp / 2.0
        valid = bool(det > min_cond * (h * h))
        A = ((Cxx * Syy - Cxy * Sxy) / det, (Cxy * Sxx - Cxx * Sxy) / det,
             (Cyx * Syy - Cyy * Sxy) / det, (Cyy * Sxx - Cyx * Sxy) / det)
    else:
        valid = n_used >= 2 and bool(trp > 0.0)
        M = (Cxx + Cyy) / trp
        A = (M, zeros[0], zeros[0], M)
    residual = torch.full((G, 2), nan, dtype=torch.float64)
    if valid:
        fit[0], fit[1], fit[2], fit[3] = A
        fit[4] = cmx - (A[0] * pmx + A[1] * pmy)
        fit[5] = cmy - (A[2] * pmx + A[3] * pmy)
        rx = cx - (cmx + (A[0] * dpx + A[1] * dpy))
        ry = cy - (cmy + (A[2] * dpx + A[3] * dpy))
    else:
        rx = ry = zeros
    residual[:, 0] = torch.where(used, rx, residual[:, 0])
    residual[:, 1] = torch.where(used, ry, residual[:, 1])
    fit[6], fit[7] = float(valid), float(n_used)
    inside = gsum(w * (residual[:, 0] * residual[:, 0])) \
        + gsum(w * (residual[:, 1] * residual[:, 1]))
    return fit, residual, inside


def distortion_error(rows, row_x, row_y, group, n_groups, points, grid, fit="scale",
                     min_cond=1e-9, oob_weight=0.0, mask=None, perm=None, grad=None, err=None,
                     acc=None, fit_out=None, residual=None, variant=0, workspace=None, qbits=None,
                     dimension=None):
    """tfrt_distortion_error: the DistortionError of the columns of ``rows`` -- the centroids of
    the groups must be a scaled (``fit="scale"``) or affine (``"affine"``) copy of the object
    points ``points`` (G, k) float64, at whatever magnification and offset fits best.  The
    columns, ``row_x`` / ``row_y``, ``group``, ``perm``, ``n_groups``, ``grid`` (``spot_grid``),
    ``qbits``, ``mask``, ``oob_weight``, ``variant`` and ``dimension`` are ``spot_error``'s
    (without ``dimension`` the rows are those of a 3-D block, as there).  Returns (err {sum,
    terms, mean}, grad, acc (G, 4) int64 {count, Sx, Sy, 0}, fit_out (8,) float64 {A00, A01, A10,
    A11, t0, t1, valid, groups used}, residual (G, 2) float64 -- NaN for a group without rays, 0
    without a valid fit).  ``grad``, ``err``, ``acc``, ``fit_out``, ``residual``, ``workspace``
    (uint8): buffers to reuse -- with all six given a CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64 fixed
    point, the same operations and the same order of the sums over the groups (``acc``,
    ``fit_out``, ``residual`` and the gradient rows agree bit for bit; the penalty sum is torch's
    and agrees to rounding)."""
    what = "distortion_error"
    n_groups = int(n_groups)
    if group.dtype != torch.int32 or group.dim() != 1 or not group.is_contiguous():
        raise ValueError(f"{what}: group must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= SPOT_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {SPOT_MAX_GROUPS}")
    if fit not in DISTORTION_FITS:
        raise ValueError(f"{what}: fit must be 'scale' or 'affine', got {fit!r}")
    min_cond = float(min_cond)
    if not (min_cond >= 0.0 and np.isfinite(min_cond)):
        raise ValueError(f"{what}: min_cond must be finite and >= 0")
    n = rows.shape[1]
    _check_field_codes(what, rows, row_x, row_y, dimension)
    k = 2 if row_y >= 0 else 1
    if points.dtype != torch.float64 or tuple(points.shape) != (n_groups, k) \
            or not points.is_contiguous() or points.device != rows.device:
        raise ValueError(f"{what}: points must be contiguous float64 of shape (n_groups, {k}) "
                         "on the rows' device")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups > SPOT_LDS_GROUPS):
        raise ValueError(f"{what}: variant must be 0, 1 (up to {SPOT_LDS_GROUPS} groups) or 2")
    if qbits is None:
        qbits = spot_qbits(group.numel())
    if not 1 <= qbits <= 52 or n >= 1 << (62 - qbits):
        raise ValueError(f"{what}: qbits must lie in 1 .. 52 with n < 2^(62 - qbits)")
    grad, err = _column_buffers(what, rows, grad, err, mask, perm)
    dev = rows.device
    made = dict(acc=((n_groups, 4), torch.int64), fit_out=((8,), torch.float64),
                residual=((n_groups, 2), torch.float64))
    given = dict(acc=acc, fit_out=fit_out, residual=residual)
    for name, (shape, dtype) in made.items():
        if given[name] is None:
            given[name] = torch.empty(shape, dtype=dtype, device=dev)
        b = given[name]
        if tuple(b.shape) != shape or b.dtype != dtype or not b.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dtype} of shape {shape}")
    acc, fit_out, residual = given["acc"], given["fit_out"], given["residual"]
    if not rows.is_cuda:
        _distortion_error_cpu(rows, row_x, row_y, group, n_groups, points, grid,
                              DISTORTION_FITS[fit], min_cond, float(oob_weight), mask, perm, grad,
                              err, acc, fit_out, residual, int(qbits), dimension)
        return err, grad, acc, fit_out, residual
    L = _lib.lib()
    workspace = _column_workspace(
        what, rows, grad, workspace,
        lambda: L.tfrt_distortion_error_workspace_bytes(n, n_groups), group, mask, perm, err, acc,
        fit_out, residual, points)
    x0, x1, qsx, y0, y1, qsy = grid
    # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
    check(L.tfrt_distortion_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
        _p(mask), row_x, row_y, _p(group), group.numel(), _p(perm), n_groups, _p(points),
        DISTORTION_FITS[fit], min_cond, x0, x1, qsx, y0, y1, qsy, int(qbits), float(oob_weight),
        _p(grad), grad.stride(0), _p(err), _p(fit_out), _p(residual), _p(acc), int(variant),
        _p(workspace), workspace.numel(), _stream(rows)), "tfrt_distortion_error")
    return err, grad, acc, fit_out, residual


def _distortion_error_cpu(rows, row_x, row_y, group, n_groups, points, grid, fit_kind, min_cond,
                          oob, mask, perm, grad, err, acc, fit_out, residual, qbits, dimension):
    """The CPU path of ``distortion_error`` (every torch op rounds on its own, as the kernels
    do)."""
    x0, x1, qsx, y0, y1, qsy = grid
    two = row_y >= 0
    n = rows.shape[1]
    qmax = float(np.ldexp(1.0, qbits))
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counting = torch.ones(n, dtype=torch.bool) if mask is None else (mask[:n] >= 0)
    finite = torch.isfinite(x) & torch.isfinite(y)
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64)
    label[s_ok] = group[s[s_ok]].long()
    spot = counting & finite & s_ok & (label >= 0) & (label < n_groups)
    inside, pen, gx, gy = _outside_cpu(x, y, two, grid, oob, spot, None)
    xi, yi, li = x[inside], y[inside], label[inside]
    acc.zero_()
    acc[:, 0].index_add_(0, li, torch.ones_like(li))
    acc[:, 1].index_add_(0, li, torch.round((xi - x0) * qsx).clamp(0.0, qmax).long())
    if two:
        acc[:, 2].index_add_(0, li, torch.round((yi - y0) * qsy).clamp(0.0, qmax).long())
    fit, res, e_inside = _distortion_fit_cpu(acc, points, grid, two, fit_kind, min_cond)
    fit_out.copy_(fit)
    residual.copy_(res)
    gx[inside] = 2.0 * res[li, 0]
    if two:
        gy[inside] = 2.0 * res[li, 1]
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, spot)
    e = e_inside + pen
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    err[0], err[1] = e, n_terms
    err[2] = e / n_terms if n_terms > 0 else float("nan")


# ----------------------------------------- group centroids at targets, or registered by parent
def centroid_error(rows, row_x, row_y, group, n_groups, grid, targets=None, parents=None,
                   n_parents=None, oob_weight=0.0, mask=None, perm=None, grad=None, err=None,
                   acc=None, residual=None, used_out=None, parent_acc=None, variant=0,
                   workspace=None, qbits=None, dimension=None):
    """tfrt_centroid_error: the CentroidError of the columns of ``rows`` -- the centroid of every
    group must lie at its row of ``targets`` (G, k) float64 (a row with a non-finite entry: not
    pinned), or the centroids of the groups with the same entry of ``parents`` (G,) int32 must
    coincide (an entry outside ``[0, n_parents)``: left out).  Exactly one of the two is given.
    The columns, ``row_x`` / ``row_y``, ``group``, ``perm``, ``n_groups``, ``grid``
    (``spot_grid``), ``qbits``, ``mask``, ``oob_weight``, ``variant`` and ``dimension`` are
    ``spot_error``'s.  Returns (err {sum, terms, mean}, grad, acc (G, 4) int64 {count, Sx, Sy, 0},
    residual (G, 2) float64 -- ``c - t`` of a used group, 0 for a group with rays and no target,
    NaN for a group without rays --, used_out (2,) float64 {groups used, parents with rays},
    parent_acc (P, 4) int64, the parents' records (None with ``targets``)).  ``grad``, ``err``,
    ``acc``, ``residual``, ``used_out``, ``parent_acc``, ``workspace`` (uint8): buffers to reuse
    -- with all of them given a CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64 fixed
    point, the same operations per group and the same order of the sums over the groups (``acc``,
    ``parent_acc``, ``residual`` and the gradient rows agree bit for bit; the penalty sum is
    torch's and agrees to rounding)."""
    what = "centroid_error"
    n_groups = int(n_groups)
    if group.dtype != torch.int32 or group.dim() != 1 or not group.is_contiguous():
        raise ValueError(f"{what}: group must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= SPOT_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {SPOT_MAX_GROUPS}")
    if (targets is None) == (parents is None):
        raise ValueError(f"{what}: exactly one of targets and parents must be given")
    n = rows.shape[1]
    _check_field_codes(what, rows, row_x, row_y, dimension)
    k = 2 if row_y >= 0 else 1
    if targets is not None:
        if targets.dtype != torch.float64 or tuple(targets.shape) != (n_groups, k) \
                or not targets.is_contiguous() or targets.device != rows.device:
            raise ValueError(f"{what}: targets must be contiguous float64 of shape (n_groups, "
                             f"{k}) on the rows' device")
        n_parents = 0
    else:
        if parents.dtype != torch.int32 or tuple(parents.shape) != (n_groups,) \
                or not parents.is_contiguous() or parents.device != rows.device:
            raise ValueError(f"{what}: parents must be contiguous int32 of shape (n_groups,) on "
                             "the rows' device")
        if n_parents is None:
            raise ValueError(f"{what}: parents need n_parents")
        n_parents = int(n_parents)
        if not 1 <= n_parents <= SPOT_MAX_GROUPS:
            raise ValueError(f"{what}: n_parents must lie in 1 .. {SPOT_MAX_GROUPS}")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups > SPOT_LDS_GROUPS):
        raise ValueError(f"{what}: variant must be 0, 1 (up to {SPOT_LDS_GROUPS} groups) or 2")
    if qbits is None:
        qbits = spot_qbits(group.numel())
    if not 1 <= qbits <= 52 or n >= 1 << (62 - qbits):
        raise ValueError(f"{what}: qbits must lie in 1 .. 52 with n < 2^(62 - qbits)")
    grad, err = _column_buffers(what, rows, grad, err, mask, perm)
    dev = rows.device
    made = dict(acc=((n_groups, 4), torch.int64), residual=((n_groups, 2), torch.float64),
                used_out=((2,), torch.float64))
    given = dict(acc=acc, residual=residual, used_out=used_out)
    if parents is not None:
        made["parent_acc"] = ((n_parents, 4), torch.int64)
        given["parent_acc"] = parent_acc
    for name, (shape, dtype) in made.items():
        if given[name] is None:
            given[name] = torch.empty(shape, dtype=dtype, device=dev)
        b = given[name]
        if tuple(b.shape) != shape or b.dtype != dtype or not b.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dtype} of shape {shape}")
    acc, residual, used_out = given["acc"], given["residual"], given["used_out"]
    parent_acc = given.get("parent_acc")
    if not rows.is_cuda:
        _centroid_error_cpu(rows, row_x, row_y, group, n_groups, grid, targets, parents,
                            n_parents, float(oob_weight), mask, perm, grad, err, acc, residual,
                            used_out, parent_acc, int(qbits), dimension)
        return err, grad, acc, residual, used_out, parent_acc
    L = _lib.lib()
    workspace = _column_workspace(
        what, rows, grad, workspace,
        lambda: L.tfrt_centroid_error_workspace_bytes(n, n_groups), group, mask, perm, err, acc,
        residual, used_out, targets, parents, parent_acc)
    x0, x1, qsx, y0, y1, qsy = grid
    # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
    check(L.tfrt_centroid_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
        _p(mask), row_x, row_y, _p(group), group.numel(), _p(perm), n_groups, _p(targets),
        _p(parents), n_parents, _p(parent_acc), x0, x1, qsx, y0, y1, qsy, int(qbits),
        float(oob_weight), _p(grad), grad.stride(0), _p(err), _p(used_out), _p(residual), _p(acc),
        int(variant), _p(workspace), workspace.numel(), _stream(rows)), "tfrt_centroid_error")
    return err, grad, acc, residual, used_out, parent_acc


def centroid_parent_centroids(parent_acc, grid, fields=2):
    """The (P, fields) float64 centroids of the parents' records of ``centroid_error``, NaN for a
    parent without rays: ``x0 + (Sx / count) / qsx``, the expression the table launch forms its
    targets by, bit for bit on either device.  (``spot_centroids`` divides by the Python number
    ``qsx``, which torch on the device turns into a product with its reciprocal; here the divisor
    is a tensor and the device divides.)"""
    x0, _, qsx, y0, _, qsy = grid
    cnt = parent_acc[:, 0].double()
    cnt = torch.where(cnt > 0, cnt, torch.full_like(cnt, float("nan")))
    cols = [x0 + (parent_acc[:, 1].double() / cnt) / torch.full_like(cnt, qsx)]
    if fields == 2:
        cols.append(y0 + (parent_acc[:, 2].double() / cnt) / torch.full_like(cnt, qsy))
    return torch.stack(cols, dim=1)


def _centroid_table_cpu(acc, grid, two, targets, parents, n_parents, parent_acc):
    """(residual (G, 2), used (G,) bool, inside error) of a record table: centroid_math.h,
    operation by operation, over all groups at once (CPU tensors); ``parent_acc`` is filled."""
    x0, _, qsx, y0, _, qsy = grid
    G = acc.shape[0]
    rays = acc[:, 0] > 0
    zeros = torch.zeros(G, dtype=torch.float64)

    def centroid(table):
        w = table[:, 0].double()
        safe = torch.where(table[:, 0] > 0, w, torch.ones_like(w))
        cx = x0 + (table[:, 1].double() / safe) / qsx
        cy = y0 + (table[:, 2].double() / safe) / qsy if two else torch.zeros_like(w)
        return cx, cy

    w = acc[:, 0].double()
    cx, cy = centroid(acc)
    if targets is not None:
        tx = targets[:, 0]
        ty = targets[:, 1] if two else zeros
        has = torch.isfinite(tx) & torch.isfinite(ty)
    else:
        p = parents.long()
        has = (p >= 0) & (p < n_parents)
        parent_acc.zero_()
        sel = rays & has
        parent_acc.index_add_(0, p[sel], acc[sel])
        Cx, Cy = centroid(parent_acc)
        at = p.clamp(0, n_parents - 1)
        tx, ty = Cx[at], Cy[at]
    used = rays & has
    nan = float("nan")
    residual = torch.full((G, 2), nan, dtype=torch.float64)
    residual[:, 0] = torch.where(used, cx - tx, torch.where(rays, zeros, residual[:, 0]))
    residual[:, 1] = torch.where(used, cy - ty, torch.where(rays, zeros, residual[:, 1]))
    rx = torch.where(used, residual[:, 0], zeros)
    ry = torch.where(used, residual[:, 1], zeros)
    inside = distortion_group_sum(w * (rx * rx), used) + distortion_group_sum(w * (ry * ry), used)
    return residual, used, inside


def _centroid_error_cpu(rows, row_x, row_y, group, n_groups, grid, targets, parents, n_parents,
                        oob, mask, perm, grad, err, acc, residual, used_out, parent_acc, qbits,
                        dimension):
    """The CPU path of ``centroid_error`` (every torch op rounds on its own, as the kernels
    do)."""
    x0, x1, qsx, y0, y1, qsy = grid
    two = row_y >= 0
    n = rows.shape[1]
    qmax = float(np.ldexp(1.0, qbits))
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counting = torch.ones(n, dtype=torch.bool) if mask is None else (mask[:n] >= 0)
    finite = torch.isfinite(x) & torch.isfinite(y)
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64)
    label[s_ok] = group[s[s_ok]].long()
    spot = counting & finite & s_ok & (label >= 0) & (label < n_groups)
    inside, pen, gx, gy = _outside_cpu(x, y, two, grid, oob, spot, None)
    xi, yi, li = x[inside], y[inside], label[inside]
    acc.zero_()
    acc[:, 0].index_add_(0, li, torch.ones_like(li))
    acc[:, 1].index_add_(0, li, torch.round((xi - x0) * qsx).clamp(0.0, qmax).long())
    if two:
        acc[:, 2].index_add_(0, li, torch.round((yi - y0) * qsy).clamp(0.0, qmax).long())
    res, used, e_inside = _centroid_table_cpu(acc, grid, two, targets, parents, n_parents,
                                              parent_acc)
    residual.copy_(res)
    used_out[0] = float(int(used.sum()))
    used_out[1] = 0.0 if parent_acc is None else float(int((parent_acc[:, 0] > 0).sum()))
    gx[inside] = 2.0 * res[li, 0]
    if two:
        gy[inside] = 2.0 * res[li, 1]
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, spot)
    e = e_inside + pen
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    err[0], err[1] = e, n_terms
    err[2] = e / n_terms if n_terms > 0 else float("nan")


# ------------------------------------------------- the covariance of every group: size and shape
MOMENT_LDS_GROUPS = 256            # tfrt_moment_error: 9 planes of sums, 2 of centres in LDS, 22 KiB
MOMENT_MAX_MBITS = 40
MOMENT_MODES = {"covariance": 0, "round": 1}
MOMENT_SEED_MAX_GRID = 2048        # workgroups of 256 lanes of k_moment_seed


def moment_mbits(n_source):
    """Fraction bits of tfrt_moment_error's grid for a source of ``n_source`` rays: even, at most
    40, with ``n_source * 2^(mbits + 1) < 2^62`` -- every limb sum of pass 2 fits an int64."""
    return min(MOMENT_MAX_MBITS, 2 * ((61 - int(n_source).bit_length()) // 2))


def penalty_sum_fixed(pens, outside):
    """The sum of ``pens[outside]`` over the n columns in the shape and order of the kernels, as
    float64 torch ops on the CPU: the accumulate launch's ``B = min(512, ceil(n / 1024))``
    workgroups of 256 threads, thread t of workgroup b adds its columns ``256 b + t``,
    ``+ 256 B``, ... onto 0.0, a wave's 64 lanes by ``v += v[lane ^ d]`` for d = 32 .. 1, a
    workgroup's 4 waves in index order; then the partials as ``distortion_group_sum`` adds the
    groups."""
    n = pens.numel()
    if n == 0:
        return torch.zeros((), dtype=torch.float64)
    B = min(SPOT_MAX_GRID, (n + SPOT_RAYS_PER_BLOCK - 1) // SPOT_RAYS_PER_BLOCK)
    stride = B * 256
    trips = (n + stride - 1) // stride
    v = torch.zeros(trips * stride, dtype=torch.float64)
    v[:n] = torch.where(outside, pens, torch.zeros_like(pens))
    lanes = torch.zeros(stride, dtype=torch.float64)
    for trip in v.view(trips, stride):
        lanes = lanes + trip                   # (penalties are >= 0: adding 0.0 changes no bit)
    w = lanes.view(B * 4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :d] + w[:, d:2 * d]
    waves = w[:, 0].reshape(B, 4)
    partial = torch.zeros(B, dtype=torch.float64)
    for k in range(4):
        partial = partial + waves[:, k]
    return distortion_group_sum(partial, torch.ones(B, dtype=torch.bool))


def moment_error(rows, row_x, row_y, group, n_groups, grid, covariance=None, shape=None,
                 oob_weight=0.0, mask=None, perm=None, grad=None, err=None, acc=None, mom=None,
                 group_rows=None, cov=None, used_out=None, variant=0, workspace=None, mbits=None,
                 dimension=None):
    """tfrt_moment_error: the MomentError of the columns of ``rows`` -- the covariance of every
    group's rays must be its row of ``covariance`` (G, 3) float64 ``{txx, txy, tyy}`` ((G, 1) with
    one field; a NaN component is free), or, with ``shape="round"`` (two fields), isotropic at
    whatever size.  Exactly one of the two is given.  The columns, ``row_x`` / ``row_y``,
    ``group``, ``perm``, ``n_groups``, ``mask``, ``oob_weight`` and ``dimension`` are
    ``spot_error``'s; ``grid`` is ``spot_grid(domain, mbits)`` with ``mbits`` (None:
    ``moment_mbits(group.numel())``) even, 2 .. 40.  ``variant``: 0 by G, 1 tables in LDS (up to
    ``MOMENT_LDS_GROUPS`` groups), 2 global atomics.  Returns (err {sum, terms, mean}, grad, acc (G, 4) int64 {n, Sx,
    Sy, 0}, mom (G, 9) int64 {xx, xy, yy} x {HH, HL, LL}, group_rows (G, 8) float64 {cx, cy, 4Dxx,
    4Dxy, 4Dyy, used, 0, 0}, cov (G, 6) float64 {Cxx, Cxy, Cyy, Dxx, Dxy, Dyy} -- NaN for a group
    of fewer than two rays --, used_out (2,) float64 {groups used, groups with rays}).  ``grad``,
    ``err``, ``acc``, ``mom``, ``group_rows``, ``cov``, ``used_out``, ``workspace`` (uint8):
    buffers to reuse -- with all of them given a CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64
    records, the same operations per group and per ray and the same order of every sum: every
    output agrees bit for bit."""
    what = "moment_error"
    n_groups = int(n_groups)
    if group.dtype != torch.int32 or group.dim() != 1 or not group.is_contiguous():
        raise ValueError(f"{what}: group must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= SPOT_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {SPOT_MAX_GROUPS}")
    if (covariance is None) == (shape is None):
        raise ValueError(f"{what}: exactly one of covariance and shape must be given")
    if shape is not None and shape != "round":
        raise ValueError(f"{what}: shape must be 'round', got {shape!r}")
    n = rows.shape[1]
    _check_field_codes(what, rows, row_x, row_y, dimension)
    two = row_y >= 0
    k3 = 3 if two else 1
    if shape is not None and not two:
        raise ValueError(f"{what}: shape='round' needs two fields")
    if covariance is not None and (
            covariance.dtype != torch.float64 or tuple(covariance.shape) != (n_groups, k3)
            or not covariance.is_contiguous() or covariance.device != rows.device):
        raise ValueError(f"{what}: covariance must be contiguous float64 of shape (n_groups, "
                         f"{k3}) on the rows' device")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups > MOMENT_LDS_GROUPS):
        raise ValueError(f"{what}: variant must be 0, 1 (up to {MOMENT_LDS_GROUPS} groups) or 2")
    if mbits is None:
        mbits = moment_mbits(group.numel())
    mbits = int(mbits)
    if not 2 <= mbits <= MOMENT_MAX_MBITS or mbits % 2 or n >= 1 << (61 - mbits):
        raise ValueError(f"{what}: mbits must be even and lie in 2 .. {MOMENT_MAX_MBITS} with "
                         "n < 2^(61 - mbits)")
    grad, err = _column_buffers(what, rows, grad, err, mask, perm)
    dev = rows.device
    made = dict(acc=((n_groups, 4), torch.int64), mom=((n_groups, 9), torch.int64),
                group_rows=((n_groups, 8), torch.float64), cov=((n_groups, 6), torch.float64),
                used_out=((2,), torch.float64))
    given = dict(acc=acc, mom=mom, group_rows=group_rows, cov=cov, used_out=used_out)
    for name, (shp, dtype) in made.items():
        if given[name] is None:
            given[name] = torch.empty(shp, dtype=dtype, device=dev)
        b = given[name]
        if tuple(b.shape) != shp or b.dtype != dtype or not b.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dtype} of shape {shp}")
    acc, mom, group_rows = given["acc"], given["mom"], given["group_rows"]
    cov, used_out = given["cov"], given["used_out"]
    mode = MOMENT_MODES["round" if shape is not None else "covariance"]
    if not rows.is_cuda:
        _moment_error_cpu(rows, row_x, row_y, group, n_groups, grid, mode, covariance,
                          float(oob_weight), mask, perm, grad, err, acc, mom, group_rows, cov,
                          used_out, mbits, dimension)
        return err, grad, acc, mom, group_rows, cov, used_out
    L = _lib.lib()
    workspace = _column_workspace(
        what, rows, grad, workspace,
        lambda: L.tfrt_moment_error_workspace_bytes(n, n_groups), group, mask, perm, err, acc,
        mom, group_rows, cov, used_out, covariance)
    x0, x1, msx, y0, y1, msy = grid
    # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
    check(L.tfrt_moment_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
        _p(mask), row_x, row_y, _p(group), group.numel(), _p(perm), n_groups, mode,
        _p(covariance), x0, x1, msx, y0, y1, msy, mbits, float(oob_weight), _p(grad),
        grad.stride(0), _p(err), _p(used_out), _p(group_rows), _p(cov), _p(acc), _p(mom),
        int(variant), _p(workspace), workspace.numel(), _stream(rows)), "tfrt_moment_error")
    return err, grad, acc, mom, group_rows, cov, used_out


def moment_covariances(cov, fields=2):
    """The (G, 3) float64 covariances ``{Cxx, Cxy, Cyy}`` of a ``moment_error`` evaluation, (G, 1)
    with one field: the second moments of every group's rays about its centre, in scene units
    squared, NaN for a group of fewer than two rays."""
    return cov[:, :3 if fields == 2 else 1]


def _moment_table_cpu(acc, mom, grid, two, mode, covariance, mbits):
    """(group_rows (G, 8), cov (G, 6), used (G,) bool, rays (G,) bool, inside error) of the two
    record tables: moment_math.h, operation by operation, over all groups at once (CPU)."""
    x0, _, msx, y0, _, msy = grid
    G = acc.shape[0]
    h = mbits // 2
    cnt = acc[:, 0]
    rays, used = cnt > 0, cnt >= 2
    nan = float("nan")
    zeros = torch.zeros(G, dtype=torch.float64)
    nans = torch.full((G,), nan, dtype=torch.float64)
    safe = torch.where(rays, cnt, torch.ones_like(cnt))
    nf = safe.double()
    kx = torch.div(2 * acc[:, 1] + safe, 2 * safe, rounding_mode="floor")
    ky = torch.div(2 * acc[:, 2] + safe, 2 * safe, rounding_mode="floor")
    cx = torch.where(rays, x0 + kx.double() / msx, nans)
    cy = torch.where(rays, y0 + ky.double() / msy, nans) if two else torch.where(rays, zeros, nans)
    hi, mid = float(np.ldexp(1.0, mbits)), float(np.ldexp(1.0, h))      # (times 2^k: exact)

    def value(first):
        m = mom[:, first:first + 3].double()
        return (m[:, 0] * hi + m[:, 1] * mid) + m[:, 2]

    C = [(value(0) / nf) / (msx * msx),
         (value(3) / nf) / (msx * msy) if two else zeros,
         (value(6) / nf) / (msy * msy) if two else zeros]
    if mode == MOMENT_MODES["round"]:
        s = (C[0] + C[2]) / 2.0
        D = [C[0] - s, C[1], C[2] - s]
    else:
        t = [covariance[:, 0], covariance[:, 1] if two else nans,
             covariance[:, 2] if two else nans]
        D = [torch.where(torch.isnan(t[c]), zeros, C[c] - t[c]) for c in range(3)]
    e = nf * ((D[0] * D[0] + 2.0 * (D[1] * D[1])) + D[2] * D[2])
    group_rows = torch.zeros((G, 8), dtype=torch.float64)
    group_rows[:, 0], group_rows[:, 1] = cx, cy
    cov = torch.full((G, 6), nan, dtype=torch.float64)
    for c in range(3):
        group_rows[:, 2 + c] = torch.where(used, 4.0 * D[c], zeros)
        cov[:, c] = torch.where(used, C[c], nans)
        cov[:, 3 + c] = torch.where(used, D[c], nans)
    group_rows[:, 5] = used.double()
    inside = distortion_group_sum(torch.where(used, e, zeros), used)
    return group_rows, cov, used, rays, inside, kx, ky


def _moment_error_cpu(rows, row_x, row_y, group, n_groups, grid, mode, covariance, oob, mask,
                      perm, grad, err, acc, mom, group_rows, cov, used_out, mbits, dimension):
    """The CPU path of ``moment_error`` (every torch op rounds on its own, as the kernels do)."""
    x0, x1, msx, y0, y1, msy = grid
    two = row_y >= 0
    n = rows.shape[1]
    h = mbits // 2
    low = (1 << h) - 1
    mmax = float(np.ldexp(1.0, mbits))
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counting = torch.ones(n, dtype=torch.bool) if mask is None else (mask[:n] >= 0)
    finite = torch.isfinite(x) & torch.isfinite(y)
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64)
    label[s_ok] = group[s[s_ok]].long()
    spot = counting & finite & s_ok & (label >= 0) & (label < n_groups)
    inside, _, gx, gy = _outside_cpu(x, y, two, grid, oob, spot, None)
    zero = torch.zeros((), dtype=torch.float64)
    ex = torch.maximum(x0 - x, zero) + torch.maximum(x - x1, zero)
    ey = (torch.maximum(y0 - y, zero) + torch.maximum(y - y1, zero)) if two \
        else torch.zeros_like(x)
    pen = penalty_sum_fixed(oob * (ex * ex + ey * ey), spot & ~inside)
    xi, yi, li = x[inside], y[inside], label[inside]
    mx = torch.round((xi - x0) * msx).clamp(0.0, mmax).long()
    my = torch.round((yi - y0) * msy).clamp(0.0, mmax).long() if two else torch.zeros_like(mx)
    acc.zero_()
    acc[:, 0].index_add_(0, li, torch.ones_like(li))
    acc[:, 1].index_add_(0, li, mx)
    if two:
        acc[:, 2].index_add_(0, li, my)
    # pass 2: the limb products about the integer centres of the used groups
    cnt = acc[:, 0]
    safe = torch.where(cnt > 0, cnt, torch.ones_like(cnt))
    kx = torch.div(2 * acc[:, 1] + safe, 2 * safe, rounding_mode="floor")
    ky = torch.div(2 * acc[:, 2] + safe, 2 * safe, rounding_mode="floor")
    in_used = (cnt >= 2)[li]
    lu = li[in_used]
    dx, dy = (mx - kx[li])[in_used], (my - ky[li])[in_used]
    xl, xh, yl, yh = dx & low, dx >> h, dy & low, dy >> h
    mom.zero_()
    sums = [xh * xh, 2 * (xh * xl), xl * xl]
    if two:
        sums += [xh * yh, xh * yl + xl * yh, xl * yl, yh * yh, 2 * (yh * yl), yl * yl]
    for p, v in enumerate(sums):
        mom[:, p].index_add_(0, lu, v)
    rows_g, cov_g, used, rays, e_inside = _moment_table_cpu(acc, mom, grid, two, mode,
                                                            covariance, mbits)[:5]
    group_rows.copy_(rows_g)
    cov.copy_(cov_g)
    used_out[0], used_out[1] = float(int(used.sum())), float(int(rays.sum()))
    row = rows_g[li]
    ux = xi - row[:, 0]
    if two:
        uy = yi - row[:, 1]
        gxi, gyi = row[:, 2] * ux + row[:, 3] * uy, row[:, 3] * ux + row[:, 4] * uy
    else:
        gxi = row[:, 2] * ux
    live = row[:, 5] != 0.0
    gx[inside] = torch.where(live, gxi, torch.zeros_like(gxi))
    if two:
        gy[inside] = torch.where(live, gyi, torch.zeros_like(gyi))
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, spot)
    e = e_inside + pen
    n_terms = float(int(counting.sum()) * (2 if two else 1))
    err[0], err[1] = e, n_terms
    err[2] = e / n_terms if n_terms > 0 else float("nan")


# ------------------------------------------------------- every group with the same density
MIXING_MAX_GROUPS = 1024
MIXING_MAX_CELLS = 1 << 20         # n_groups * bins
MIXING_LDS_CELLS = 4096            # tfrt_mixing_error: the whole table as int64 in LDS, 32 KiB


def mixing_error(rows, row_x, row_y, group, n_groups, bins, grid, oob_weight=0.0, mask=None,
                 perm=None, grad=None, err=None, hq=None, pull=None, group_errors=None,
                 used_out=None, workspace=None, variant=0, dimension=None, weights=None):
    """tfrt_mixing_error: the MixingError of the columns of ``rows`` -- every group of rays must
    land with the same density on the (ny, nx) bins, whatever that density is.  The columns,
    ``row_x`` / ``row_y`` (-1: one field), ``mask``, ``oob_weight``, ``dimension`` and ``weights``
    are ``density_error``'s, ``grid`` is ``density_grid(domain, nx, ny)``; ``bins`` is ``(nx, ny)``
    (``(nx,)`` or ``nx`` with one field).  ``group``: contiguous int32, one label per SOURCE ray;
    ``perm``: optional int32 (n,), the source ray of column i (None: column i is source ray i);
    ``n_groups``: G, at most ``MIXING_MAX_GROUPS`` with ``G * nx * ny <= MIXING_MAX_CELLS``.  A
    column without a source ray, with a label outside ``[0, G)`` or -- with ``weights`` -- with a
    weight that is not in [0, 1] does not count.  ``variant``: 0 by the number of cells, 1 the
    table in LDS (up to ``MIXING_LDS_CELLS`` cells), 2 global atomics.

    Returns (err {sum, 1, mean}, grad, hq (G, ny, nx) int64 -- (G, nx) with one field --, pull of
    hq's shape float64: D, group_errors (G,) float64: e_g, NaN for a group without mass, used_out
    (2,) float64 {groups used, N}).  ``grad``, ``err``, ``hq``, ``pull``, ``group_errors``,
    ``used_out``, ``workspace`` (uint8): buffers to reuse -- with all of them given a CUDA call
    allocates nothing.  Rows of ``grad`` other than the fields' own (all of them with a direction
    field) are written only when ``grad`` is made here (zeros).

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64
    histogram, the same operations per cell and per ray and the same order of every sum: every
    output agrees bit for bit."""
    what = "mixing_error"
    n_groups = int(n_groups)
    two = row_y >= 0
    counts = (int(bins),) if np.ndim(bins) == 0 else tuple(int(b) for b in bins)
    if len(counts) != (2 if two else 1) or any(c < 1 for c in counts):
        raise ValueError(f"{what}: bins must give one count >= 1 per field, got {bins!r}")
    nx, ny = counts[0], (counts[1] if two else 1)
    if group.dtype != torch.int32 or group.dim() != 1 or not group.is_contiguous():
        raise ValueError(f"{what}: group must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= MIXING_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {MIXING_MAX_GROUPS}")
    if nx * ny > DENSITY_MAX_BINS or n_groups * nx * ny > MIXING_MAX_CELLS:
        raise ValueError(f"{what}: at most {DENSITY_MAX_BINS} bins and {MIXING_MAX_CELLS} cells "
                         "(n_groups * bins)")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups * nx * ny > MIXING_LDS_CELLS):
        raise ValueError(f"{what}: variant must be 0, 1 (up to {MIXING_LDS_CELLS} cells) or 2")
    n = rows.shape[1]
    _check_field_codes(what, rows, row_x, row_y, dimension)
    if weights is not None:
        _check_weights(what, weights)
        if weights.numel() != group.numel():
            raise ValueError(f"{what}: {weights.numel()} weights for {group.numel()} labels -- "
                             "one of each per source ray")
    grad, err = _column_buffers(what, rows, grad, err, mask, perm)
    dev = rows.device
    shape = (n_groups, ny, nx) if two else (n_groups, nx)
    made = dict(hq=(shape, torch.int64), pull=(shape, torch.float64),
                group_errors=((n_groups,), torch.float64), used_out=((2,), torch.float64))
    given = dict(hq=hq, pull=pull, group_errors=group_errors, used_out=used_out)
    for name, (shp, dtype) in made.items():
        if given[name] is None:
            given[name] = torch.empty(shp, dtype=dtype, device=dev)
        b = given[name]
        if tuple(b.shape) != shp or b.dtype != dtype or not b.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dtype} of shape {shp}")
    hq, pull = given["hq"], given["pull"]
    group_errors, used_out = given["group_errors"], given["used_out"]
    if not rows.is_cuda:
        _mixing_error_cpu(rows, row_x, row_y, group, n_groups, nx, ny, grid, float(oob_weight),
                          mask, perm, grad, err, hq, pull, group_errors, used_out, dimension,
                          weights)
        return err, grad, hq, pull, group_errors, used_out
    L = _lib.lib()
    workspace = _column_workspace(
        what, rows, grad, workspace,
        lambda: L.tfrt_mixing_error_workspace_bytes(n, n_groups, nx, ny), group, mask, perm, err,
        hq, pull, group_errors, used_out, weights)
    x0, x1, sx, y0, y1, sy = grid
    # (the field-code form covers plain rows: codes below 2 * dimension are rows of the block)
    check(L.tfrt_mixing_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], 3 if dimension is None else int(dimension),
        _p(mask), row_x, row_y, _p(group), group.numel(), _p(perm), n_groups, _p(weights), nx, ny,
        x0, x1, sx, y0, y1, sy, float(oob_weight), _p(grad), grad.stride(0), _p(err),
        _p(used_out), _p(group_errors), _p(pull), _p(hq), int(variant), _p(workspace),
        workspace.numel(), _stream(rows)), "tfrt_mixing_error")
    return err, grad, hq, pull, group_errors, used_out


def mixing_bins_sum(values):
    """The sums of the rows of ``values`` (G, B) in the fixed shape and order of k_mixing_pulls,
    as float64 torch ops on the CPU: thread j of 1,024 takes the bins j, j + 1024, ... of its
    group in ascending order from 0.0, the 64 lanes of a wave are combined by ``v += v[lane ^ d]``
    for d = 32 .. 1, then the 16 waves in index order from 0.0."""
    T = DISTORTION_BLOCK
    G, B = values.shape
    trips = max((B + T - 1) // T, 1)
    v = torch.zeros((G, trips * T), dtype=torch.float64)
    v[:, :B] = values
    s = torch.zeros((G, T), dtype=torch.float64)
    for trip in range(trips):
        s = s + v[:, trip * T:(trip + 1) * T]   # (squares are >= 0: adding 0.0 changes no bit)
    w = s.view(G, T // 64, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :d] + w[:, :, d:2 * d]
    total = torch.zeros(G, dtype=torch.float64)
    for wave in range(T // 64):
        total = total + w[:, wave, 0]
    return total


def _mixing_tables_cpu(hq2):
    """(pull (G, B), group_errors (G,), used (G,) bool, E_mix, N) of the int64 histogram ``hq2``
    (G, B): mixing_math.h, operation by operation, over all cells at once (CPU)."""
    G, B = hq2.shape
    nq = hq2.sum(dim=1)
    pq = hq2.sum(dim=0)
    Nq = int(nq.sum())
    used = nq > 0
    nan = torch.full((G,), float("nan"), dtype=torch.float64)
    if Nq <= 0:
        return (torch.zeros((G, B), dtype=torch.float64), nan, used,
                torch.zeros((), dtype=torch.float64), 0.0)
    Nf = torch.tensor(float(Nq), dtype=torch.float64)       # (int -> double: to nearest, even)
    N = Nf * 2.3283064365386963e-10
    # (a tensor over a tensor: torch turns ``number / tensor`` into a reciprocal and a product)
    scale = torch.tensor(2.0 * float(B), dtype=torch.float64) / N
    safe = torch.where(used, nq, torch.ones_like(nq)).double()
    d = hq2.double() / safe[:, None] - (pq.double() / Nf)[None, :]
    zero = torch.zeros((), dtype=torch.float64)
    pull = torch.where(used[:, None], scale * d, zero)
    e_g = float(B) * mixing_bins_sum(torch.where(used[:, None], d * d, zero))
    term = (safe / Nf) * e_g
    e_mix = distortion_group_sum(torch.where(used, term, torch.zeros_like(term)), used)
    return pull, torch.where(used, e_g, nan), used, e_mix, float(N)


def _mixing_error_cpu(rows, row_x, row_y, group, n_groups, nx, ny, grid, oob, mask, perm, grad,
                      err, hq, pull, group_errors, used_out, dimension, weights):
    """The CPU path of ``mixing_error`` (every torch op rounds on its own, as the kernels do)."""
    x0, x1, sx, y0, y1, sy = grid
    two = row_y >= 0
    n = rows.shape[1]
    bins = nx * ny
    x, y, link = _fields_cpu(rows, row_x, row_y, dimension)
    counts = torch.isfinite(x) & torch.isfinite(y)
    if mask is not None:
        counts &= mask[:n] >= 0
    w = None
    if weights is not None:
        w, w_ok = _source_weights(weights, perm, n)
        counts &= w_ok
    s = torch.arange(n, dtype=torch.int64) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64)
    label[s_ok] = group[s[s_ok]].long()
    counts &= s_ok & (label >= 0) & (label < n_groups)
    inside, _, gx, gy = _outside_cpu(x, y, two, grid, oob, counts, w)
    zero = torch.zeros((), dtype=torch.float64)
    ex = torch.maximum(x0 - x, zero) + torch.maximum(x - x1, zero)
    ey = (torch.maximum(y0 - y, zero) + torch.maximum(y - y1, zero)) if two \
        else torch.zeros_like(x)
    pens = oob * (ex * ex + ey * ey)
    if w is not None:
        pens = pens * w
    pen = penalty_sum_fixed(pens, counts & ~inside)
    xi, yi, li = x[inside], y[inside], label[inside]
    wi = w[inside] if w is not None else None
    ia, ib, tx = _density_axis(xi, x0, sx, nx)
    flat = hq.view(-1)
    flat.zero_()
    base = li * bins

    def splat(index, b):
        if wi is not None:
            b = b * wi
        flat.index_add_(0, base + index, torch.round(b * DENSITY_FIXED_ONE).long())
    if two:
        ja, jb, ty = _density_axis(yi, y0, sy, ny)
        wx0, wx1, wy0, wy1 = 1.0 - tx, tx, 1.0 - ty, ty
        splat(ja * nx + ia, wy0 * wx0)
        splat(ja * nx + ib, wy0 * wx1)
        splat(jb * nx + ia, wy1 * wx0)
        splat(jb * nx + ib, wy1 * wx1)
    else:
        splat(ia, 1.0 - tx)
        splat(ib, tx)
    D2, e_g, used, e_mix, N = _mixing_tables_cpu(hq.view(n_groups, bins))
    pull.view(n_groups, bins).copy_(D2)
    group_errors.copy_(e_g)
    used_out[0], used_out[1] = float(int(used.sum())), N
    D = D2.reshape(-1)
    if two:
        d00, d01 = D[base + ja * nx + ia], D[base + ja * nx + ib]
        d10, d11 = D[base + jb * nx + ia], D[base + jb * nx + ib]
        gxi = sx * ((1.0 - ty) * (d01 - d00) + ty * (d11 - d10))
        gyi = sy * ((1.0 - tx) * (d10 - d00) + tx * (d11 - d01))
        gy[inside] = gyi if wi is None else gyi * wi
    else:
        gxi = sx * (D[base + ib] - D[base + ia])
    gx[inside] = gxi if wi is None else gxi * wi
    _write_grad_cpu(grad, n, dimension, row_x, row_y, gx, gy, link, counts)
    e = e_mix + pen
    err[0], err[1], err[2] = e, 1.0, e


# ------------------------------------------------------- rays of a group through one point
FOCUS_MAX_GROUPS = 1 << 20
FOCUS_LDS_GROUPS = 256             # tfrt_focus_error: ten planes of G int64 in LDS, 20 KiB
FOCUS_MAX_PBITS = 40
FOCUS_SLOTS = 10                   # {count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty, tz}
_FOCUS_Z_SLOTS = (3, 5, 6, 9)


def focus_pbits(n_source):
    """Fraction bits of tfrt_focus_error's fixed point for a source of ``n_source`` rays:
    ``min(40, 60 - bit_length(n_source))`` -- every entry is below 2 in absolute value, so no
    int64 sum can overflow."""
    return min(FOCUS_MAX_PBITS, 60 - int(n_source).bit_length())


def focus_grid(domain):
    """The box constants of tfrt_focus_error from ``domain`` = ((x0, x1), (y0, y1)[, (z0, z1)]):
    ``(x0, x1, y0, y1, z0, z1, cx, cy, cz, R, iR)`` in float64 -- the box, its centre
    ``c = 0.5 * (lo + hi)``, ``R`` the largest half-width ``0.5 * (hi - lo)`` and ``iR = 1 / R``,
    each computed once here; a 2-D domain leaves the z entries 0."""
    try:
        box = [(float(d[0]), float(d[1])) for d in domain]
    except (IndexError, TypeError) as e:
        raise ValueError("focus_grid: domain must be ((x0, x1), (y0, y1)) or "
                         "((x0, x1), (y0, y1), (z0, z1))") from e
    if len(box) not in (2, 3) \
            or any(not (np.isfinite(a) and np.isfinite(b) and b > a) for a, b in box):
        raise ValueError("focus_grid: domain needs one finite (lo, hi), lo < hi, per axis of a "
                         f"2-D or 3-D trace; got {domain!r}")
    box += [(0.0, 0.0)] * (3 - len(box))
    lo = np.array([b[0] for b in box], dtype=np.float64)
    hi = np.array([b[1] for b in box], dtype=np.float64)
    c = 0.5 * (lo + hi)
    R = np.float64(max(0.5 * (hi - lo)))
    iR = np.float64(1.0) / R
    if not (np.isfinite(R) and np.isfinite(iR)):
        raise ValueError(f"focus_grid: the box {domain!r} has no finite half-width")
    return tuple(float(v) for b in box for v in b) + tuple(float(v) for v in c) \
        + (float(R), float(iR))


def _focus_columns(rows, group, n_groups, grid, mask, perm, dimension):
    """(counts, label, u, m, L) of the columns of the geometry block ``rows``, the operations of
    tfrt_focus_error one by one as torch ops (on the block's device): which columns count, their
    group (clamped into [0, G) where a column does not count), the link's direction, the
    normalised end point and the link's length."""
    d = dimension
    n = rows.shape[1]
    dev = rows.device
    _, e, u, L, ok = _link_torch(rows, d)
    counts = ok if mask is None else ok & (mask[:n] >= 0)
    s = torch.arange(n, dtype=torch.int64, device=dev) if perm is None else perm[:n].long()
    s_ok = (s >= 0) & (s < group.numel())
    label = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if group.numel() > 0:
        label = torch.where(s_ok, group[s.clamp(0, group.numel() - 1)].long(), label)
    counts = counts & s_ok & (label >= 0) & (label < n_groups)
    for a in range(d):
        counts = counts & (e[a] >= grid[2 * a]) & (e[a] <= grid[2 * a + 1])
    c = torch.tensor(grid[6:6 + d], dtype=torch.float64, device=dev)[:, None]
    m = (e - c) * grid[10]
    return counts, label.clamp(0, n_groups - 1), u, m, L


def _dot_rows(v, w):
    """v . w of two (d, n) blocks, the products summed left to right."""
    s = v[0] * w[0] + v[1] * w[1]
    return s + v[2] * w[2] if v.shape[0] == 3 else s


def _focus_solve(acc, pbits, min_det, d):
    """The (G, 4) table {x, y, z, has_focus} of a (G, 10) record table: focus_math.h's
    focus_solve, operation by operation, over all groups at once."""
    inv = float(np.ldexp(1.0, -int(pbits)))
    cnt = acc[:, 0]
    n = cnt.double()
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (
        (acc[:, p].double() * inv) / n for p in (1, 2, 3, 4, 5, 6, 7, 8, 9))
    if d == 2:
        det = a00 * a11 - a01 * a01
        xs = [(a11 * b0 - a01 * b1) / det, (a00 * b1 - a01 * b0) / det, torch.zeros_like(det)]
    else:
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = a00 * c00 + a01 * c01 + a02 * c02
        xs = [(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det,
              (c02 * b0 + c12 * b1 + c22 * b2) / det]
    has = (cnt >= 2) & (det >= min_det)
    nan = torch.full_like(det, float("nan"))
    return torch.stack([torch.where(has, x, nan) for x in xs] + [has.double()], dim=1)


def _focus_terms(counts, label, u, m, L, foci, R):
    """(has, term, g_start, g_end) of the columns against the table ``foci``: focus_math.h's
    focus_term; ``has``: the column counts and its group has a focus (the others hold garbage)."""
    d = u.shape[0]
    f = foci[label]
    has = counts & (f[:, 3] != 0.0)
    q = m - f[:, :d].t()
    a = _dot_rows(u, q)
    rho = R * (q - a * u)
    lever = (R * a) / L
    two = 2.0 * rho
    return has, _dot_rows(rho, rho), two * lever, two * (1.0 - lever)


def focus_terms(rows, group, n_groups, grid, foci, mask=None, perm=None, dimension=3):
    """The (n,) float64 terms of a tfrt_focus_error evaluation from its table ``foci``, as torch
    ops on the block's device: the squared distance of the group's focus from a ray's line, 0 for
    a ray without a term."""
    counts, label, u, m, L = _focus_columns(rows, group, int(n_groups), grid, mask, perm,
                                            dimension)
    has, term, _, _ = _focus_terms(counts, label, u, m, L, foci, grid[9])
    return torch.where(has, term, torch.zeros_like(term))


def focus_points(foci, grid, dimension=3):
    """The (G, dimension) float64 foci in scene coordinates, ``c + R * x``, from the (G, 4) table
    of tfrt_focus_error; NaN for a group without a focus."""
    d = int(dimension)
    c = torch.tensor(grid[6:6 + d], dtype=torch.float64, device=foci.device)
    return c + grid[9] * foci[:, :d]


def focus_error(rows, groups, n_groups, grid, min_det, mask=None, perm=None, dimension=3,
                grad=None, err=None, acc=None, foci=None, workspace=None, variant=0):
    """tfrt_focus_error: the FocusError of the columns of the (2 * dimension, n) geometry block
    ``rows`` -- rays of one group, taken as lines, must pass through one common point.
    ``groups``: contiguous int32 labels, one per SOURCE ray; ``perm``: optional int32 (n,), the
    source ray of column i (None: column i is source ray i); ``n_groups``: G, labels outside
    [0, G) have no term; ``grid`` from ``focus_grid``; ``min_det``: a group has a focus if it has
    at least two rays and ``det(A / count) >= min_det``; ``mask``: optional int32, column i counts
    if mask[i] >= 0.  The fixed point has ``focus_pbits(groups.numel())`` fraction bits.  Returns
    (err {sum, terms, mean}, grad (2 * dimension, n) float64 -- every row written for every
    column --, acc (G, 10) int64 {count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty, tz}, foci (G, 4)
    float64 {x, y, z, has_focus} in normalised coordinates (``focus_points`` gives the scene's),
    NaN for a group without a focus).  ``grad``, ``err``, ``acc``, ``foci``, ``workspace`` (uint8):
    buffers to reuse -- with all five given a CUDA call allocates nothing.  ``variant``: 0 by G,
    1 the table in LDS, 2 global atomics.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64 fixed
    point and the same operations, each rounded on its own (``acc``, ``foci`` and the gradient
    agree bit for bit; the error sum is torch's and agrees to rounding)."""
    n_groups = int(n_groups)
    if groups.dtype != torch.int32 or groups.dim() != 1 or not groups.is_contiguous():
        raise ValueError("focus_error: groups must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= FOCUS_MAX_GROUPS:
        raise ValueError(f"focus_error: n_groups must lie in 1 .. {FOCUS_MAX_GROUPS}")
    if dimension not in (2, 3) or rows.dim() != 2 or rows.shape[0] != 2 * dimension:
        raise ValueError("focus_error: rows must be the (2 * dimension, n) geometry block of a "
                         f"2-D or 3-D trace, got dimension {dimension!r} and shape "
                         f"{tuple(rows.shape)}")
    if len(grid) != 11:
        raise ValueError("focus_error: grid must come from focus_grid")
    min_det = float(min_det)
    if not (min_det > 0.0 and np.isfinite(min_det)):
        raise ValueError("focus_error: min_det must be finite and > 0")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups > FOCUS_LDS_GROUPS):
        raise ValueError(f"focus_error: variant must be 0, 1 (up to {FOCUS_LDS_GROUPS} groups) "
                         "or 2")
    n = rows.shape[1]
    pbits = focus_pbits(groups.numel())
    if n >= 1 << (61 - pbits):
        raise ValueError("focus_error: more columns than the source's fixed point allows "
                         "(n < 2^(61 - pbits))")
    grad, err = _column_buffers("focus_error", rows, grad, err, mask, perm)
    if acc is None:
        acc = torch.empty((n_groups, FOCUS_SLOTS), dtype=torch.int64, device=rows.device)
    if tuple(acc.shape) != (n_groups, FOCUS_SLOTS) or acc.dtype != torch.int64 \
            or not acc.is_contiguous():
        raise ValueError(f"focus_error: acc must be contiguous int64 of shape (n_groups, "
                         f"{FOCUS_SLOTS})")
    if foci is None:
        foci = torch.empty((n_groups, 4), dtype=torch.float64, device=rows.device)
    if tuple(foci.shape) != (n_groups, 4) or foci.dtype != torch.float64 \
            or not foci.is_contiguous():
        raise ValueError("focus_error: foci must be contiguous float64 of shape (n_groups, 4)")
    if not rows.is_cuda:
        _focus_error_cpu(rows, groups, n_groups, grid, min_det, mask, perm, dimension, grad, err,
                         acc, foci, pbits)
        return err, grad, acc, foci
    L = _lib.lib()
    workspace = _column_workspace(
        "focus_error", rows, grad, workspace,
        lambda: L.tfrt_focus_error_workspace_bytes(n, n_groups), groups, mask, perm, err, acc, foci)
    check(L.tfrt_focus_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], int(dimension), _p(mask), _p(groups),
        groups.numel(), _p(perm), n_groups, *grid[:6], pbits, min_det, _p(grad), grad.stride(0),
        _p(err), _p(acc), _p(foci), int(variant), _p(workspace), workspace.numel(),
        _stream(rows)), "tfrt_focus_error")
    return err, grad, acc, foci


def _focus_error_cpu(rows, groups, n_groups, grid, min_det, mask, perm, d, grad, err, acc, foci,
                     pbits):
    """The CPU path of ``focus_error`` (every torch op rounds on its own, as the kernels do)."""
    n = rows.shape[1]
    counts, label, u, m, L = _focus_columns(rows, groups, n_groups, grid, mask, perm, d)
    _focus_records_cpu(acc, counts, label, u, m, pbits, d)
    foci.copy_(_focus_solve(acc, pbits, min_det, d))
    has, term, gs, ge = _focus_terms(counts, label, u, m, L, foci, grid[9])
    zero = torch.zeros((), dtype=torch.float64)
    for b in range(d):
        grad[b, :n] = torch.where(has, gs[b], zero)
        grad[d + b, :n] = torch.where(has, ge[b], zero)
    n_terms = int(has.sum())
    e = term[has].sum()
    err[0], err[1] = e, float(n_terms)
    err[2] = e / n_terms if n_terms > 0 else float("nan")


def _focus_records_cpu(acc, counts, label, u, m, pbits, d):
    """The (G, 10) records of the counting columns into ``acc``: P = I - u u^T and
    t = m - (u . m) u as integers."""
    one = float(np.ldexp(1.0, pbits))
    w = _dot_rows(u, m)
    pairs = {1: (0, 0), 2: (0, 1), 3: (0, 2), 4: (1, 1), 5: (1, 2), 6: (2, 2)}
    li = label[counts]
    acc.zero_()
    acc[:, 0].index_add_(0, li, torch.ones_like(li))
    for p in range(1, FOCUS_SLOTS):
        if d == 2 and p in _FOCUS_Z_SLOTS:
            continue
        if p < 7:
            a, b = pairs[p]
            v = 1.0 - u[a] * u[a] if a == b else -(u[a] * u[b])
        else:
            v = m[p - 7] - w * u[p - 7]
        acc[:, p].index_add_(0, li, torch.round(v[counts] * one).long())


# ------------------------------------------------------- the foci of all groups in one plane
FLATFIELD_ROW = 8                  # {x0, x1, x2, used, mu0, mu1, mu2, e_g}: one 64-byte line
FLATFIELD_BLOCK = DISTORTION_BLOCK  # k_flatfield_fit: one workgroup of 16 waves


def flatfield_axis(axis, dimension=3):
    """The unit normal of tfrt_flatfield_error from ``axis``, ``dimension`` numbers that are finite
    and not all zero: ``axis / sqrt(axis . axis)`` in float64, the products summed left to right,
    formed once here; a tuple of three floats (2-D: the third is 0.0)."""
    d = int(dimension)
    try:
        a = [np.float64(v) for v in axis]
    except (TypeError, ValueError) as e:
        raise ValueError(f"flatfield_axis: axis must be {d} numbers, got {axis!r}") from e
    if len(a) != d or not all(np.isfinite(v) for v in a) or not any(v != 0.0 for v in a):
        raise ValueError(f"flatfield_axis: axis must be {d} finite numbers, not all zero; got "
                         f"{axis!r}")
    s = a[0] * a[0] + a[1] * a[1]
    if d == 3:
        s = s + a[2] * a[2]
    r = np.sqrt(s)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"flatfield_axis: the length of {axis!r} is not a finite number > 0")
    return tuple(float(v / r) for v in a) + (0.0,) * (3 - d)


def _flatfield_fit(acc, pbits, min_det, d, a, grid):
    """(table (G, 8), fit_out (8,), inside error, number of terms) of a (G, 10) record table on
    the CPU: flatfield_math.h and k_flatfield_fit, operation by operation, over all groups at once,
    the sums over the groups in the kernel's shape and order (``distortion_group_sum``)."""
    G = acc.shape[0]
    R = grid[9]
    foci = _focus_solve(acc, pbits, min_det, d)
    used = foci[:, 3] != 0.0
    x = foci[:, :3]
    # y = A^-1 a by the cofactors of _focus_solve
    inv = float(np.ldexp(1.0, -int(pbits)))
    n = acc[:, 0].double()
    a00, a01, a02, a11, a12, a22 = ((acc[:, p].double() * inv) / n for p in (1, 2, 3, 4, 5, 6))
    if d == 2:
        det = a00 * a11 - a01 * a01
        ys = [(a11 * a[0] - a01 * a[1]) / det, (a00 * a[1] - a01 * a[0]) / det]
        h = a[0] * x[:, 0] + a[1] * x[:, 1]
    else:
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = a00 * c00 + a01 * c01 + a02 * c02
        ys = [(c00 * a[0] + c01 * a[1] + c02 * a[2]) / det,
              (c01 * a[0] + c11 * a[1] + c12 * a[2]) / det,
              (c02 * a[0] + c12 * a[1] + c22 * a[2]) / det]
        h = a[0] * x[:, 0] + a[1] * x[:, 1] + a[2] * x[:, 2]
    gsum = lambda v: distortion_group_sum(v, used)          # noqa: E731
    W, S = gsum(n), gsum(n * h)
    n_used = int(used.sum())
    terms = int(acc[used, 0].sum())
    hbar = S / W
    valid = n_used >= 2
    table = torch.zeros((G, FLATFIELD_ROW), dtype=torch.float64)
    table[:, :3] = x                                        # (NaN without a focus)
    table[:, 3] = used.double()
    inside = torch.zeros((), dtype=torch.float64)
    if valid:
        zero = torch.zeros((), dtype=torch.float64)
        s = R * (h - hbar)
        two = 2.0 * s
        e = s * s
        for b, y in enumerate(ys):
            table[:, 4 + b] = torch.where(used, two * y, zero)
        table[:, 7] = torch.where(used, e, zero)
        inside = gsum(n * e)
    c = grid[6:9]
    ac = a[0] * c[0] + a[1] * c[1]
    if d == 3:
        ac = ac + a[2] * c[2]
    fit = torch.zeros(8, dtype=torch.float64)
    fit[0], fit[1], fit[2] = hbar, ac + R * float(hbar), W
    fit[3], fit[4] = float(n_used), float(valid)
    return table, fit, inside, terms


def _flatfield_rays(counts, label, u, m, L, table, R, valid):
    """(has, g_start, g_end) of the columns against the table: flatfield_math.h's flatfield_ray;
    ``has``: the column counts, its group is used and the plane is valid (the others hold
    garbage)."""
    d = u.shape[0]
    f = table[label]
    has = counts & (f[:, 3] != 0.0) & valid
    q = m - f[:, :d].t()
    alpha = _dot_rows(u, q)
    lever = (R * alpha) / L
    rest = 1.0 - lever
    mu = f[:, 4:4 + d].t()
    beta = _dot_rows(mu, u)
    k = beta / L
    rho = R * (q - alpha * u)
    muP = mu - beta * u
    turn = k * rho
    return has, muP * lever + turn, muP * rest - turn


def flatfield_terms(rows, group, n_groups, grid, table, mask=None, perm=None, dimension=3):
    """The (n,) float64 terms of a tfrt_flatfield_error evaluation from its ``table``, as torch
    ops on the block's device: ``e_g`` of the ray's own group -- the squared distance of the
    group's focus from the plane -- for a counting ray of a used group, 0 for every other ray."""
    counts, label, _, _, _ = _focus_columns(rows, group, int(n_groups), grid, mask, perm,
                                            dimension)
    f = table[label]
    return torch.where(counts & (f[:, 3] != 0.0), f[:, 7], torch.zeros_like(f[:, 7]))


def flatfield_error(rows, groups, n_groups, grid, axis, min_det, mask=None, perm=None,
                    dimension=3, variant=0, grad=None, err=None, acc=None, table=None,
                    fit_out=None, workspace=None):
    """tfrt_flatfield_error: the FlatFieldError of the columns of the (2 * dimension, n) geometry
    block ``rows`` -- the foci of all groups (``focus_error``'s, from the same records) must lie
    in one plane with the normal ``axis``, wherever along the normal it has to stand.  ``rows``,
    ``groups``, ``perm``, ``n_groups``, ``grid`` (``focus_grid``), ``min_det``, ``mask`` and
    ``variant`` are ``focus_error``'s; ``axis``: ``dimension`` finite numbers, not all zero,
    normalised once here (``flatfield_axis``).  Returns (err {sum, terms, mean}, grad
    (2 * dimension, n) float64 -- every row written for every column --, acc (G, 10) int64, table
    (G, 8) float64 {x0, x1, x2, used, mu0, mu1, mu2, e_g} -- the focus in normalised coordinates
    (``focus_points`` gives the scene's), NaN and zeros for a group without a focus; mu and e_g 0
    without a valid plane --, fit_out (8,) float64 {hbar, a . c + R * hbar, W, groups used, valid,
    0, 0, 0}).  ``grad``, ``err``, ``acc``, ``table``, ``fit_out``, ``workspace`` (uint8): buffers
    to reuse -- with all six given a CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same int64 fixed
    point, the same operations and the same order of the sums over the groups: ``acc``, ``table``,
    ``fit_out``, the gradient and the error agree bit for bit."""
    what = "flatfield_error"
    n_groups = int(n_groups)
    if groups.dtype != torch.int32 or groups.dim() != 1 or not groups.is_contiguous():
        raise ValueError(f"{what}: groups must be a contiguous int32 vector, one label per "
                         "source ray")
    if not 1 <= n_groups <= FOCUS_MAX_GROUPS:
        raise ValueError(f"{what}: n_groups must lie in 1 .. {FOCUS_MAX_GROUPS}")
    if dimension not in (2, 3) or rows.dim() != 2 or rows.shape[0] != 2 * dimension:
        raise ValueError(f"{what}: rows must be the (2 * dimension, n) geometry block of a "
                         f"2-D or 3-D trace, got dimension {dimension!r} and shape "
                         f"{tuple(rows.shape)}")
    if len(grid) != 11:
        raise ValueError(f"{what}: grid must come from focus_grid")
    try:
        a = flatfield_axis(axis, dimension)
    except ValueError as e:
        raise ValueError(f"{what}: axis must be {dimension} finite numbers, not all zero; got "
                         f"{axis!r}") from e
    min_det = float(min_det)
    if not (min_det > 0.0 and np.isfinite(min_det)):
        raise ValueError(f"{what}: min_det must be finite and > 0")
    if variant not in (0, 1, 2) or (variant == 1 and n_groups > FOCUS_LDS_GROUPS):
        raise ValueError(f"{what}: variant must be 0, 1 (up to {FOCUS_LDS_GROUPS} groups) or 2")
    n = rows.shape[1]
    pbits = focus_pbits(groups.numel())
    if n >= 1 << (61 - pbits):
        raise ValueError(f"{what}: more columns than the source's fixed point allows "
                         "(n < 2^(61 - pbits))")
    grad, err = _column_buffers(what, rows, grad, err, mask, perm)
    dev = rows.device
    made = dict(acc=((n_groups, FOCUS_SLOTS), torch.int64),
                table=((n_groups, FLATFIELD_ROW), torch.float64), fit_out=((8,), torch.float64))
    given = dict(acc=acc, table=table, fit_out=fit_out)
    for name, (shape, dtype) in made.items():
        if given[name] is None:
            given[name] = torch.empty(shape, dtype=dtype, device=dev)
        b = given[name]
        if tuple(b.shape) != shape or b.dtype != dtype or not b.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous {dtype} of shape {shape}")
    acc, table, fit_out = given["acc"], given["table"], given["fit_out"]
    if not rows.is_cuda:
        _flatfield_error_cpu(rows, groups, n_groups, grid, a, min_det, mask, perm, dimension,
                             grad, err, acc, table, fit_out, pbits)
        return err, grad, acc, table, fit_out
    if table.data_ptr() % 64 != 0:
        raise ValueError(f"{what}: table must be 64-byte aligned")
    L = _lib.lib()
    workspace = _column_workspace(
        what, rows, grad, workspace,
        lambda: L.tfrt_flatfield_error_workspace_bytes(n, n_groups), groups, mask, perm, err, acc,
        table, fit_out)
    check(L.tfrt_flatfield_error(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], int(dimension), _p(mask), _p(groups),
        groups.numel(), _p(perm), n_groups, *grid[:6], pbits, min_det, *a, _p(grad),
        grad.stride(0), _p(err), _p(acc), _p(table), _p(fit_out), int(variant), _p(workspace),
        workspace.numel(), _stream(rows)), "tfrt_flatfield_error")
    return err, grad, acc, table, fit_out


def _flatfield_error_cpu(rows, groups, n_groups, grid, a, min_det, mask, perm, d, grad, err, acc,
                         table, fit_out, pbits):
    """The CPU path of ``flatfield_error`` (every torch op rounds on its own, as the kernels
    do)."""
    n = rows.shape[1]
    counts, label, u, m, L = _focus_columns(rows, groups, n_groups, grid, mask, perm, d)
    _focus_records_cpu(acc, counts, label, u, m, pbits, d)
    t, fit, inside, terms = _flatfield_fit(acc, pbits, min_det, d, a, grid)
    table.copy_(t)
    fit_out.copy_(fit)
    has, gs, ge = _flatfield_rays(counts, label, u, m, L, table, grid[9], bool(fit[4] != 0.0))
    zero = torch.zeros((), dtype=torch.float64)
    for b in range(d):
        grad[b, :n] = torch.where(has, gs[b], zero)
        grad[d + b, :n] = torch.where(has, ge[b], zero)
    err[0], err[1] = inside, float(terms)
    err[2] = inside / terms if terms > 0 else float("nan")


# ------------------------------------------------------- a sum of error terms (SumError)

COMBINE_MAX_TERMS = _lib.COMBINE_MAX_TERMS


def goal_error_columns(rows, fields, goal, mask=None, perm=None, by_ray=False, n_source=None,
                       grad=None, err=None, workspace=None):
    """tfrt_goal_error_columns: GoalError on fixed-shape columns.  ``rows``: the (4 or 6, n) ray
    block (float32 / float64 / float16, contiguous columns, any row stride); ``fields``: the
    distinct rows compared with the goal's columns; ``goal``: contiguous float64, (len(fields),
    n_source) or -- ``by_ray`` -- (n_source, len(fields)), one entry per field and SOURCE ray;
    ``mask``: optional int32, column i counts if mask[i] >= 0; ``perm``: optional int32 (n,), the
    source ray of column i (None: column i is source ray i); a column whose source ray lies
    outside [0, n_source) does not count (``n_source``: the goal's ray count unless given
    smaller).  Returns (err {sum, terms, mean}, grad (rows, n) float64): the rows of ``fields`` are
    written for every column (0.0 where it does not count), other rows only when ``grad`` is made
    here (zeros).  ``grad``, ``err``, ``workspace`` (uint8): buffers to reuse -- with all three
    given a CUDA call allocates nothing.

    CUDA tensors run the kernels.  CPU tensors run a torch restatement with the same operations
    per column, each rounded on its own (the gradient agrees bit for bit; the error sum is torch's
    and agrees to rounding)."""
    k, n = rows.shape
    fields = [int(f) for f in fields]
    nf = len(fields)
    if k not in (4, 6) or not 1 <= nf <= k or any(not 0 <= f < k for f in fields) \
            or len(set(fields)) != nf:
        raise ValueError(f"goal_error_columns: a block of 4 or 6 rows and 1 .. rows distinct "
                         f"fields inside it, got {k} rows and fields {fields}")
    if goal.dtype != torch.float64 or goal.dim() != 2 or not goal.is_contiguous() \
            or goal.shape[1 if by_ray else 0] != nf:
        raise ValueError("goal_error_columns: goal must be contiguous float64 (fields, n_source), "
                         "or (n_source, fields) with by_ray")
    rays = goal.shape[0 if by_ray else 1]
    n_source = rays if n_source is None else int(n_source)
    if not 0 <= n_source <= rays:
        raise ValueError(f"goal_error_columns: n_source must lie in 0 .. {rays}")
    grad, err = _column_buffers("goal_error_columns", rows, grad, err, mask, perm)
    strides = (1, nf) if by_ray else (rays, 1)
    if not rows.is_cuda:
        _goal_error_columns_cpu(rows, fields, goal, mask, perm, by_ray, n_source, grad, err)
        return err, grad
    L = _lib.lib()
    workspace = _column_workspace(
        "goal_error_columns", rows, grad, workspace,
        lambda: L.tfrt_goal_error_columns_workspace_bytes(n), goal, mask, perm, err)
    codes = (ctypes.c_int32 * nf)(*fields)
    check(L.tfrt_goal_error_columns(
        _p(rows), rows.stride(0), n, _DT[rows.dtype], k, _p(mask), _p(perm), n_source, codes, nf,
        _p(goal), strides[0], strides[1], _p(grad), grad.stride(0), _p(err), _p(workspace),
        workspace.numel(), _stream(rows)), "tfrt_goal_error_columns")
    return err, grad


def _goal_error_columns_cpu(rows, fields, goal, mask, perm, by_ray, n_source, grad, err):
    """The CPU path of ``goal_error_columns`` (every torch op rounds on its own, as the kernels
    do)."""
    n = rows.shape[1]
    counts = torch.ones(n, dtype=torch.bool)
    if mask is not None:
        counts &= mask[:n] >= 0
    s = perm[:n].long() if perm is not None else torch.arange(n)
    counts &= (s >= 0) & (s < n_source)
    s = s.clamp(0, max(n_source - 1, 0))
    zero = torch.zeros((), dtype=torch.float64)
    total = torch.zeros((), dtype=torch.float64)
    for c, f in enumerate(fields):
        if n_source > 0:
            g = goal[s, c] if by_ray else goal[c, s]
            d = torch.where(counts, rows[f].double() - g, zero)
        else:
            d = torch.zeros(n, dtype=torch.float64)
        total = total + (d * d).sum()
        # (a column that does not count gets +0.0, not 2 * 0.0 with the residual's sign)
        grad[f, :n] = torch.where(counts, 2.0 * d, zero)
    terms = float(len(fields) * int(counts.sum()))
    err[0], err[1] = total, terms
    err[2] = total / terms if terms > 0 else float("nan")


def error_combine(terms, weights, reduce="sum", n=None, n_rows=6, out=None, err=None, coeff=None):
    """tfrt_error_combine: the weighted sum of 1 .. 8 error terms in one launch.  ``terms``: a
    sequence of ``(grad, row_mask, error)`` -- ``grad`` a float64 seed block of ``n_rows`` rows
    with contiguous columns (or None in EVERY term: only the errors are combined), ``row_mask``
    the rows the term wrote (bit r for row r), ``error`` its float64 triple {sum, terms, mean}.
    ``weights``: contiguous float64 (K,) on the terms' device; ``reduce``: "sum", c_k = w_k, or
    "mean", c_k = w_k / terms_k (0 for a term without terms), terms_k read from the triple.
    ``n``: the columns (default: the first block's).  Returns (err {E, 1, E}, out (n_rows, n)
    float64 or None, coeff (K,)): row r of ``out`` is ``c_k * g_k[r]`` of the first term naming
    it, plus ``c_k * g_k[r]`` of every later one, each product and sum rounded on its own; 0.0
    for a row nobody names.  ``out`` (it must not overlap a term's block), ``err``, ``coeff``:
    buffers to reuse -- with all three given a CUDA call allocates nothing.

    CUDA tensors run the kernel; CPU tensors a torch restatement with the same operations in the
    same order (every result agrees bit for bit)."""
    terms = list(terms)
    K = len(terms)
    if reduce not in ("sum", "mean"):
        raise ValueError(f"error_combine: reduce must be 'sum' or 'mean', got {reduce!r}")
    if not 1 <= K <= COMBINE_MAX_TERMS:
        raise ValueError(f"error_combine: 1 .. {COMBINE_MAX_TERMS} terms, got {K}")
    if n_rows not in (4, 6):
        raise ValueError(f"error_combine: n_rows must be 4 or 6, got {n_rows!r}")
    if weights.dtype != torch.float64 or tuple(weights.shape) != (K,) \
            or not weights.is_contiguous():
        raise ValueError(f"error_combine: weights must be contiguous float64 ({K},)")
    grads = [t[0] for t in terms]
    with_grad = any(g is not None for g in grads)
    if with_grad and any(g is None for g in grads):
        raise ValueError("error_combine: every term needs a gradient block, or none has one")
    if n is None:
        n = grads[0].shape[1] if with_grad else 0
    n = int(n)
    for g, row_mask, e in terms:
        if e.dtype != torch.float64 or e.numel() != 3 or not e.is_contiguous():
            raise ValueError("error_combine: a term's error must be 3 contiguous float64")
        if not 0 <= int(row_mask) < (1 << n_rows):
            raise ValueError(f"error_combine: row_mask {row_mask!r} names a row outside the "
                             f"{n_rows} of the block")
        if g is not None and (g.dtype != torch.float64 or g.dim() != 2 or g.shape[0] != n_rows
                              or g.shape[1] < n):
            raise ValueError(f"error_combine: a term's grad must be float64 ({n_rows}, {n})")
    dev = weights.device
    if with_grad and n > 0:
        if out is None:
            out = torch.empty((n_rows, n), dtype=torch.float64, device=dev)
        if out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] != n_rows \
                or out.shape[1] < n:
            raise ValueError(f"error_combine: out must be float64 ({n_rows}, {n})")
    if err is None:
        err = torch.empty(3, dtype=torch.float64, device=dev)
    if coeff is None:
        coeff = torch.empty(K, dtype=torch.float64, device=dev)
    if coeff.dtype != torch.float64 or tuple(coeff.shape) != (K,) or not coeff.is_contiguous():
        raise ValueError(f"error_combine: coeff must be contiguous float64 ({K},)")
    if not weights.is_cuda:
        _error_combine_cpu(terms, weights, reduce, n if with_grad else 0, n_rows, out, err, coeff)
        return err, out, coeff
    _need_gpu(weights, out, err, coeff, *grads, *(t[2] for t in terms))
    if with_grad and n > 0 and any(t.stride(1) != 1 for t in grads + [out]):
        raise ValueError("error_combine: the blocks must have contiguous columns")
    desc = (_lib.CombineTerm * K)()
    for d, (g, row_mask, e) in zip(desc, terms):
        d.grad = None if g is None else g.data_ptr()
        d.stride = 0 if g is None else g.stride(0)
        d.row_mask = int(row_mask)
        d.error = e.data_ptr()
    check(_lib.lib().tfrt_error_combine(
        desc, K, _p(weights), 0 if reduce == "sum" else 1, n, n_rows, _p(out),
        0 if out is None else out.stride(0), _p(err), _p(coeff), _stream(weights)),
        "tfrt_error_combine")
    return err, out, coeff


def _error_combine_cpu(terms, weights, reduce, n, n_rows, out, err, coeff):
    """The CPU path of ``error_combine`` (every torch op rounds on its own, as the kernel does)."""
    cs = []
    for k, (_, _, e) in enumerate(terms):
        if reduce == "sum":
            c = weights[k].clone()
        else:
            c = weights[k] / e[1] if float(e[1]) > 0.0 else torch.zeros((), dtype=torch.float64)
        cs.append(c)
        coeff[k] = c
    total = cs[0] * terms[0][2][0]
    for c, (_, _, e) in zip(cs[1:], terms[1:]):
        total = total + c * e[0]
    err[0], err[1], err[2] = total, 1.0, total
    if n <= 0 or out is None:
        return
    for r in range(n_rows):
        acc = None
        for c, (g, row_mask, _) in zip(cs, terms):
            if (int(row_mask) >> r) & 1:
                p = c * g[r, :n]
                acc = p if acc is None else acc + p
        out[r, :n] = 0.0 if acc is None else acc


def restore_plan(ids, counts_dev, P, cls_col, perm, n_src, n_rows=None, total=None, zero=False):
    """(inv, dest_of, original ids) of one output class of a trace over permuted rays
    (tfrt_restore_order): row j of the class in the reference's order = row ``inv[j]`` of the
    trace's output, ``dest_of`` is the inverse.  ``cls_col``: the class's TFRT_CLS_* column of
    ``counts_dev`` (the device counts of the trace), or None: ``ids`` is one segment (the
    unfinished set; ``total``: its row count as an int32 device scalar, default all of ``ids``).
    Entries beyond the class's row count are not written."""
    cap = ids.numel() if n_rows is None else int(n_rows)
    dev = ids.device
    new = torch.zeros if zero else torch.empty    # (zero: rows past the count must be valid indices)
    inv = new(cap, dtype=torch.int32, device=dev)
    dest = new(cap, dtype=torch.int32, device=dev)
    ids_o = new(cap, dtype=torch.int32, device=dev)
    if cap == 0:
        return inv, dest, ids_o
    L = _lib.lib()
    nseg = int(P) if cls_col is not None else 1
    wsb = L.tfrt_restore_order_workspace_bytes(int(n_src), nseg)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    if cls_col is not None:
        base = counts_dev.data_ptr()
        seg_n = ctypes.c_void_p(base + 4 * cls_col)
        seg_b = ctypes.c_void_p(base + 4 * (4 + cls_col))
        total = ctypes.c_void_p(base + 4 * (_lib.COUNTS_PER_PASS * int(P) + cls_col))
        check(L.tfrt_restore_order(_p(ids), cap, seg_n, seg_b, _lib.COUNTS_PER_PASS, nseg, total,
                                   _p(perm), int(n_src), _p(inv), _p(dest), _p(ids_o), _p(ws), wsb,
                                   _stream(ids)), "tfrt_restore_order")
    else:
        check(L.tfrt_restore_order(_p(ids), cap, None, None, 1, 1, _p(total), _p(perm), int(n_src),
                                   _p(inv), _p(dest), _p(ids_o), _p(ws), wsb, _stream(ids)),
              "tfrt_restore_order")
    return inv, dest, ids_o


def restore_order(out, perm):
    """Outputs of a trace over PERMUTED rays (``permute_rays(src, perm)``, e.g. ``perm =
    ray_order(src)``, the form tfrt_scene3d.coherent_rays wants) brought back to what the trace of
    ``src`` itself gives: ray ids mapped through ``perm``, and inside every class the rays of one
    pass sorted by ray id again (the reference's per-pass boolean_mask order,
    engine.py:2069-2111).  ``out``: the dict of trace3d(); returns a new dict.  Device kernels
    (tfrt_restore_order, tfrt_gather_rows): a counting sort by (pass, original id), no host sync."""
    n_src = perm.numel()
    counts_dev = out["counts_dev"]
    P = out["counts"].shape[0]
    new = dict(out)

    def rows(t, inv):
        if t.requires_grad:
            return t.index_select(t.dim() - 1, inv.long())
        return gather_rows(t, inv)

    for col, cls in enumerate(_CLASS_NAMES_BY_COUNT_COLUMN):
        if cls not in out or out[cls].shape[1] == 0 or out.get(cls + "_id") is None:
            continue
        n = out[cls].shape[1]
        inv, _, ids_o = restore_plan(out[cls + "_id"], counts_dev, P, col, perm, n_src, n)
        new[cls] = rows(out[cls], inv)
        new[cls + "_id"] = ids_o
        if out.get(cls + "_face") is not None:
            new[cls + "_face"] = gather_rows(out[cls + "_face"], inv)
        new.pop(cls + "_rows", None)
    if "unfinished" in out and out["unfinished"].shape[1]:
        n_u = out["unfinished"].shape[1]
        inv, _, ids_o = restore_plan(out["unfinished_id"], None, 0, None, perm, n_src, n_u)
        new["unfinished"] = rows(out["unfinished"], inv)
        new["unfinished_id"] = ids_o
    return new


def source3d_order(program, n, first=0, face_verts=None, axis=None, out=None, device=None,
                   stable=True, return_keys=False):
    """``ray_order`` of rays ``first .. first + n`` of a source program (tfrt_source3d_order): the
    rays are never written in source order.  ``stable=False``: the same order up to ties, most
    significant digit first (tfrt_source3d_order_cells) -- fewer launches; rays with the same key may
    land in an order that varies from run to run.  ``return_keys``: also the uint32 keys the
    program's float32 evaluation made (natural order, as int32 bits)."""
    n = int(n)
    dev = device if device is not None else (out.device if out is not None else face_verts.device)
    perm = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    if perm.dtype != torch.int32 or perm.numel() != n or not perm.is_contiguous():
        raise TfrtError("source3d_order: `out` must be a contiguous int32 tensor of n entries")
    _need_gpu(perm, face_verts)
    keys = torch.empty(n, dtype=torch.int32, device=perm.device) if return_keys else None
    if n:
        L = _lib.lib()
        fv = None if face_verts is None else _c(face_verts.detach(), torch.float64)
        wsb = L.tfrt_ray_order_workspace_bytes(n)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        ax = None if axis is None else (ctypes.c_double * 3)(*[float(v) for v in axis])
        fn = L.tfrt_source3d_order if stable else L.tfrt_source3d_order_cells
        check(fn(ctypes.byref(program), int(first), n, _p(fv), 0 if fv is None else fv.shape[0], ax,
                 _p(perm), _p(keys), _p(ws), wsb, _stream(perm)), "tfrt_source3d_order")
    return (perm, keys) if return_keys else perm


def epoch_advance(counters):
    """``c[0] += 1`` for up to 8 distinct int64 device counters in one launch (tfrt_epoch_advance):
    the distributions of a source step to their next draw."""
    counters = [c for c in counters if c is not None]
    if not counters:
        return
    _need_gpu(*counters)
    for at in range(0, len(counters), 8):
        part = counters[at:at + 8]
        arr = (ctypes.c_void_p * len(part))(*[c.data_ptr() for c in part])
        check(_lib.lib().tfrt_epoch_advance(arr, len(part), _stream(part[0])), "tfrt_epoch_advance")


def points_generate(program, n, first=0, index=None, columns=3, want_points=True, want_aux=False,
                    device=None):
    """Samples of one distribution (a ``_lib.PointsProgram``) at its current epoch
    (tfrt_points_generate): (points (n, columns) f64 or None, aux0, aux1 (n,) f64 or None)."""
    dev = device if device is not None else (index.device if index is not None else None)
    n = int(n)
    pts = torch.empty((n, columns), dtype=torch.float64, device=dev) if want_points else None
    a0 = torch.empty(n, dtype=torch.float64, device=dev) if want_aux else None
    a1 = torch.empty(n, dtype=torch.float64, device=dev) if want_aux else None
    ref = pts if pts is not None else a0
    if n and ref is not None:
        _need_gpu(ref)
        check(_lib.lib().tfrt_points_generate(ctypes.byref(program), _p(index), int(first), n,
                                              _p(pts), int(columns), _p(a0), _p(a1), _stream(ref)),
              "tfrt_points_generate")
    return pts, a0, a1


def source3d_generate(program, n, dtype=None, first=0, index=None, rays_out=None, fields=False,
                      device=None):
    """Rays of a source program (``_lib.Source3DProgram``) at the current epochs of its
    distributions (tfrt_source3d_generate): (ray block (6, n) of ``dtype`` or None, fields (6, n)
    f64 or None); ``index``: the rays ``first + index[j]`` instead of ``first + j``."""
    n = int(n)
    dev = device if device is not None else (index.device if index is not None else
                                             (rays_out.device if rays_out is not None else None))
    rays = rays_out
    if rays is None and dtype is not None:
        rays = torch.empty((6, n), dtype=dtype, device=dev)
    fl = torch.empty((6, n), dtype=torch.float64, device=dev) if fields else None
    ref = rays if rays is not None else fl
    if n and ref is not None:
        _need_gpu(ref)
        dt = _DT[rays.dtype] if rays is not None else _lib.F64
        check(_lib.lib().tfrt_source3d_generate(
            ctypes.byref(program), _p(index), int(first), n, dt, _p(rays),
            rays.stride(0) if rays is not None else 0, _p(fl), n if fl is not None else 0,
            _stream(ref)), "tfrt_source3d_generate")
    return rays, fl


def samples_generate(program, n, first=0, index=None, want_values=True, want_ranks=False,
                     device=None):
    """Samples of one 1-D distribution (a ``_lib.SamplesProgram``) at its current epoch
    (tfrt_samples_generate): (values -- angles (n,) or points (n, 2) f64 -- or None, ranks (n,) f64
    or None); ``index``: the samples ``first + index[j]`` instead of ``first + j``."""
    dev = device if device is not None else (index.device if index is not None else None)
    n = int(n)
    cols = 1 if program.kind in (_lib.SMP_UNIFORM_ANGLE, _lib.SMP_LAMBERT_ANGLE) else \
        (int(program.columns) if program.kind == _lib.SMP_TABLE else 2)
    shape = (n,) if cols == 1 else (n, 2)
    vals = torch.empty(shape, dtype=torch.float64, device=dev) if want_values else None
    ranks = torch.empty(n, dtype=torch.float64, device=dev) if want_ranks else None
    ref = vals if vals is not None else ranks
    if n and ref is not None:
        _need_gpu(ref, index)
        check(_lib.lib().tfrt_samples_generate(ctypes.byref(program), _p(index), int(first), n,
                                               _p(vals), cols, _p(ranks), _stream(ref)),
              "tfrt_samples_generate")
    return vals, ranks


def source2d_generate(program, n, dtype=None, first=0, index=None, rays_out=None, fields=False,
                      device=None):
    """Rays of a 2-D source program (``_lib.Source2DProgram``) at the current epochs of its
    distributions (tfrt_source2d_generate): (ray block (4, n) of ``dtype`` or None, fields (4, n)
    f64 or None); ``index``: the rays ``first + index[j]`` instead of ``first + j``."""
    n = int(n)
    dev = device if device is not None else (index.device if index is not None else
                                             (rays_out.device if rays_out is not None else None))
    rays = rays_out
    if rays is None and dtype is not None:
        rays = torch.empty((4, n), dtype=dtype, device=dev)
    fl = torch.empty((4, n), dtype=torch.float64, device=dev) if fields else None
    ref = rays if rays is not None else fl
    if n and ref is not None:
        _need_gpu(ref, index)
        dt = _DT[rays.dtype] if rays is not None else _lib.F64
        check(_lib.lib().tfrt_source2d_generate(
            ctypes.byref(program), _p(index), int(first), n, dt, _p(rays),
            rays.stride(0) if rays is not None else 0, _p(fl), n if fl is not None else 0,
            _stream(ref)), "tfrt_source2d_generate")
    return rays, fl


def source3d_pool_rows(program, n, first=0, index=None, out=None, device=None):
    """The pool rows the rays ``first + index[j]`` (``first + j``) of a TFRT_SRC_POOL program are made
    from at its current epoch (tfrt_source3d_pool_rows): (n,) int32 -- what every stored field that
    is not geometry is gathered through."""
    return _pool_rows("tfrt_source3d_pool_rows", program, n, first, index, out, device)


def source2d_pool_rows(program, n, first=0, index=None, out=None, device=None):
    """``source3d_pool_rows`` for a 2-D pool program (a ``_lib.Source2DProgram`` of kind
    TFRT_SRC_POOL; tfrt_source2d_pool_rows)."""
    return _pool_rows("tfrt_source2d_pool_rows", program, n, first, index, out, device)


def _pool_rows(entry, program, n, first, index, out, device):
    n = int(n)
    dev = device if device is not None else (index.device if index is not None else
                                             (out.device if out is not None else None))
    rows = out if out is not None else torch.empty(n, dtype=torch.int32, device=dev)
    if rows.dtype != torch.int32 or rows.numel() != n or not rows.is_contiguous():
        raise TfrtError(f"{entry[5:]}: `out` must be a contiguous int32 tensor of n entries")
    if index is not None and (index.dtype != torch.int32 or index.numel() != n
                              or not index.is_contiguous()):
        raise TfrtError(f"{entry[5:]}: `index` must be a contiguous int32 tensor of n entries")
    if n:
        _need_gpu(rows, index)
        check(getattr(_lib.lib(), entry)(ctypes.byref(program), _p(index), int(first), n, _p(rows),
                                         _stream(rows)), entry)
    return rows


def morton_order(face_verts):
    """Permutation of the faces by the Morton code of their centroids (30-bit, 10 bits per
    axis): spatially close faces become neighbours.  Pass it as ``cluster_order``."""
    fv = face_verts.detach()
    c = (fv[:, 0:3] + fv[:, 3:6] + fv[:, 6:9]) / 3.0
    lo, hi = c.min(dim=0).values, c.max(dim=0).values
    q = ((c - lo) / torch.clamp(hi - lo, min=1e-300) * 1023.0).clamp(0, 1023).to(torch.int64)

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v

    key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return torch.argsort(key, stable=True).to(torch.int32)


def cluster_order(face_verts, leaf=16, group=128):
    """Permutation of the faces that makes every aligned run of ``leaf`` consecutive entries
    (and of ``group`` entries: the kernels' clusters and superclusters) a compact patch:
    recursive median split of the face centroids along the longest axis of their bounding box,
    the left part a multiple of ``group`` (of ``leaf`` below that), down to parts of <= ``leaf``
    faces; outsized faces (a target plane behind a fine lens mesh, ...) go last.  Pass it as
    ``cluster_order``.  Unlike a Morton order there are no space-filling-curve jumps inside a run,
    so the clusters' bounding spheres stay small (measured on the cfg4 lens: 10 cluster hits per
    ray instead of 17).  On the device (tfrt_cluster_order: a radix sort per tree level, no host
    sync), once per mesh topology."""
    _need_gpu(face_verts)
    fv = _c(face_verts.detach(), torch.float64)
    M = fv.shape[0]
    order = torch.empty(M, dtype=torch.int32, device=fv.device)
    if M:
        L = _lib.lib()
        wsb = L.tfrt_cluster_order_workspace_bytes(M, int(leaf), int(group))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=fv.device)
        check(L.tfrt_cluster_order(_p(fv), M, int(leaf), int(group), _p(order), _p(ws), wsb,
                                   _stream(fv)), "tfrt_cluster_order")
    return order


def snell3d(x_start, y_start, z_start, x_end, y_end, z_end, norm, n_in, n_out, new_ray_length):
    """geometry.snells_law_3D (geometry.py:671-753) -> (6,n) f64 block of the new rays."""
    args = [_c(a, torch.float64) for a in (x_start, y_start, z_start, x_end, y_end, z_end, norm)]
    _need_gpu(*args)
    n = args[0].shape[0]
    n_in = _c(torch.as_tensor(n_in, dtype=torch.float64, device=args[0].device).expand(n), torch.float64)
    n_out = _c(torch.as_tensor(n_out, dtype=torch.float64, device=args[0].device).expand(n), torch.float64)
    out = torch.empty((6, n), dtype=torch.float64, device=args[0].device)
    check(_lib.lib().tfrt_snell3d(n, *[_p(a) for a in args], _p(n_in), _p(n_out),
                                  float(new_ray_length), _p(out), _stream(out)), "tfrt_snell3d")
    return out


def snell2d(x_start, y_start, x_end, y_end, norm, n_in, n_out, new_ray_length):
    """geometry.snells_law_2D (geometry.py:565-653) -> (4,n) f64 block of the new rays."""
    args = [_c(a, torch.float64) for a in (x_start, y_start, x_end, y_end, norm)]
    _need_gpu(*args)
    n = args[0].shape[0]
    n_in = _c(torch.as_tensor(n_in, dtype=torch.float64, device=args[0].device).expand(n), torch.float64)
    n_out = _c(torch.as_tensor(n_out, dtype=torch.float64, device=args[0].device).expand(n), torch.float64)
    out = torch.empty((4, n), dtype=torch.float64, device=args[0].device)
    check(_lib.lib().tfrt_snell2d(n, *[_p(a) for a in args], _p(n_in), _p(n_out),
                                  float(new_ray_length), _p(out), _stream(out)), "tfrt_snell2d")
    return out


# ================================================================================= 2-D

from ._lib import Scene2D  # noqa: E402


class Scene2DArgs:
    """Device tensors describing the merged 2-D boundary sets (tfrt_scene2d).  ``segments`` /
    ``arcs`` are the dicts built by ``OpticalSystem2D._merge_kind`` (``geo`` (M,4|5) f64,
    ``cat`` int32, optional ``mat_in/mat_out/n_in/n_out``) or None."""

    def __init__(self, segments, arcs, n_table, index_mode, ghost, intersect_epsilion=1e-10,
                 size_epsilion=1e-10, ray_start_epsilion=1e-10, finite_tir_gradient=False,
                 deterministic=False):
        self.segments, self.arcs = segments, arcs
        self.finite_tir_gradient = bool(finite_tir_gradient)
        self.deterministic = bool(deterministic)           # ordered reverse-sweep sums
        self.n_table = _c(n_table, torch.float64)
        self.index_mode, self.ghost = index_mode, ghost
        self.eps = (float(intersect_epsilion), float(size_epsilion), float(ray_start_epsilion))
        self._keep = []

    def struct(self, seg_geo, arc_geo):
        sc = Scene2D()
        self._keep = []

        def fill(prefix, info, geo, count_field):
            n = 0 if geo is None else geo.shape[0]
            setattr(sc, count_field, n)
            names = {"seg": ("seg", "seg_cat", "seg_mat_in", "seg_mat_out", "seg_n_in", "seg_n_out"),
                     "arc": ("arc", "arc_cat", "arc_mat_in", "arc_mat_out", "arc_n_in", "arc_n_out")}[prefix]
            for nm in names:
                setattr(sc, nm, None)
            if n == 0:
                return
            setattr(sc, names[0], geo.data_ptr())
            setattr(sc, names[1], info["cat"].data_ptr())
            if self.ghost:
                ones = torch.ones(n, dtype=torch.float64, device=geo.device)
                self._keep.append(ones)
                setattr(sc, names[4], ones.data_ptr())
                setattr(sc, names[5], ones.data_ptr())
            elif self.index_mode:
                if info["mat_in"] is None or info["mat_out"] is None:
                    raise TfrtError("StandardReaction('index') needs mat_in / mat_out on every "
                                    "optical boundary")
                setattr(sc, names[2], info["mat_in"].data_ptr())
                setattr(sc, names[3], info["mat_out"].data_ptr())
            else:
                if info["n_in"] is None or info["n_out"] is None:
                    raise TfrtError("StandardReaction('value') needs n_in / n_out on every optical "
                                    "boundary")
                setattr(sc, names[4], info["n_in"].data_ptr())
                setattr(sc, names[5], info["n_out"].data_ptr())

        fill("seg", self.segments, seg_geo, "n_segments")
        fill("arc", self.arcs, arc_geo, "n_arcs")
        sc.grad_seg_n_in = sc.grad_seg_n_out = sc.grad_arc_n_in = sc.grad_arc_n_out = None
        if self.n_table is not None and self.n_table.numel() and self.index_mode and not self.ghost:
            sc.n_table = self.n_table.data_ptr()
            sc.n_table_stride = self.n_table.shape[1]
            sc.n_materials = self.n_table.shape[0]
        else:
            sc.n_table, sc.n_table_stride, sc.n_materials = None, 0, 0
        sc.intersect_epsilion, sc.size_epsilion, sc.ray_start_epsilion = self.eps
        sc.finite_tir_gradient = 1 if self.finite_tir_gradient else 0
        sc.deterministic = 1 if self.deterministic else 0
        return sc

    def index_args(self):
        """"value" mode: the per-primitive indices as handed in (seg_n_in, seg_n_out, arc_n_in,
        arc_n_out; they may require grad: d error / d index), None where absent or not read."""
        if self.ghost or self.index_mode:
            return (None,) * 4
        return tuple(None if info is None else info.get(f) for info in (self.segments, self.arcs)
                     for f in ("n_in", "n_out"))


_GRAD_INDEX_2D = ("grad_seg_n_in", "grad_seg_n_out", "grad_arc_n_in", "grad_arc_n_out")


class _Trace2D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, seg_geo, arc_geo, seg_n_in, seg_n_out, arc_n_in, arc_n_out, scene, opts):
        # (the index tensors: the per-primitive indices of "value" mode when they require grad --
        # the values are read through `scene`; listing them here gives their gradients a place to go)
        _need_gpu(src, seg_geo, arc_geo)
        dev = src.device
        if src.dtype not in _DT:
            raise TfrtError(f"ray state dtype must be float32, float64 or float16, got {src.dtype}")
        src = src.contiguous()
        seg_geo = _c(seg_geo, torch.float64)
        arc_geo = _c(arc_geo, torch.float64)
        N = src.shape[1]
        P = int(opts["max_passes"])
        flags = int(opts["flags"])
        dt = _DT[src.dtype]
        L = _lib.lib()
        Ms = 0 if seg_geo is None else seg_geo.shape[0]
        Ma = 0 if arc_geo is None else arc_geo.shape[0]
        wsb = L.tfrt_trace2d_workspace_bytes(N, Ms, Ma, P, dt)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        capN = max(N, 1)
        ints = _IntPool(dev, bool(opts.get("zero_init")), _lib.COUNTS_PER_PASS * (P + 1), flags,
                        capN, P)
        counts = ints.counts

        def alloc(flag, cap):
            if not (flags & flag):
                return None, None, None
            return (torch.empty((4, cap), dtype=src.dtype, device=dev),  # (see _Trace3D.forward)
                    ints.take(cap), ints.take(cap))

        fin = alloc(_lib.COMPILE_FINISHED, capN)
        act = alloc(_lib.COMPILE_ACTIVE, capN * max(P, 1))
        stp = alloc(_lib.COMPILE_STOPPED, capN)
        dead = alloc(_lib.COMPILE_DEAD, capN)
        unf = torch.empty((4, capN), dtype=src.dtype, device=dev)
        unf_id = ints.take(capN)
        sc = scene.struct(seg_geo, arc_geo)
        outs = [_ray_out(*o) for o in (fin, act, stp, dead)]
        check(L.tfrt_trace2d_forward(
            _p(src), src.shape[1], N, ctypes.byref(sc), float(opts["new_ray_length"]),
            float(opts["dead_ray_length"] or 0.0), P, dt, flags,
            ctypes.byref(outs[0]), ctypes.byref(outs[1]), ctypes.byref(outs[2]),
            ctypes.byref(outs[3]), _p(unf), _p(unf_id), _p(counts), _p(ws), wsb, _stream(src)),
            "tfrt_trace2d_forward")
        tape = TraceTape()
        tape.src, tape.seg, tape.arc, tape.scene, tape.opts = src, seg_geo, arc_geo, scene, dict(opts)
        tape.ws, tape.wsb, tape.counts, tape.dt = ws, wsb, counts, dt
        tape.caps = [o[0].shape[1] if o[0] is not None else 0 for o in (fin, act, stp, dead)]
        ctx.tape = tape
        opts["_aux"] = {
            "counts": counts, "unfinished": unf, "unfinished_id": unf_id,
            "finished_id": fin[1], "finished_face": fin[2], "active_id": act[1],
            "active_face": act[2], "stopped_id": stp[1], "stopped_face": stp[2],
            "dead_id": dead[1], "dead_face": dead[2],
        }
        empty = torch.empty((4, 0), dtype=src.dtype, device=dev)
        ctx.present = [o[0] is not None for o in (fin, act, stp, dead)]
        ctx.set_materialize_grads(False)
        return _with_rows([o[0] if o[0] is not None else empty for o in (fin, act, stp, dead)],
                          ctx.present)

    @staticmethod
    def backward(ctx, *grads):
        t = ctx.tape
        dev = t.src.device
        g_seg = None if t.seg is None else torch.zeros_like(t.seg)
        g_arc = None if t.arc is None else torch.zeros_like(t.arc)
        need_src = ctx.needs_input_grad[0]
        g_src = torch.zeros((4, t.src.shape[1]), dtype=torch.float64, device=dev) if need_src else None
        gs = _class_grads(ctx.present, t.caps, 4, dev, grads)
        sc = t.scene.struct(t.seg, t.arc)
        sizes = [0 if g is None else g.shape[0] for g in (t.seg, t.seg, t.arc, t.arc)]
        g_n = [torch.zeros(m, dtype=torch.float64, device=dev) if ctx.needs_input_grad[3 + k] and m
               else None for k, m in enumerate(sizes)]
        for name, g in zip(_GRAD_INDEX_2D, g_n):
            setattr(sc, name, None if g is None else g.data_ptr())
        try:
            check(_lib.lib().tfrt_trace2d_backward(
                _p(t.src), t.src.shape[1], t.src.shape[1], ctypes.byref(sc),
                float(t.opts["new_ray_length"]), float(t.opts["dead_ray_length"] or 0.0),
                int(t.opts["max_passes"]), t.dt,
                _p(gs[0]), t.caps[0], _p(gs[1]), t.caps[1], _p(gs[2]), t.caps[2], _p(gs[3]),
                t.caps[3], _p(g_seg), _p(g_arc), _p(g_src), _p(t.counts), _p(t.ws), t.wsb,
                _stream(t.src)), "tfrt_trace2d_backward")
        finally:
            for name in _GRAD_INDEX_2D:
                setattr(sc, name, None)
        if g_src is not None:
            g_src = g_src.to(t.src.dtype)
        return (g_src, g_seg, g_arc, *g_n, None, None)


def trace2d(src, scene, max_passes, new_ray_length=1.0, dead_ray_length=None,
            flags=_lib.COMPILE_ACTIVE | _lib.COMPILE_FINISHED, predicted_counts=None):
    """Whole 2-D trace; same result dict as ``trace3d`` with (4, n) ray blocks.  The ``*_face``
    arrays index the merged segments first and then ``n_segments + merged arc index``."""
    opts = dict(max_passes=max_passes, new_ray_length=new_ray_length,
                dead_ray_length=dead_ray_length, flags=flags,
                zero_init=predicted_counts is not None)
    seg_geo = None if scene.segments is None else scene.segments["geo"]
    arc_geo = None if scene.arcs is None else scene.arcs["geo"]
    index = [n if isinstance(n, torch.Tensor) and n.requires_grad else None
             for n in scene.index_args()]
    outs = _Trace2D.apply(src, seg_geo, arc_geo, *index, scene, opts)
    aux = opts.pop("_aux")
    blocks, rows = _split_rows(outs, [aux[name + "_id"] is not None for name in _CLASS_NAMES], 4)
    full = dict(zip(_CLASS_NAMES, blocks))
    for name, r in rows.items():
        aux[name + "_rows"] = r
    out = _finish_trace(full, aux, int(max_passes), predicted_counts)
    out["n_segments"] = 0 if seg_geo is None else seg_geo.shape[0]
    return out


def _seam2d(fn_name, rays, prim, eps):
    _need_gpu(rays, prim)
    rays = rays.contiguous()
    prim = _c(prim, torch.float64)
    N, M = rays.shape[1], prim.shape[0]
    dev = rays.device
    f = lambda: torch.empty(N, dtype=torch.float64, device=dev)
    x, y, ray_u, prim_u = f(), f(), f(), f()
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    gather = torch.empty(N, dtype=torch.int32, device=dev)
    check(getattr(_lib.lib(), fn_name)(
        _p(rays), rays.shape[1], N, _DT[rays.dtype], _p(prim) if M else None, M,
        float(eps[0]), float(eps[1]), float(eps[2]), _p(x), _p(y), _p(valid), _p(ray_u),
        _p(prim_u), _p(gather), _stream(rays)), fn_name)
    return x, y, valid.bool(), ray_u, prim_u, gather


def segment_intersection(rays, seg, intersect_epsilion=1e-10, size_epsilion=1e-10,
                         ray_start_epsilion=1e-10):
    """OpticalSystem2D._segment_intersection (engine.py:688-749); rays (4,N), seg (M,4)."""
    return _seam2d("tfrt_segment_intersection", rays, seg,
                   (intersect_epsilion, size_epsilion, ray_start_epsilion))


def arc_intersection(rays, arc, intersect_epsilion=1e-10, size_epsilion=1e-10,
                     ray_start_epsilion=1e-10):
    """OpticalSystem2D._arc_intersection (engine.py:768-866); rays (4,N), arc (M,5)."""
    return _seam2d("tfrt_arc_intersection", rays, arc,
                   (intersect_epsilion, size_epsilion, ray_start_epsilion))


def gather_optical_2d(system, out):
    """Boundary data of the reacting rays of a 2-D pass, in the order of ``out['active']``
    (segment-hit rays then arc-hit rays), correctly paired (the reference's mixed-system
    concat pairs them wrongly, engine.py:1958-1965)."""
    face = out["active_face"].long()
    ns = out["n_segments"]
    result = {}
    seg_set = system._amalgamated_optical_segments
    arc_set = system._amalgamated_optical_arcs
    is_arc = face >= ns
    geo = {"x_start", "y_start", "x_end", "y_end", "x_center", "y_center", "angle_start",
           "angle_end", "radius"}
    keys = None
    for s in (seg_set, arc_set):
        if bool(s):
            k = set(s.keys()) - geo
            keys = k if keys is None else (keys & k)
    for f in (keys or ()):
        parts = []
        if bool(seg_set):
            parts.append(seg_set[f][face[~is_arc]])
        if bool(arc_set):
            parts.append(arc_set[f][face[is_arc] - ns])
        result[f] = torch.cat(parts) if len(parts) > 1 else parts[0]
    return result
