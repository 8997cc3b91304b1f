"""
``host_libm()``: a context in which ``torch.sin``, ``torch.cos``, ``torch.asin`` and
``torch.atan2`` of float64 CPU tensors are the C library's functions, evaluated element by
element, with the derivatives torch itself uses.

The bit-for-bit comparisons of the oracle with the reference's own source
(tests/test_reference_golden.py; fixtures by tests/golden/make_reference_golden.py and
make_reference_trace2d_golden.py) need the same elementary functions on both sides.  torch's own
float64 kernels for sin / cos / asin call MKL's vector math library, whose last bit depends on
the CPU model and vendor (0.1-0.5 % of the results differ by one ulp between an Intel and an AMD
host), and atan2 takes a vector or a scalar path depending on the CPU's instruction set; the C
library's functions do neither.  Both the fixtures and the checks are therefore computed inside
this context.  Any other call goes to torch unchanged.
"""
import contextlib
import math

import numpy as np
import torch

_TORCH = {name: getattr(torch, name) for name in ("sin", "cos", "asin", "atan2")}


def _libm(fn, *xs):
    out = np.frompyfunc(fn, len(xs), 1)(*[x.detach().numpy() for x in xs])
    return torch.from_numpy(np.array(out, dtype=np.float64))


class _Sin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _libm(math.sin, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * _Cos.apply(x)


class _Cos(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _libm(math.cos, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * -_Sin.apply(x)


def _asin(v):
    return math.asin(v) if -1.0 <= v <= 1.0 else math.nan     # (torch: NaN outside [-1, 1])


class _Asin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return _libm(_asin, x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * (-x * x + 1).rsqrt()


class _Atan2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, x):
        ctx.save_for_backward(y, x)
        return _libm(math.atan2, y, x)

    @staticmethod
    def backward(ctx, g):
        y, x = ctx.saved_tensors
        recip = (y * y + x * x).reciprocal()
        return g * x * recip, g * -y * recip


def _host_f64(*xs):
    return all(isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.device.type == "cpu"
               for x in xs)


def _wrap(name, fn):
    def call(*args, **kwargs):
        if kwargs or not _host_f64(*args):
            return _TORCH[name](*args, **kwargs)
        return fn.apply(*torch.broadcast_tensors(*args))
    return call


@contextlib.contextmanager
def host_libm():
    patched = {"sin": _wrap("sin", _Sin), "cos": _wrap("cos", _Cos), "asin": _wrap("asin", _Asin),
               "atan2": _wrap("atan2", _Atan2)}
    for name, fn in patched.items():
        setattr(torch, name, fn)
    try:
        yield
    finally:
        for name, fn in _TORCH.items():
            setattr(torch, name, fn)
