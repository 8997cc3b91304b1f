// Field codes of the coupled errors (DensityError, SpotError) on a d-D ray block -- rows 0..d-1 the
// start of a finished ray's last link, rows d..2d-1 its end:
//
//   code c < 2d          block row c
//   2d <= c < 3d         the direction cosine d_(c - 2d) of the last link
//
// The definition (include/tfrt_hip.h at tfrt_density_error_fields), every operation an IEEE f64
// operation rounded on its own:
//
//   e_a = (double) end_a - (double) start_a,  q = e_x*e_x + e_y*e_y [+ e_z*e_z] left to right,
//   L = sqrt(q),  d_a = e_a / L
//
// A column with a non-finite geometry row, or with L not finite or not > 0, has no direction: its
// fields read as NaN, which the callers' "a coordinate is non-finite" case takes.
//
// The chain rule of the seed kernels, from gv_k = d error / d (field k):
//
//   t   = sum over the direction fields k, in field order, of gv_k * d_(a_k)
//   G_b = ((gv_k of the direction field of axis b, else 0.0) - t * d_b) / L
//   grad[end_b] = G_b, grad[start_b] = -G_b, then + gv_k of a position field that names the row.
//
// With float32 rows the subtraction cancels: a direction is good to about
// eps32 * max|coordinate| / L.
#pragma once
#include "tfrt_common.h"

namespace tfrt {

// The last link of one column of a DIM-D block.  ok: every geometry row finite, L finite and > 0.
template <int DIM>
struct LinkDir {
  double s[DIM], e[DIM];   // start and end rows as read (f64)
  double d[DIM];           // direction cosines
  double L;
  bool ok;
};
// (no direction field: nothing is kept)
template <>
struct LinkDir<0> {};

template <typename T, int DIM>
__device__ __forceinline__ LinkDir<DIM> link_direction(const T* __restrict__ rows, int64_t stride,
                                                       int64_t i) {
#pragma clang fp contract(off)
  LinkDir<DIM> k;
  bool finite = true;
  double v[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    k.s[a] = ldd(rows, (int64_t)a * stride + i);
    k.e[a] = ldd(rows, (int64_t)(DIM + a) * stride + i);
    finite = finite && isfinite(k.s[a]) && isfinite(k.e[a]);
    v[a] = k.e[a] - k.s[a];
  }
  double q = v[0] * v[0] + v[1] * v[1];
  if (DIM == 3) q = q + v[DIM - 1] * v[DIM - 1];
  k.L = sqrt(q);
  k.ok = finite && isfinite(k.L) && k.L > 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) k.d[a] = v[a] / k.L;
  return k;
}

// The value of field `code` (0 <= code < 3 * DIM) of a column whose link is `k` (NaN without a
// direction).
template <int DIM>
__device__ __forceinline__ double link_field(const LinkDir<DIM>& k, int code) {
  if (!k.ok) return __builtin_nan("");
  double v = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    if (code == a) v = k.s[a];
    if (code == DIM + a) v = k.e[a];
    if (code == 2 * DIM + a) v = k.d[a];
  }
  return v;
}

// The fields x and y (y = 0.0 with fy < 0) of column i.  DIM = 0, no direction field: the two
// block rows, as the position-only kernels always read them.  DIM = 2, 3: the whole link of a
// DIM-D block, returned in `k`.
template <typename T, int DIM>
__device__ __forceinline__ void read_fields(const T* __restrict__ rows, int64_t stride, int64_t i,
                                            int fx, int fy, double& x, double& y,
                                            LinkDir<DIM>& k) {
  if constexpr (DIM != 0) {
    k = link_direction<T, DIM>(rows, stride, i);
    x = link_field<DIM>(k, fx);
    y = fy >= 0 ? link_field<DIM>(k, fy) : 0.0;
  } else {
    x = ldd(rows, (int64_t)fx * stride + i);
    y = fy >= 0 ? ldd(rows, (int64_t)fy * stride + i) : 0.0;
  }
}

// All 2 * DIM gradient rows of column i from gx = d error / d x, gy = d error / d y.  `counts`
// false (`k` may then be unset: a masked column is never read): zeros.
template <int DIM>
__device__ __forceinline__ void chain_fields(const LinkDir<DIM>& k, bool counts, int fx, int fy,
                                             double gx, double gy, double* __restrict__ grad,
                                             int64_t grad_stride, int64_t i) {
#pragma clang fp contract(off)
  double start[DIM], end[DIM];
#pragma unroll
  for (int b = 0; b < DIM; ++b) start[b] = end[b] = 0.0;
  if (counts) {
    const bool two = fy >= 0;
    const int ax = fx - 2 * DIM, ay = two ? fy - 2 * DIM : -1;   // direction axes (< 0: a position)
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      if (ax == a) t = gx * k.d[a], first = false;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      if (ay == a) t = first ? gy * k.d[a] : t + gy * k.d[a];
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      const double gvb = ax == b ? gx : (ay == b ? gy : 0.0);
      const double G = (gvb - t * k.d[b]) / k.L;
      end[b] = G;
      start[b] = -G;
      if (fx == b) start[b] = start[b] + gx;
      if (two && fy == b) start[b] = start[b] + gy;
      if (fx == DIM + b) end[b] = end[b] + gx;
      if (two && fy == DIM + b) end[b] = end[b] + gy;
    }
  }
#pragma unroll
  for (int b = 0; b < DIM; ++b) {
    grad[(int64_t)b * grad_stride + i] = start[b];
    grad[(int64_t)(DIM + b) * grad_stride + i] = end[b];
  }
}

}  // namespace tfrt
