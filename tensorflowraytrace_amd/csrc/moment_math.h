// The per-group arithmetic of MomentError (tfrt_moment.hip; the definition, operation by operation,
// is in include/tfrt_hip.h at tfrt_moment_error): the integer centre of a group's first record, the
// exact second moment about that centre reassembled from its three int64 limb sums, the covariance
// in scene units, the residual D against a target covariance or against "round", and the group's
// error.  Float64 and int64 only, every operation rounded on its own.  Compiles for the host as
// well (the convention of centroid_math.h), so that tests/moment_host checks it without a GPU.
//
// One field: the xy and yy components of every covariance and residual are 0.0, cy is 0.0.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

constexpr int MOMENT_SLOTS = 9;        // {xx, xy, yy} x {HH, HL, LL}
constexpr int MOMENT_ROW = 8;          // {cx, cy, 4Dxx, 4Dxy, 4Dyy, used, 0, 0}: one 64-byte line
constexpr int MOMENT_COV = 6;          // {Cxx, Cxy, Cyy, Dxx, Dxy, Dyy}
constexpr int MOMENT_USED_OUT = 2;     // {groups used, groups with rays}
constexpr int MOMENT_TARGET = 0, MOMENT_ROUND = 1;   // the modes

// The grid of the records: msx = 2^mbits / (x1 - x0), h = mbits / 2; `two`: a second field.
struct MomentGrid {
  double x0, msx, y0, msy;
  int32_t mbits, h;
  bool two;
};

// The integer centre of a group with n >= 1 rays from its coordinate sum S >= 0: the grid point
// nearest to S / n, halves up.  2 S + n < 2^63 because S <= n 2^mbits < 2^61.
TFRT_HD int64_t moment_centre(int64_t n, int64_t S) { return (2 * S + n) / (2 * n); }

// The low limb of d (h bits, 0 .. 2^h - 1) and the high one (an arithmetic shift: floor(d / 2^h)).
TFRT_HD int64_t moment_low(int64_t d, int h) { return d & (((int64_t)1 << h) - 1); }
TFRT_HD int64_t moment_high(int64_t d, int h) { return d >> h; }

// sum(da * db) = HH 2^mbits + HL 2^h + LL as a double, added in this order.
TFRT_HD double moment_value(const int64_t* limbs, const MomentGrid& g) {
#pragma clang fp contract(off)
  return (std::ldexp((double)limbs[0], g.mbits) + std::ldexp((double)limbs[1], g.h)) +
         (double)limbs[2];
}

// What the table launch knows of a group.  Without rays: c = NaN; not used (n < 2): C = D = NaN,
// F = 0.0, e = 0.0.  F = 4 D is what a ray's gradient is made from.
struct MomentGroup {
  bool rays, used;
  double n, cx, cy;
  double C[3], D[3], F[3];
  double e;
};

// `rec`: {n, Sx, Sy}; `mom`: the nine limb sums; `target`: {txx, txy, tyy} of the group (k == 1:
// {txx}), read in MOMENT_TARGET mode only -- a NaN component is free.
TFRT_HD MomentGroup moment_group(const int64_t* rec, const int64_t* mom, const MomentGrid& g,
                                 int mode, const double* target) {
#pragma clang fp contract(off)
  MomentGroup q;
  const double nan = __builtin_nan("");
  q.rays = rec[0] > 0;
  q.used = rec[0] >= 2;
  q.n = (double)rec[0];
  q.cx = q.cy = nan;
  q.e = 0.0;
  for (int c = 0; c < 3; ++c) q.C[c] = q.D[c] = nan, q.F[c] = 0.0;
  if (!q.rays) return q;
  q.cx = g.x0 + (double)moment_centre(rec[0], rec[1]) / g.msx;
  q.cy = g.two ? g.y0 + (double)moment_centre(rec[0], rec[2]) / g.msy : 0.0;
  if (!q.used) return q;
  q.C[0] = (moment_value(mom + 0, g) / q.n) / (g.msx * g.msx);
  q.C[1] = g.two ? (moment_value(mom + 3, g) / q.n) / (g.msx * g.msy) : 0.0;
  q.C[2] = g.two ? (moment_value(mom + 6, g) / q.n) / (g.msy * g.msy) : 0.0;
  if (mode == MOMENT_ROUND) {
    const double s = (q.C[0] + q.C[2]) / 2.0;
    q.D[0] = q.C[0] - s;
    q.D[1] = q.C[1];
    q.D[2] = q.C[2] - s;
  } else {
    const double t[3] = {target[0], g.two ? target[1] : nan, g.two ? target[2] : nan};
    for (int c = 0; c < 3; ++c) q.D[c] = std::isnan(t[c]) ? 0.0 : q.C[c] - t[c];
  }
  for (int c = 0; c < 3; ++c) q.F[c] = 4.0 * q.D[c];
  q.e = q.n * ((q.D[0] * q.D[0] + 2.0 * (q.D[1] * q.D[1])) + q.D[2] * q.D[2]);
  return q;
}

}  // namespace tfrt
