// The per-group arithmetic of DistortionError (tfrt_distortion.hip; the definition, operation by
// operation, is in include/tfrt_hip.h at tfrt_distortion_error): a group's weight, centroid and
// object point from its record, the terms it adds to the sums of the two fit passes, the fit
// (A, t) from those sums, and a group's residual against the fitted image of its object point.
// Float64 and int64 only, every operation rounded on its own.  Compiles for the host as well (the
// convention of focus_math.h), so that tests/distortion_host checks it without a GPU.
//
// One field: the y components of every point and centroid are 0.0 and the same expressions run.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

constexpr int DISTORTION_FIT_SCALE = 0;
constexpr int DISTORTION_FIT_AFFINE = 1;
constexpr int DISTORTION_FIT_OUT = 8;    // {A00, A01, A10, A11, t0, t1, valid, groups_used}
constexpr int DISTORTION_MEAN_SUMS = 5;  // {W, sum w px, sum w py, sum w cx, sum w cy}
constexpr int DISTORTION_MOMENT_SUMS = 7;   // {Sxx, Sxy, Syy, Cxx, Cxy, Cyx, Cyy}

// The domain constants of the records (tfrt_spot_error's), `two`: a second field.
struct DistortionGrid {
  double x0, qsx, y0, qsy;
  bool two;
};

// A group: USED if its record has rays; then its weight w = (double) count, its centroid c (as
// tfrt_spot_error computes it) and its object point p.
struct DistortionGroup {
  bool used;
  double w, px, py, cx, cy;
};

// rec: the group's record {count, Sx, Sy, 0}; point: its row of `points` (k f64)
TFRT_HD DistortionGroup distortion_group(const int64_t* rec, const double* point,
                                         const DistortionGrid& g) {
#pragma clang fp contract(off)
  DistortionGroup q;
  q.used = rec[0] > 0;
  q.w = q.px = q.py = q.cx = q.cy = 0.0;
  if (q.used) {
    q.w = (double)rec[0];
    q.cx = g.x0 + ((double)rec[1] / q.w) / g.qsx;
    q.px = point[0];
    if (g.two) {
      q.cy = g.y0 + ((double)rec[2] / q.w) / g.qsy;
      q.py = point[1];
    }
  }
  return q;
}

// first pass: s[0..4] += {w, w * px, w * py, w * cx, w * cy}
TFRT_HD void distortion_mean_terms(const DistortionGroup& q, double* s) {
#pragma clang fp contract(off)
  s[0] += q.w;
  s[1] += q.w * q.px;
  s[2] += q.w * q.py;
  s[3] += q.w * q.cx;
  s[4] += q.w * q.cy;
}

// The weighted means from the summed first pass: m = {pmx, pmy, cmx, cmy} (NaN with W == 0).
TFRT_HD void distortion_means(const double* s, double* m) {
#pragma clang fp contract(off)
  m[0] = s[1] / s[0];
  m[1] = s[2] / s[0];
  m[2] = s[3] / s[0];
  m[3] = s[4] / s[0];
}

// second pass: with dp = p - pm and dc = c - cm, s[0..6] += {w (dpx dpx), w (dpx dpy),
// w (dpy dpy), w (dcx dpx), w (dcx dpy), w (dcy dpx), w (dcy dpy)} -- the product of the two
// differences first, then times w.
TFRT_HD void distortion_moment_terms(const DistortionGroup& q, const double* m, double* s) {
#pragma clang fp contract(off)
  const double dpx = q.px - m[0], dpy = q.py - m[1];
  const double dcx = q.cx - m[2], dcy = q.cy - m[3];
  s[0] += q.w * (dpx * dpx);
  s[1] += q.w * (dpx * dpy);
  s[2] += q.w * (dpy * dpy);
  s[3] += q.w * (dcx * dpx);
  s[4] += q.w * (dcx * dpy);
  s[5] += q.w * (dcy * dpx);
  s[6] += q.w * (dcy * dpy);
}

// The fit from the summed second pass S = {Sxx, Sxy, Syy, Cxx, Cxy, Cyx, Cyy}, the means m and
// the number of used groups -> fit[8] = {A00, A01, A10, A11, t0, t1, valid, groups_used}; A and t
// are NaN without a valid fit.  Returns valid.
//   scale (and affine with one field): trp = Sxx + Syy, M = (Cxx + Cyy) / trp, A = M I;
//     valid iff used >= 2 and trp > 0.
//   affine: det = Sxx * Syy - Sxy * Sxy, h = trp / 2; valid iff det > min_cond * (h * h);
//     A = Scp Spp^-1 by cofactors, each entry (a * b - c * d) / det.
//   t = cm - A pm: t0 = cmx - (A00 * pmx + A01 * pmy), t1 alike.
TFRT_HD bool distortion_fit(const double* S, const double* m, long long used, int fit_kind,
                            bool two, double min_cond, double* fit) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  const double trp = S[0] + S[2];
  bool valid;
  double a00, a01, a10, a11;
  if (fit_kind == DISTORTION_FIT_AFFINE && two) {
    const double det = S[0] * S[2] - S[1] * S[1];
    const double h = trp / 2.0;
    valid = det > min_cond * (h * h);
    a00 = (S[3] * S[2] - S[4] * S[1]) / det;
    a01 = (S[4] * S[0] - S[3] * S[1]) / det;
    a10 = (S[5] * S[2] - S[6] * S[1]) / det;
    a11 = (S[6] * S[0] - S[5] * S[1]) / det;
  } else {
    valid = used >= 2 && trp > 0.0;
    a00 = a11 = (S[3] + S[6]) / trp;
    a01 = a10 = 0.0;
  }
  if (valid) {
    fit[0] = a00, fit[1] = a01, fit[2] = a10, fit[3] = a11;
    fit[4] = m[2] - (a00 * m[0] + a01 * m[1]);
    fit[5] = m[3] - (a10 * m[0] + a11 * m[1]);
  } else {
    for (int e = 0; e < 6; ++e) fit[e] = nan;
  }
  fit[6] = valid ? 1.0 : 0.0;
  fit[7] = (double)used;
  return valid;
}

// third pass: the residual r = c - (cm + A dp) of a used group (0.0 without a valid fit), NaN for
// an unused one; a used group adds w (rx rx) to e[0] and w (ry ry) to e[1].
TFRT_HD void distortion_residual(const DistortionGroup& q, const double* m, const double* fit,
                                 bool valid, double* r, double* e) {
#pragma clang fp contract(off)
  if (!q.used) {
    r[0] = r[1] = __builtin_nan("");
    return;
  }
  r[0] = r[1] = 0.0;
  if (valid) {
    const double dpx = q.px - m[0], dpy = q.py - m[1];
    r[0] = q.cx - (m[2] + (fit[0] * dpx + fit[1] * dpy));
    r[1] = q.cy - (m[3] + (fit[2] * dpx + fit[3] * dpy));
  }
  e[0] += q.w * (r[0] * r[0]);
  e[1] += q.w * (r[1] * r[1]);
}

}  // namespace tfrt
