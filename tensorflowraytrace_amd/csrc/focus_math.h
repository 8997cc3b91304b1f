// The arithmetic of FocusError (tfrt_focus.hip; the definition, operation by operation, is in
// include/tfrt_hip.h at tfrt_focus_error): the normalised end point of a ray, the fixed-point
// record it adds to its group, the focus of a group from its record -- the determinant and the
// cofactor solve, every product and sum in the order written here --, and a ray's residual and
// gradient against that focus.  Float64 and int64 only, every operation rounded on its own.
// Compiles for the host as well (the convention of transport_math.h), so that tests/focus_host
// checks it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

// A record: {count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty, tz}; 2-D leaves the z slots 0.
constexpr int FOCUS_SLOTS = 10;
constexpr int FOCUS_MAX_PBITS = 40;

// The closed box of the domain, its centre c, R = the largest half-width, iR = 1 / R (from the
// host).  2-D: the z entries are 0.
struct FocusBox {
  double lo[3], hi[3], c[3], R, iR;
};

// end inside the closed box on every axis (a NaN is outside)
template <int DIM>
TFRT_HD bool focus_inside(const double* e, const FocusBox& b) {
  bool in = true;
  for (int a = 0; a < DIM; ++a) in = in && e[a] >= b.lo[a] && e[a] <= b.hi[a];
  return in;
}

// m_a = (e_a - c_a) * iR
template <int DIM>
TFRT_HD void focus_normalise(const double* e, const FocusBox& b, double* m) {
#pragma clang fp contract(off)
  for (int a = 0; a < DIM; ++a) m[a] = (e[a] - b.c[a]) * b.iR;
}

// v . w, the products summed left to right
template <int DIM>
TFRT_HD double focus_dot(const double* v, const double* w) {
#pragma clang fp contract(off)
  double s = v[0] * w[0] + v[1] * w[1];
  if (DIM == 3) s = s + v[2] * w[2];
  return s;
}

// rint(v * 2^pbits), half to even; `one` = 2^pbits
TFRT_HD int64_t focus_fixed(double v, double one) {
#pragma clang fp contract(off)
  return (int64_t)rint(v * one);
}

// The ten slots a ray adds: P = I - u u^T (P_aa = 1 - u_a * u_a, P_ab = -(u_a * u_b)) and
// t = P m as t_a = m_a - w * u_a with w = u . m.
template <int DIM>
TFRT_HD void focus_record(const double* u, const double* m, double one, int64_t* q) {
#pragma clang fp contract(off)
  for (int p = 0; p < FOCUS_SLOTS; ++p) q[p] = 0;
  const double w = focus_dot<DIM>(u, m);
  q[0] = 1;
  q[1] = focus_fixed(1.0 - u[0] * u[0], one);
  q[2] = focus_fixed(-(u[0] * u[1]), one);
  q[4] = focus_fixed(1.0 - u[1] * u[1], one);
  q[7] = focus_fixed(m[0] - w * u[0], one);
  q[8] = focus_fixed(m[1] - w * u[1], one);
  if (DIM == 3) {
    q[3] = focus_fixed(-(u[0] * u[2]), one);
    q[5] = focus_fixed(-(u[1] * u[2]), one);
    q[6] = focus_fixed(1.0 - u[2] * u[2], one);
    q[9] = focus_fixed(m[2] - w * u[2], one);
  }
}

// The focus of a group from its record: with n = (double) count, a = ((double) Aq * inv) / n and
// b = ((double) bq * inv) / n (inv = 2^-pbits), the cofactors and the determinant of a in the
// order below; a focus if count >= 2 and det >= min_det, then x = (cofactors . b) / det.
// Returns det (NaN with count < 1); `has` and x (NaN without a focus; 2-D: x[2] = 0 with one).
template <int DIM>
TFRT_HD double focus_solve(const int64_t* rec, double inv, double min_det, double* x, bool& has) {
#pragma clang fp contract(off)
  const double nan = __builtin_nan("");
  x[0] = x[1] = x[2] = nan;
  has = false;
  if (rec[0] < 1) return nan;
  const double n = (double)rec[0];
  const double a00 = ((double)rec[1] * inv) / n, a01 = ((double)rec[2] * inv) / n;
  const double a11 = ((double)rec[4] * inv) / n;
  const double b0 = ((double)rec[7] * inv) / n, b1 = ((double)rec[8] * inv) / n;
  if (DIM == 2) {
    const double det = a00 * a11 - a01 * a01;
    has = rec[0] >= 2 && det >= min_det;
    if (has) {
      x[0] = (a11 * b0 - a01 * b1) / det;
      x[1] = (a00 * b1 - a01 * b0) / det;
      x[2] = 0.0;
    }
    return det;
  }
  const double a02 = ((double)rec[3] * inv) / n, a12 = ((double)rec[5] * inv) / n;
  const double a22 = ((double)rec[6] * inv) / n;
  const double b2 = ((double)rec[9] * inv) / n;
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  has = rec[0] >= 2 && det >= min_det;
  if (has) {
    x[0] = (c00 * b0 + c01 * b1 + c02 * b2) / det;
    x[1] = (c01 * b0 + c11 * b1 + c12 * b2) / det;
    x[2] = (c02 * b0 + c12 * b1 + c22 * b2) / det;
  }
  return det;
}

// A ray against the focus x of its group: q = m - x, a = u . q, r = q - a u, rho = R r,
// alpha = R a; the term rho . rho; with lever = alpha / L the gradient
// end_b = (2 rho_b) * (1 - lever), start_b = (2 rho_b) * lever.
template <int DIM>
TFRT_HD double focus_term(const double* u, const double* m, const double* x, double R, double L,
                          double* g_start, double* g_end) {
#pragma clang fp contract(off)
  double q[DIM], rho[DIM];
  for (int b = 0; b < DIM; ++b) q[b] = m[b] - x[b];
  const double a = focus_dot<DIM>(u, q);
  for (int b = 0; b < DIM; ++b) rho[b] = R * (q[b] - a * u[b]);
  const double lever = (R * a) / L;
  const double rest = 1.0 - lever;
  for (int b = 0; b < DIM; ++b) {
    const double two = 2.0 * rho[b];
    g_end[b] = two * rest;
    g_start[b] = two * lever;
  }
  return focus_dot<DIM>(rho, rho);
}

}  // namespace tfrt
