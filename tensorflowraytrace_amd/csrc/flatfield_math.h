// The arithmetic of FlatFieldError (tfrt_flatfield.hip; the definition, operation by operation, is
// in include/tfrt_hip.h at tfrt_flatfield_error): the focus x = A^-1 b of a group with
// y = A^-1 a beside it (a: the unit normal of the plane) by focus_math.h's cofactors, a group's
// residual, error and adjoint against the plane's height, and a ray's gradient from the adjoint of
// its group.  Everything up to the focus is focus_math.h's, which this file uses as it stands.
// Float64 and int64 only, every operation rounded on its own.  Compiles for the host as well (the
// convention of focus_math.h), so that tests/flatfield_host checks it without a GPU.
#pragma once
#include "focus_math.h"

namespace tfrt {

// A row of the table: {x0, x1, x2, used, mu0, mu1, mu2, e_g}, 64 bytes.
constexpr int FLATFIELD_ROW = 8;
// fit_out: {hbar, a . c + R * hbar, W, groups used, valid, 0, 0, 0}
constexpr int FLATFIELD_FIT_OUT = 8;

// focus_solve (the same x, `has` and det, bit for bit) and, for a group with a focus,
// y = (cofactors . a) / det with the same cofactors in the same order (2-D: y[2] = 0); y is 0
// without a focus.
template <int DIM>
TFRT_HD double flatfield_solve(const int64_t* rec, double inv, double min_det, const double* axis,
                               double* x, double* y, bool& has) {
#pragma clang fp contract(off)
  const double det = focus_solve<DIM>(rec, inv, min_det, x, has);
  y[0] = y[1] = y[2] = 0.0;
  if (!has) return det;
  const double n = (double)rec[0];
  const double a00 = ((double)rec[1] * inv) / n, a01 = ((double)rec[2] * inv) / n;
  const double a11 = ((double)rec[4] * inv) / n;
  if (DIM == 2) {
    y[0] = (a11 * axis[0] - a01 * axis[1]) / det;
    y[1] = (a00 * axis[1] - a01 * axis[0]) / det;
    return det;
  }
  const double a02 = ((double)rec[3] * inv) / n, a12 = ((double)rec[5] * inv) / n;
  const double a22 = ((double)rec[6] * inv) / n;
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  y[0] = (c00 * axis[0] + c01 * axis[1] + c02 * axis[2]) / det;
  y[1] = (c01 * axis[0] + c11 * axis[1] + c12 * axis[2]) / det;
  y[2] = (c02 * axis[0] + c12 * axis[1] + c22 * axis[2]) / det;
  return det;
}

// A used group against the plane's height hbar: r = h - hbar, s = R * r, e = s * s and the adjoint
// mu_b = (2 * s) * y_b (2-D: mu[2] = 0).  Returns e.
template <int DIM>
TFRT_HD double flatfield_group(double h, double hbar, double R, const double* y, double* mu) {
#pragma clang fp contract(off)
  const double s = R * (h - hbar);
  const double two = 2.0 * s;
  mu[0] = two * y[0];
  mu[1] = two * y[1];
  mu[2] = DIM == 3 ? two * y[2] : 0.0;
  return s * s;
}

// A counting ray of a used group, against the focus x and the adjoint mu of its group:
// focus_term's q = m - x, alpha = u . q, rho = R * (q - alpha * u), lever = (R * alpha) / L; then
// beta = mu . u, muP = mu - beta * u, k = beta / L and
// end_b = muP_b * (1 - lever) - k * rho_b, start_b = muP_b * lever + k * rho_b.
template <int DIM>
TFRT_HD void flatfield_ray(const double* u, const double* m, const double* x, const double* mu,
                           double R, double L, double* g_start, double* g_end) {
#pragma clang fp contract(off)
  double q[DIM];
  for (int b = 0; b < DIM; ++b) q[b] = m[b] - x[b];
  const double alpha = focus_dot<DIM>(u, q);
  const double lever = (R * alpha) / L;
  const double rest = 1.0 - lever;
  const double beta = focus_dot<DIM>(mu, u);
  const double k = beta / L;
  for (int b = 0; b < DIM; ++b) {
    const double rho = R * (q[b] - alpha * u[b]);
    const double muP = mu[b] - beta * u[b];
    const double turn = k * rho;
    g_end[b] = muP * rest - turn;
    g_start[b] = muP * lever + turn;
  }
}

}  // namespace tfrt
