// The per-ray arithmetic of TransportError (tfrt_transport.hip; the definition, operation by
// operation, is in include/tfrt_hip.h at tfrt_transport_error): the projection of a landing point
// onto a direction, its integer sort key, and the target it is pulled to -- the goal's quantile at
// the ray's mid-rank, read from a table of Q + 1 knots.  Float64 only, every operation rounded on
// its own.  Compiles for the host as well (the convention of density_map.h), so that
// tests/transport_host checks it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

// Width of a sort key: two digits of 13 bits, the widest the radix sort of tfrt_order.hip takes in
// two passes.  ops.TRANSPORT_KEY_BITS and tests/transport_error_reference.py carry the same number.
constexpr int TRANSPORT_KEY_BITS = 26;
constexpr uint32_t TRANSPORT_KEY_INVALID = (1u << TRANSPORT_KEY_BITS) - 1u;   // sorts last
constexpr int TRANSPORT_MAX_DIRECTIONS = 64;
constexpr int TRANSPORT_MAX_KNOTS = 65536;

// One projection direction (c, s) = (cos, sin): a point of the unit square projects into [a, b],
// a = min(0, c) + min(0, s), b = max(0, c) + max(0, s); the keys cover three times that width,
// [a - (b - a), b + (b - a)], so a ray up to one domain width outside still has a key of its own.
struct TransportDirection {
  double c, s, lo, scale;
};

TFRT_HD TransportDirection transport_direction(double c, double s) {
#pragma clang fp contract(off)
  TransportDirection d;
  const double a = fmin(0.0, c) + fmin(0.0, s);
  const double b = fmax(0.0, c) + fmax(0.0, s);
  d.c = c, d.s = s;
  d.lo = a - (b - a);
  d.scale = (double)(1u << TRANSPORT_KEY_BITS) / (3.0 * (b - a));
  return d;
}

// xi = (x - x0) * ix, with ix = 1 / (x1 - x0) from the host.
TFRT_HD double transport_normalise(double x, double x0, double ix) {
#pragma clang fp contract(off)
  return (x - x0) * ix;
}

// p = c * xi + s * eta: two products, one sum.  (One field: p = xi, no arithmetic.)
TFRT_HD double transport_project(double c, double s, double xi, double eta) {
#pragma clang fp contract(off)
  const double pc = c * xi;
  const double ps = s * eta;
  return pc + ps;
}

// q = clamp(floor((p - lo) * scale), 0, 2^26 - 2), the comparisons written so that a NaN takes 0.
TFRT_HD uint32_t transport_key(const TransportDirection& d, double p) {
#pragma clang fp contract(off)
  const double top = (double)(TRANSPORT_KEY_INVALID - 1u);
  const double v = floor((p - d.lo) * d.scale);
  if (!(v >= 0.0)) return 0u;
  return v <= top ? (uint32_t)v : TRANSPORT_KEY_INVALID - 1u;
}

// The target of a ray of mid-rank rank2 / 2 among n_valid: u = (rank2 * 0.5) / n_valid -- exactly
// (first + count * 0.5) / n_valid, both numerators are exact --, z = u * Q, m = min(floor(z),
// Q - 1), f = z - m, t = T[m] + f * (T[m + 1] - T[m]).  Reads T[0 .. Q] only: rank2 <= 2 n_valid.
TFRT_HD double transport_target(const double* T, int Q, int32_t rank2, int32_t n_valid) {
#pragma clang fp contract(off)
  const double u = ((double)rank2 * 0.5) / (double)n_valid;
  const double z = u * (double)Q;
  double fm = floor(z);
  if (!(fm >= 0.0)) fm = 0.0;
  if (fm > (double)(Q - 1)) fm = (double)(Q - 1);
  const int m = (int)fm;
  const double f = z - fm;
  const double t0 = T[m];
  return t0 + f * (T[m + 1] - t0);
}

}  // namespace tfrt
