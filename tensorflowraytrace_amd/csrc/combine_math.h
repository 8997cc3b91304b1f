// The per-element arithmetic of a sum of error terms (tfrt_combine.hip; the definitions, operation
// by operation, are in include/tfrt_hip.h at tfrt_goal_error_columns and tfrt_error_combine): a
// GoalError's residual, term and seed on a fixed-shape column, a term's coefficient, and the
// weighted accumulation of seeds and errors.  Float64 only, every operation rounded on its own.
// Compiles for the host as well (the convention of transport_math.h), so that tests/combine_host
// checks it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef TFRT_HD
#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif
#endif

namespace tfrt {

constexpr int COMBINE_MAX_TERMS = 8;

// Whether column i has a source ray: s = perm ? perm[i] : i inside [0, n_source).
TFRT_HD bool goal_source_ok(int64_t s, int64_t n_source) { return s >= 0 && s < n_source; }

// d = o - goal, the term d * d, the seed 2 * d.
TFRT_HD double goal_residual(double o, double goal) {
#pragma clang fp contract(off)
  return o - goal;
}
TFRT_HD double goal_term(double d) {
#pragma clang fp contract(off)
  return d * d;
}
TFRT_HD double goal_seed(double d) {
#pragma clang fp contract(off)
  return 2.0 * d;
}

// c_k: the weight itself (reduce == 0, sum), or the weight over the term's own count of error
// terms (reduce == 1, mean) -- 0.0 for a term that has none, so that its NaN-free sum drops out.
TFRT_HD double combine_coefficient(double weight, double terms, int reduce) {
#pragma clang fp contract(off)
  if (reduce == 0) return weight;
  return terms > 0.0 ? weight / terms : 0.0;
}

// acc = c * g for the first term of a row -- not added to a zero: one term with weight 1.0 comes
// back with its own bits, -0.0 included --, acc = acc + c * g for every later one; the product and
// the sum are two roundings.
TFRT_HD double combine_first(double c, double g) {
#pragma clang fp contract(off)
  return c * g;
}
TFRT_HD double combine_next(double acc, double c, double g) {
#pragma clang fp contract(off)
  const double p = c * g;
  return acc + p;
}

}  // namespace tfrt
