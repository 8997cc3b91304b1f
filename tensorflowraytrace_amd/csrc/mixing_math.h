// The per-group and per-bin arithmetic of MixingError (tfrt_mixing.hip; the definition, operation
// by operation, is in include/tfrt_hip.h at tfrt_mixing_error): a cell's share of its group and
// of the pool, its squared difference and its pull, a group's error from the sum over its bins
// and its term of E_mix.  Float64 and int64 only, every operation rounded on its own.  Compiles
// for the host as well (the convention of centroid_math.h), so that tests/mixing_host checks it
// without a GPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

constexpr int MIXING_MAX_GROUPS = 1024;
constexpr int MIXING_MAX_CELLS = 1 << 20;   // n_groups * bins
constexpr int MIXING_USED_OUT = 2;          // {groups_used, N}

// Is the label of a source ray a group?
TFRT_HD bool mixing_label_ok(int32_t label, int32_t n_groups) {
  return label >= 0 && label < n_groups;
}

// What every cell of an evaluation shares: the pooled mass Nq as a double, N = Nq 2^-32 and the
// scale 2 B / N of the pulls.  Nq == 0: nothing landed, every pull is 0.
struct MixingPool {
  bool rays;
  double nq, n, scale;
};

TFRT_HD MixingPool mixing_pool(int64_t Nq, int64_t bins) {
#pragma clang fp contract(off)
  MixingPool P;
  P.rays = Nq > 0;
  P.nq = P.n = P.scale = 0.0;
  if (P.rays) {
    P.nq = (double)Nq;
    P.n = P.nq * 2.3283064365386963e-10;   // 2^-32: exact
    P.scale = (2.0 * (double)bins) / P.n;
  }
  return P;
}

// One cell of a group with mass nq_g > 0 in a pool with rays: p = Hq / nq_g, m = Pq / Nq,
// d = p - m; the pull D = scale * d goes to *pull, d * d is returned.
TFRT_HD double mixing_cell(int64_t hq, int64_t nq_g, int64_t pq, const MixingPool& P,
                           double* pull) {
#pragma clang fp contract(off)
  const double p = (double)hq / (double)nq_g;
  const double m = (double)pq / P.nq;
  const double d = p - m;
  *pull = P.scale * d;
  return d * d;
}

// e_g = B * (the sum of d * d over the group's bins); NaN for a group that is not used.
TFRT_HD double mixing_group_error(bool used, int64_t bins, double sum) {
#pragma clang fp contract(off)
  if (!used) return __builtin_nan("");
  return (double)bins * sum;
}

// The term of a used group in E_mix: (nq_g / Nq) * e_g.
TFRT_HD double mixing_term(int64_t nq_g, const MixingPool& P, double e_g) {
#pragma clang fp contract(off)
  return ((double)nq_g / P.nq) * e_g;
}

}  // namespace tfrt
