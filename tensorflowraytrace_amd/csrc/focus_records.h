// The group records of FocusError, shared by the files that fill them (tfrt_focus.hip and
// tfrt_flatfield.hip): the constants of a launch, the classification of a column, the accumulate
// launch -- the ten slots of focus_record into the record of the ray's group -- and the entry's
// checks of the arguments both entries take, with the box constants they make.  The definition is
// in include/tfrt_hip.h at tfrt_focus_error; the launches are described at the top of
// tfrt_focus.hip.  Templates only, so that each file that launches them carries its own
// instantiations (as k_error_clear of error_sums.h).
#pragma once
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "focus_math.h"

namespace tfrt {

constexpr int FOCUS_LDS_GROUPS = 256;       // 10 planes of int64: 20 KiB per workgroup
constexpr int FOCUS_MAX_GROUPS = 1 << 20;
constexpr int FOCUS_MAX_GRID = 512;         // workgroups of the accumulate launch
constexpr int FOCUS_RAYS_PER_BLOCK = 4 * BLOCK;

struct FocusArgs {
  FocusBox box;
  double one;          // 2^pbits
  int64_t n_source;
  int32_t n_groups;
};

// Does column i count, and for which group?  Returns the label, or -1.  `link` is set whenever
// the mask lets the column through.
template <typename T, int DIM>
__device__ __forceinline__ int focus_classify(const T* __restrict__ rows, int64_t stride,
                                              const int32_t* __restrict__ mask,
                                              const int32_t* __restrict__ group,
                                              const int32_t* __restrict__ perm, int64_t i,
                                              const FocusArgs& g, LinkDir<DIM>& link) {
  if (mask != nullptr && mask[i] < 0) return -1;
  link = link_direction<T, DIM>(rows, stride, i);
  if (!link.ok) return -1;
  // (nothing is read out of bounds, whatever perm and group hold)
  const int64_t s = perm != nullptr ? (int64_t)perm[i] : i;
  if (s < 0 || s >= g.n_source) return -1;
  const int label = group[s];
  if (label < 0 || label >= g.n_groups) return -1;
  return focus_inside<DIM>(link.e, g.box) ? label : -1;
}

template <typename T, bool LDS, int DIM>
__global__ __launch_bounds__(BLOCK) void k_focus_accumulate(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, FocusArgs g,
    unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long table[];   // LDS variant: FOCUS_SLOTS planes of G each
  const int G = g.n_groups;
  if (LDS) {
    for (int e = threadIdx.x; e < FOCUS_SLOTS * G; e += BLOCK) table[e] = 0ull;
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    const int label = focus_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
    if (label < 0) continue;
    double m[DIM];
    int64_t q[FOCUS_SLOTS];
    focus_normalise<DIM>(link.e, g.box, m);
    focus_record<DIM>(link.d, m, g.one, q);
#pragma unroll
    for (int p = 0; p < FOCUS_SLOTS; ++p) {
      if (DIM == 2 && (p == 3 || p == 5 || p == 6 || p == 9)) continue;   // the z slots stay 0
      unsigned long long* at =
          LDS ? table + (p * G + label) : acc + (FOCUS_SLOTS * (int64_t)label + p);
      atomicAdd(at, (unsigned long long)q[p]);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < FOCUS_SLOTS * G; e += BLOCK) {
      const unsigned long long v = table[e];
      const int plane = e / G, label = e - plane * G;
      if (v != 0ull) atomicAdd(acc + (FOCUS_SLOTS * (int64_t)label + plane), v);
    }
  }
}

// The checks of the arguments tfrt_focus_error and tfrt_flatfield_error share (`table`: the
// per-group table either writes), and the constants of their launches: the box, its centre, R and
// iR, 2^pbits.  Returns 0 or TFRT_E_BADARG; the workspace is the caller's to check.
inline int focus_args(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                      int32_t dimension, const int32_t* group, int64_t n_source, int32_t n_groups,
                      const double (&domain)[6], int32_t pbits, double min_det, const double* grad,
                      int64_t grad_stride, const double* error_out, const int64_t* acc,
                      const double* table, int32_t variant, const void* workspace, FocusArgs& g) {
  if (dimension < 2 || dimension > 3 || n < 0 || n > INT32_MAX || n_source < 0 ||
      n_source > INT32_MAX || n_groups < 1 || n_groups > FOCUS_MAX_GROUPS || !group ||
      !error_out || !acc || !table || !workspace || variant < 0 || variant > 2 || pbits < 1 ||
      pbits > FOCUS_MAX_PBITS || !state_dtype_ok(state_dtype))
    return TFRT_E_BADARG;
  if (n >= ((int64_t)1 << (61 - pbits))) return TFRT_E_BADARG;   // n * 2 * 2^pbits stays below 2^62
  if (!(min_det > 0.0) || !isfinite(min_det)) return TFRT_E_BADARG;
  if (n > 0 && (!rows || !grad || stride < n || grad_stride < n)) return TFRT_E_BADARG;
  double half = 0.0;
  for (int a = 0; a < 3; ++a) {
    const bool used = a < dimension;
    g.box.lo[a] = used ? domain[2 * a] : 0.0;
    g.box.hi[a] = used ? domain[2 * a + 1] : 0.0;
    if (used && (!isfinite(g.box.lo[a]) || !isfinite(g.box.hi[a]) || !(g.box.hi[a] > g.box.lo[a])))
      return TFRT_E_BADARG;
    g.box.c[a] = 0.5 * (g.box.lo[a] + g.box.hi[a]);
    half = fmax(half, 0.5 * (g.box.hi[a] - g.box.lo[a]));
  }
  g.box.R = half, g.box.iR = 1.0 / half;
  if (!isfinite(g.box.iR) || !isfinite(half)) return TFRT_E_BADARG;
  if (variant == 1 && n_groups > FOCUS_LDS_GROUPS) return TFRT_E_BADARG;
  g.one = ldexp(1.0, pbits), g.n_source = n_source, g.n_groups = n_groups;
  return 0;
}

// The clear and the accumulate launch of both entries: `acc` zeroed, then the ten slots of every
// counting column (the table in LDS with `lds`, global atomics without).
template <typename T, int DIM>
inline void focus_fill_records(const T* rows, int64_t stride, int64_t n, const int32_t* mask,
                               const int32_t* group, const int32_t* perm, const FocusArgs& g,
                               bool lds, unsigned long long* acc, hipStream_t st) {
  const int grid = error_grid(n, FOCUS_RAYS_PER_BLOCK, FOCUS_MAX_GRID);
  const int entries = FOCUS_SLOTS * g.n_groups;
  hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(entries, BLOCK)), dim3(BLOCK), 0, st, acc,
                     entries);
  if (grid == 0) return;
  if (lds)
    hipLaunchKernelGGL((k_focus_accumulate<T, true, DIM>), dim3(grid), dim3(BLOCK),
                       (size_t)entries * sizeof(unsigned long long), st, rows, stride, n, mask,
                       group, perm, g, acc);
  else
    hipLaunchKernelGGL((k_focus_accumulate<T, false, DIM>), dim3(grid), dim3(BLOCK), 0, st, rows,
                       stride, n, mask, group, perm, g, acc);
}

}  // namespace tfrt
