// What the coupled errors (tfrt_density.hip, tfrt_spot.hip) share: both add integers to a small
// table (a histogram, the groups' records) with atomics, sum a penalty for the columns outside the
// domain in a fixed shape, and seed the gradient from the same classification.
#pragma once
#include <type_traits>

#include "tfrt_common.h"

namespace tfrt {

// A kernel's weights argument is a base of its constants: NoWeights without weights -- an empty
// base, so the unweighted kernels' arguments are the constants alone, byte for byte --, the
// error's own weights struct with them.
struct NoWeights {};
template <bool WEIGHTED, typename W>
using weights_base = std::conditional_t<WEIGHTED, W, NoWeights>;

// v times the ray's weight, as the last operation on v; without weights v itself, no product.
template <bool WEIGHTED>
__device__ __forceinline__ double weighed(double v, double w) {
#pragma clang fp contract(off)
  if constexpr (WEIGHTED) return v * w;
  return v;
}

// fixed-shape sum over a workgroup of NW waves (V: double or long long): xor butterflies inside
// the wave, waves in index order; every thread of the workgroup must call it.  `wsum` is reused: a
// barrier at the end.
template <int NW, typename V>
__device__ __forceinline__ V error_block_sum(V v, V* wsum) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  V s = 0;
  for (int w = 0; w < NW; ++w) s += wsum[w];
  __syncthreads();
  return s;
}

// error_block_sum's sum -- the same butterflies inside the wave, the waves in index order from 0,
// the same bits -- with the sum over the waves made by thread 0 alone and handed round through
// `total` (one V in LDS).  Every thread still gets the sum; what changes is where the compiler may
// put the work.  In a kernel that makes several sums of which only thread 0 uses the result
// (k_centroid_table: five), error_block_sum's NW loads per sum stayed live in registers until the
// kernel's last block, because the adds were sunk into it: 126 registers and 276 bytes of scratch
// there; the store of the total ends every sum where it stands (42 registers, no scratch).  Every
// thread of the workgroup must call it.  `wsum` and `total` may be reused by the next call: that
// call writes `wsum` only in front of its first barrier, which every thread reaches after it has
// read `total` here, and thread 0 writes `total` only behind it.
template <int NW, typename V>
__device__ __forceinline__ V error_block_total(V v, V* wsum, V* total) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    V s = 0;
    for (int w = 0; w < NW; ++w) s += wsum[w];
    *total = s;
  }
  __syncthreads();
  return *total;
}

// The table (the histogram, the records of every group), cleared in front of the adds.  A launch,
// not a memset node: replayed inside a step's graph, a memset node in this place left the 896
// bytes of the imaging example's 28 records uncleared (every count came back as a stale word plus
// the rays added), and behind a source that is re-drawn in the graph it left every bin of the
// examples' histograms with a stale 2^46 (16,384 rays' worth) under the weights added; a kernel
// node in the same place clears them.  The cause is not known; the node costs what a memset node
// costs, one tiny launch.  (A template only so that both files that launch it can carry it.)
template <typename = void>
__global__ __launch_bounds__(BLOCK) void k_error_clear(unsigned long long* __restrict__ table,
                                                       int entries) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e < entries) table[e] = 0ull;
}

// One axis of a column outside the closed domain [lo, hi]: how far outside v lies (0 inside on
// this axis), and the derivative of that by v (-1, 0, +1).
__device__ __forceinline__ double outside_by(double v, double lo, double hi) {
#pragma clang fp contract(off)
  return fmax(lo - v, 0.0) + fmax(v - hi, 0.0);
}
__device__ __forceinline__ double outside_sign(double v, double lo, double hi) {
  return v < lo ? -1.0 : (v > hi ? 1.0 : 0.0);
}

// Workgroups of a grid-stride launch over n columns: one per `per_block` columns, at most `most`.
inline int error_grid(int64_t n, int per_block, int most) {
  if (n <= 0) return 0;
  const int64_t want = (n + per_block - 1) / per_block;
  return (int)(want < most ? want : most);
}

// The argument checks both *_error_run share: the columns, the fields, the domain constants
// (`sx`, `sy`: the scale of an axis), the buffers and the variant.
inline bool error_args_ok(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                          int32_t row_x, int32_t row_y, double x0, double x1, double sx, double y0,
                          double y1, double sy, double oob_weight, const double* grad,
                          int64_t grad_stride, const double* error_out, const int64_t* table,
                          int32_t variant, const void* workspace) {
  if (n < 0 || n > INT32_MAX || row_x == row_y || !error_out || !table || !workspace ||
      variant < 0 || variant > 2)
    return false;
  if (!(x1 > x0) || !(sx > 0.0) || !isfinite(sx) || !(oob_weight >= 0.0) || !isfinite(oob_weight) ||
      !isfinite(x0) || !isfinite(x1))
    return false;
  if (row_y >= 0 && (!(y1 > y0) || !(sy > 0.0) || !isfinite(sy) || !isfinite(y0) || !isfinite(y1)))
    return false;
  if (n > 0 && (!rows || !grad || stride < n || grad_stride < n)) return false;
  return state_dtype_ok(state_dtype);
}

// The dimension of the direction fields of a launch, chosen by the field codes on a `dim`-D block:
// fn gets a dim_tag<0> when both are rows of the block (position fields only), else a dim_tag<2>
// or dim_tag<3> (`[&](auto d) { constexpr int DIM = decltype(d)::value; ... }`).
template <int DIM>
struct dim_tag {
  static constexpr int value = DIM;
};
template <typename F>
inline void dispatch_fields(int dim, int row_x, int row_y, F&& fn) {
  if (row_x < 2 * dim && row_y < 2 * dim)
    fn(dim_tag<0>{});
  else if (dim == 3)
    fn(dim_tag<3>{});
  else
    fn(dim_tag<2>{});
}

}  // namespace tfrt
