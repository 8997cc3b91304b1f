// Shared device helpers for the tfrt HIP kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tfrt_hip.h"
#include "trace_math.h"

namespace tfrt {

constexpr int BLOCK = 256;       // 4 waves of 64
constexpr int WAVES = BLOCK / 64;

template <typename T>
__device__ __forceinline__ double ldd(const T* p, int64_t i) {
  return static_cast<double>(p[i]);
}

// One ray of a SoA ray block (ROWS rows of `stride` elements).
template <typename T>
__device__ __forceinline__ void load_ray3(const T* rays, int64_t stride, int64_t i, double s[3],
                                          double e[3]) {
  s[0] = ldd(rays, i);
  s[1] = ldd(rays, stride + i);
  s[2] = ldd(rays, 2 * stride + i);
  e[0] = ldd(rays, 3 * stride + i);
  e[1] = ldd(rays, 4 * stride + i);
  e[2] = ldd(rays, 5 * stride + i);
}

template <typename T>
__device__ __forceinline__ void store_ray3(T* rays, int64_t stride, int64_t i, const double s[3],
                                           const double e[3]) {
  rays[i] = static_cast<T>(s[0]);
  rays[stride + i] = static_cast<T>(s[1]);
  rays[2 * stride + i] = static_cast<T>(s[2]);
  rays[3 * stride + i] = static_cast<T>(e[0]);
  rays[4 * stride + i] = static_cast<T>(e[1]);
  rays[5 * stride + i] = static_cast<T>(e[2]);
}

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

// number of set bits of `mask` strictly below this lane
// (v_mbcnt_lo + v_mbcnt_hi: the hardware's masked bit count below the lane, two instructions;
// `popc(mask & lanes_below)` compiles to four)
__device__ __forceinline__ int rank_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                        __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Ordering point between LDS accesses of ONE wave that communicate across lanes.  The LDS
// executes a wave's instructions in issue order, so no wait is needed; this only keeps the
// compiler from moving memory accesses across it.
__device__ __forceinline__ void wave_fence() {
  __asm__ volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

inline int cdiv(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The element type of a ray block, chosen by a `state_dtype` code: fn gets a state_tag<T> for
// TFRT_F32 / TFRT_F64 / TFRT_F16 (`[&](auto tag) { using T = typename decltype(tag)::type; ... }`)
// and its result is returned; any other code returns `miss` without calling fn.
template <typename T>
struct state_tag {
  using type = T;
};
template <typename F>
inline int dispatch_state(int state_dtype, int miss, F&& fn) {
  switch (state_dtype) {
    case TFRT_F32: return fn(state_tag<float>{});
    case TFRT_F64: return fn(state_tag<double>{});
    case TFRT_F16: return fn(state_tag<_Float16>{});
    default: return miss;
  }
}
inline bool state_dtype_ok(int dtype) {
  return dtype == TFRT_F32 || dtype == TFRT_F64 || dtype == TFRT_F16;
}
// (an unknown code sizes like float32: the workspace sizing entries take any code)
inline size_t state_bytes(int dtype) { return dtype == TFRT_F64 ? 8 : (dtype == TFRT_F16 ? 2 : 4); }

// One pass's input rays: the source for pass 0, the previous pass's output otherwise.
template <typename T>
struct PassIn {
  const T* rays;
  int64_t stride;
  const int32_t* ids;    // source-ray index of a slot, or null: the slot itself
  const int32_t* last;   // the face (2-D: primitive) the ray left, or null: none
};

// What a forward entry (tfrt_trace3d_forward, tfrt_trace3d_compact, tfrt_trace2d_forward) hands
// its typed function, validated: the arguments of the C entry under the names used below it.
template <typename Scene>
struct TraceCall {
  const void* src;
  int64_t src_stride, N;
  const Scene* sc;
  double L, dead_len;
  int P, dtype;
  uint32_t flags;
  const tfrt_ray_out *fin, *act, *stp, *dead;
  void* unfinished;
  int32_t* unfinished_id;
  int32_t* counts;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t st;
};

// The counters a trace without a set-up launch starts from: the first pass's ray count, the
// trailing totals and the grid scan's ticket (when there is one).  (A template only so that the
// files that launch it are the ones that carry it.)
template <typename = void>
__global__ void k_init(int32_t* nrays0, int n, int32_t* tail8, unsigned int* scan_ticket) {
  if (threadIdx.x == 0) *nrays0 = n;
  if (threadIdx.x < 8) tail8[threadIdx.x] = 0;
  if (threadIdx.x == 0 && scan_ticket != nullptr) *scan_ticket = 0u;
}

// The first *n_ptr rays of a SoA block of ROWS rows, and their ids (their positions when the
// input has none).
template <typename T, int ROWS>
__global__ __launch_bounds__(BLOCK) void k_copy_rays(const T* __restrict__ in, int64_t sin,
                                                     const int32_t* __restrict__ id_in,
                                                     const int32_t* __restrict__ n_ptr,
                                                     T* __restrict__ out, int64_t sout,
                                                     int32_t* __restrict__ id_out) {
  const int n = *n_ptr;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  for (int k = 0; k < ROWS; ++k) out[k * sout + i] = in[k * sin + i];
  if (id_out) id_out[i] = id_in ? id_in[i] : i;
}

// scan_rows_grid's single-workgroup sibling (1024 threads, up to SCAN_GRID_MIN_ROWS rows): every
// thread takes a run of consecutive rows.  `off` receives global offsets (the consumer gets no
// rowbase), `total` (LDS, NB ints) the column sums, visible to every thread on return.
template <int NB>
__device__ __forceinline__ void scan_rows_one(const int32_t* __restrict__ cnt,
                                              int32_t* __restrict__ off, int nrows, int* total) {
  const int per = (nrows + 1023) / 1024;
  const int b0 = min(nrows, (int)threadIdx.x * per), b1 = min(nrows, b0 + per);
  int loc[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) loc[c] = 0;
  for (int b = b0; b < b1; ++b)
    for (int c = 0; c < NB; ++c) loc[c] += cnt[b * NB + c];
  __shared__ int wsum[16][NB];
  __shared__ int wbase[16][NB];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  int pre[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    int v = loc[c];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    pre[c] = v - loc[c];  // exclusive within the wave
    if (lane == 63) wsum[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < NB) {
    int run = 0;
    for (int w = 0; w < 16; ++w) {
      wbase[w][threadIdx.x] = run;
      run += wsum[w][threadIdx.x];
    }
    total[threadIdx.x] = run;
  }
  __syncthreads();
  int run[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) run[c] = wbase[wave][c] + pre[c];
  for (int b = b0; b < b1; ++b)
    for (int c = 0; c < NB; ++c) {
      off[b * NB + c] = run[c];
      run[c] += cnt[b * NB + c];
    }
}

// Exclusive scan of per-ray-block histograms (rows of NB counters, NB = 4 or 8) over a grid of
// 1024-thread workgroups, one row per thread: coalesced int4 loads and stores, a wave scan by
// shuffles and one exchange through LDS.  `off` receives the offsets *within the row's
// workgroup*; the workgroup that finishes last (a ticket) turns the per-workgroup sums `rowtot`
// into the bases `rowbase` (the consumer adds rowbase[(row >> 10) * NB + c]) and gets the column
// sums in `total` (LDS, NB ints): the function returns true there and false everywhere else.
// One workgroup scanning everything could not keep enough loads in flight: 54 us for the
// 15.6k rows of a 4M-ray pass.  `ticket` must be 0 on entry and is left 0.
template <int NB>
__device__ __forceinline__ bool scan_rows_grid(const int32_t* __restrict__ cnt,
                                               int32_t* __restrict__ off, int nrows,
                                               int32_t* __restrict__ rowtot,
                                               int32_t* __restrict__ rowbase,
                                               unsigned int* __restrict__ ticket, int* total) {
  static_assert(NB == 4 || NB == 8, "rows are one or two int4");
  constexpr int Q = NB / 4;
  __shared__ int wsum[16][NB];
  __shared__ int wbase[16][NB];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 1024 + (int)threadIdx.x;
  const int4* cnt4 = reinterpret_cast<const int4*>(cnt);
  int4* off4 = reinterpret_cast<int4*>(off);
  int v[NB], pre[NB];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int4 x = r < nrows ? cnt4[(int64_t)r * Q + q] : make_int4(0, 0, 0, 0);
    v[4 * q] = x.x;
    v[4 * q + 1] = x.y;
    v[4 * q + 2] = x.z;
    v[4 * q + 3] = x.w;
  }
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    int x = v[c];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(x, d, 64);
      if (lane >= d) x += o;
    }
    pre[c] = x - v[c];  // exclusive within the wave
    if (lane == 63) wsum[wave][c] = x;
  }
  __syncthreads();
  if (threadIdx.x < NB) {
    int run = 0;
    for (int w = 0; w < 16; ++w) {
      wbase[w][threadIdx.x] = run;
      run += wsum[w][threadIdx.x];
    }
    rowtot[blockIdx.x * NB + threadIdx.x] = run;
  }
  __syncthreads();
  if (r < nrows) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
      off4[(int64_t)r * Q + q] =
          make_int4(wbase[wave][4 * q] + pre[4 * q], wbase[wave][4 * q + 1] + pre[4 * q + 1],
                    wbase[wave][4 * q + 2] + pre[4 * q + 2], wbase[wave][4 * q + 3] + pre[4 * q + 3]);
  }
  // the last workgroup to arrive sees every rowtot (release / acquire through the ticket)
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = atomicAdd(ticket, 1u);
    is_last = (t == gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!is_last) return false;
  __threadfence();
  if (threadIdx.x < NB) {
    int run = 0;
    for (unsigned int b = 0; b < gridDim.x; ++b) {
      rowbase[b * NB + threadIdx.x] = run;
      run += __atomic_load_n(&rowtot[b * NB + threadIdx.x], __ATOMIC_RELAXED);
    }
    total[threadIdx.x] = run;
  }
  if (threadIdx.x == 0) *ticket = 0u;  // ready for the next pass
  __syncthreads();
  return true;
}

}  // namespace tfrt
