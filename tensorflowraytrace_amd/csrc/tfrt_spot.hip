// SpotError: rays that left the same object point must meet in one point -- wherever that is.
//
// Every source ray carries a group label; the finished rays of a group form a spot, and the error
// is the sum over the rays of |x - c|^2 with c the CENTROID of the ray's own group (the squared RMS
// spot size times the ray count, the basic merit function of lens design), plus a penalty for rays
// outside the domain.  The definition, operation by operation, is in include/tfrt_hip.h at
// tfrt_spot_error; tests/spot_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: a coordinate enters its group's record as the INTEGER
// rint((x - x0) * qs), qs = 2^qbits / (x1 - x0), with n * 2^qbits < 2^62: int64 sums that cannot
// overflow and do not depend on the order in which the atomics land.  Every floating-point
// reduction has a fixed shape and order.  No float atomics and no compare-and-swap loop anywhere.
//
// The gradient needs no derivative of the centroid: d/dx_i sum_j |x_j - c|^2 = 2 (x_i - c) -
// 2 (dc/dx_i) sum_j (x_j - c), and the residuals of a group sum to zero.
//
// Four launches:
//
//   k_spot_clear       zeroes the records.  A launch, not a memset node: replayed inside the step's
//                      graph, a memset node in this place left the 896 bytes of the imaging
//                      example's 28 records uncleared (every count came back as a stale word plus the
//                      rays added); a kernel node in the same place clears them.  The cause is not
//                      known; the node costs what a memset node costs, one tiny launch.
//   k_spot_accumulate  one lane per column (a fixed grid for n, grid-stride): {1, qx, qy} -> the
//                      record of the ray's group; the out-of-domain penalty and the number of
//                      counting columns as one partial per workgroup.  Two variants:
//                      <true>  G <= SPOT_LDS_GROUPS: a per-workgroup table in LDS (ds_add_u64),
//                              kept as three planes of G int64 (24 B x G <= 24 KiB, consecutive
//                              labels in consecutive banks; four workgroups fit a CU), flushed with
//                              one global atomic per non-zero entry.  Many rays share few groups:
//                              the contention stays in LDS.
//                      <false> more groups: three global 64-bit atomics per ray, all in the ray's
//                              one 32-byte record.
//   k_spot_seed        one lane per column (a fixed grid for n, grid-stride): the same
//                      classification, the centroid of the ray's own group from its record (three
//                      loads, two divisions: no centroid launch and no centroid table), both
//                      gradient rows of EVERY column (zeros where a ray does not count), the inside
//                      terms as one partial per workgroup.
//   k_spot_finish      ONE workgroup: the partials in index order, {sum, terms, mean}.
//
// A field is a row of the ray block or a direction cosine of the finished ray's last link
// (tfrt_spot_error_fields: rays of one group must leave PARALLEL; the codes, the direction and the
// chain rule of its gradient: direction_fields.h).  The accumulate and the seed are templated on
// "has a direction field": without one they are the kernels of position fields, load for load;
// with one they recompute the direction from the rows they stream, and the seed writes EVERY row
// of the column.
//
// Weighted (tfrt_spot_error_weighted): every source ray carries a radiant power w in [0, 1], which
// enters as the INTEGER wq = rint(w * 2^wbits); wr = wq * 2^-wbits is the weight everywhere, so the
// weighted residuals of a group sum to zero in the quantised quantities.  The product wq * qx is
// kept in two limbs (wq * (qx >> h) and wq * (qx & (2^h - 1)), h = qbits / 2) so that the position
// keeps its full qbits; a record is one 64-byte line of eight int64
// {W, Xhi, Xlo, Yhi, Ylo, count, 0, 0}.  The accumulate and the seed are sibling kernels
// (k_spot_accumulate_weighted, k_spot_seed_weighted) with the weights as one more argument; the
// unweighted kernels are untouched.  The weight is read once per column through `perm`, behind
// the index check that the label lookup needs anyway.  The table in LDS has six planes of G
// int64: SPOT_WEIGHTED_LDS_GROUPS = 512 keeps it at the 24 KiB of the unweighted table at 1,024
// groups -- six workgroups, 24 waves, share a CU's 160 KiB; twice the table would leave three, too
// few to hide the latency of the ds_add_u64 behind other waves' loads.  More groups: six global
// 64-bit atomics, all in the ray's one line.
#include "tfrt_common.h"
#include "direction_fields.h"

namespace tfrt {

constexpr int SPOT_LDS_GROUPS = 1024;      // 3 planes of int64: 24 KiB per workgroup
constexpr int SPOT_WEIGHTED_LDS_GROUPS = 512;   // weighted, 6 planes of int64: 24 KiB
constexpr int SPOT_MAX_WBITS = 20;
constexpr int SPOT_MAX_GROUPS = 1 << 20;
constexpr int SPOT_MAX_GRID = 512;         // workgroups of the accumulate launch
constexpr int SPOT_RAYS_PER_BLOCK = 4 * BLOCK;
constexpr int SPOT_SEED_MAX_GRID = 8192;   // workgroups of the seed launch (one column per lane up to 2M)
constexpr int FINISH_BLOCK = 1024;
constexpr int FINISH_WAVES = FINISH_BLOCK / 64;

struct SpotGrid {
  double x0, x1, qsx, y0, y1, qsy, oob, qmax;
  int64_t n_source;
  int32_t n_groups, row_x, row_y;   // row_x, row_y: field codes (direction_fields.h)
};

// The weights of tfrt_spot_error_weighted: one f64 in [0, 1] per SOURCE ray.
struct SpotWeights {
  const double* weight;
  double one, inv;           // 2^wbits, 2^-wbits
  int32_t h;                 // qbits / 2: the low limb's bits
};

// What one column does.  kind 0: masked off; 3: counts, but contributes nothing (a non-finite
// coordinate, or no spot); 1: inside the closed domain; 2: outside, ex / ey and their signs.
struct SpotRay {
  int kind;
  int label;
  double x, y;       // kind 1: the coordinates; kind 2: ex, ey
  double dx, dy;     // kind 2: d ex / d x, d ey / d y (-1, 0, +1)
};

template <typename T, int DIM>
__device__ __forceinline__ SpotRay spot_classify(const T* __restrict__ rows, int64_t stride,
                                                 const int32_t* __restrict__ mask,
                                                 const int32_t* __restrict__ group,
                                                 const int32_t* __restrict__ perm, int64_t i,
                                                 const SpotGrid& g, LinkDir<DIM>& link) {
#pragma clang fp contract(off)
  SpotRay r;
  r.kind = 0;
  r.label = 0;
  r.x = r.y = r.dx = r.dy = 0.0;
  if (mask != nullptr && mask[i] < 0) return r;
  r.kind = 3;
  const bool two = g.row_y >= 0;
  double x, y;
  read_fields<T, DIM>(rows, stride, i, g.row_x, g.row_y, x, y, link);
  if (!isfinite(x) || !isfinite(y)) return r;
  // (nothing is read out of bounds, whatever perm and group hold)
  const int64_t s = perm != nullptr ? (int64_t)perm[i] : i;
  if (s < 0 || s >= g.n_source) return r;
  const int label = group[s];
  if (label < 0 || label >= g.n_groups) return r;
  r.label = label;
  const bool out = x < g.x0 || x > g.x1 || (two && (y < g.y0 || y > g.y1));
  if (out) {
    r.kind = 2;
    r.x = fmax(g.x0 - x, 0.0) + fmax(x - g.x1, 0.0);
    r.dx = x < g.x0 ? -1.0 : (x > g.x1 ? 1.0 : 0.0);
    if (two) {
      r.y = fmax(g.y0 - y, 0.0) + fmax(y - g.y1, 0.0);
      r.dy = y < g.y0 ? -1.0 : (y > g.y1 ? 1.0 : 0.0);
    }
    return r;
  }
  r.kind = 1;
  r.x = x;
  r.y = y;
  return r;
}

// The same for tfrt_spot_error_weighted: a column with a spot (kinds 1 and 2) whose weight does not
// count or quantises to 0 is in no spot (kind 3 -- every "no spot" case ends alike, so the order of
// the checks does not show).  s has passed spot_classify's index check; the read of perm is the one
// that served the label.  wq = rint(w * 2^wbits) > 0, wr = wq * 2^-wbits.
template <typename T, int DIM>
__device__ __forceinline__ SpotRay spot_classify_weighted(
    const T* __restrict__ rows, int64_t stride, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, int64_t i,
    const SpotGrid& g, const SpotWeights& wt, LinkDir<DIM>& link, double& wq, double& wr) {
#pragma clang fp contract(off)
  SpotRay r = spot_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
  wq = wr = 0.0;
  if (r.kind == 1 || r.kind == 2) {
    const int64_t s = perm != nullptr ? (int64_t)perm[i] : i;
    // (a NaN fails both comparisons; the product with a power of two is exact)
    const double w = wt.weight[s];
    wq = w >= 0.0 && w <= 1.0 ? rint(w * wt.one) : 0.0;
    wr = wq * wt.inv;
    if (wq == 0.0) r.kind = 3;
  }
  return r;
}

__device__ __forceinline__ unsigned long long spot_fixed(double v, double lo, double qs,
                                                         double qmax) {
#pragma clang fp contract(off)
  // round half to even (v_rndne_f64); the clamp keeps the closed domain inside [0, 2^qbits]
  return (unsigned long long)(long long)fmin(fmax(rint((v - lo) * qs), 0.0), qmax);
}

// fixed-shape sums over a workgroup of NW waves: xor butterflies inside the wave, waves in index
// order; every thread of the workgroup must call them.  `wsum` is reused: a barrier at the end.
template <int NW>
__device__ __forceinline__ double spot_block_sum(double v, double* wsum) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < NW; ++w) s += wsum[w];
  __syncthreads();
  return s;
}

template <int NW>
__device__ __forceinline__ long long spot_block_count(long long v, long long* wcnt) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane_id() == 0) wcnt[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int w = 0; w < NW; ++w) s += wcnt[w];
  __syncthreads();
  return s;
}

// The records of every group, cleared in front of the adds.
__global__ __launch_bounds__(BLOCK) void k_spot_clear(unsigned long long* __restrict__ acc,
                                                      int entries) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e < entries) acc[e] = 0ull;
}

template <typename T, bool LDS, int DIM>
__global__ __launch_bounds__(BLOCK) void k_spot_accumulate(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotGrid g,
    unsigned long long* __restrict__ acc, double* __restrict__ pen_partial,
    long long* __restrict__ cnt_partial) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long table[];   // LDS variant: planes count | Sx | Sy of G each
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  const int G = g.n_groups;
  const bool two = g.row_y >= 0;
  if (LDS) {
    for (int e = threadIdx.x; e < 3 * G; e += BLOCK) table[e] = 0ull;
    __syncthreads();
  }
  double pen = 0.0;
  long long counting = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    const SpotRay r = spot_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
    counting += r.kind != 0 ? 1 : 0;
    if (r.kind == 2) {
      pen += g.oob * (r.x * r.x + r.y * r.y);
    } else if (r.kind == 1) {
      const unsigned long long qx = spot_fixed(r.x, g.x0, g.qsx, g.qmax);
      const unsigned long long qy = two ? spot_fixed(r.y, g.y0, g.qsy, g.qmax) : 0ull;
      if (LDS) {
        atomicAdd(&table[r.label], 1ull);
        atomicAdd(&table[G + r.label], qx);
        if (two) atomicAdd(&table[2 * G + r.label], qy);
      } else {
        unsigned long long* rec = acc + 4 * (int64_t)r.label;
        atomicAdd(&rec[0], 1ull);
        atomicAdd(&rec[1], qx);
        if (two) atomicAdd(&rec[2], qy);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * G; e += BLOCK) {
      const unsigned long long v = table[e];
      const int plane = e / G, label = e - plane * G;
      if (v != 0ull) atomicAdd(&acc[4 * (int64_t)label + plane], v);
    }
  }
  const double s = spot_block_sum<WAVES>(pen, wsum);
  const long long c = spot_block_count<WAVES>(counting, wcnt);
  if (threadIdx.x == 0) {
    pen_partial[blockIdx.x] = s;
    cnt_partial[blockIdx.x] = c;
  }
}

// tfrt_spot_error_weighted's accumulate: the planes W | Xhi | Xlo | Yhi | Ylo | count of G each in
// LDS -- the order of a record of eight int64 --, or six global atomics in the ray's one line.
template <typename T, bool LDS, int DIM>
__global__ __launch_bounds__(BLOCK) void k_spot_accumulate_weighted(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotGrid g,
    SpotWeights wt, unsigned long long* __restrict__ acc, double* __restrict__ pen_partial,
    long long* __restrict__ cnt_partial) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long table[];
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  const int G = g.n_groups;
  const bool two = g.row_y >= 0;
  const unsigned long long low = (1ull << wt.h) - 1ull;
  if (LDS) {
    for (int e = threadIdx.x; e < 6 * G; e += BLOCK) table[e] = 0ull;
    __syncthreads();
  }
  double pen = 0.0;
  long long counting = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq, wr;
    const SpotRay r =
        spot_classify_weighted<T, DIM>(rows, stride, mask, group, perm, i, g, wt, link, wq, wr);
    counting += r.kind != 0 ? 1 : 0;
    if (r.kind == 2) {
      pen += (g.oob * (r.x * r.x + r.y * r.y)) * wr;
    } else if (r.kind == 1) {
      const unsigned long long q = (unsigned long long)(long long)wq;
      const unsigned long long qx = spot_fixed(r.x, g.x0, g.qsx, g.qmax);
      const unsigned long long qy = two ? spot_fixed(r.y, g.y0, g.qsy, g.qmax) : 0ull;
      if (LDS) {
        atomicAdd(&table[r.label], q);
        atomicAdd(&table[G + r.label], q * (qx >> wt.h));
        atomicAdd(&table[2 * G + r.label], q * (qx & low));
        if (two) {
          atomicAdd(&table[3 * G + r.label], q * (qy >> wt.h));
          atomicAdd(&table[4 * G + r.label], q * (qy & low));
        }
        atomicAdd(&table[5 * G + r.label], 1ull);
      } else {
        unsigned long long* rec = acc + 8 * (int64_t)r.label;
        atomicAdd(&rec[0], q);
        atomicAdd(&rec[1], q * (qx >> wt.h));
        atomicAdd(&rec[2], q * (qx & low));
        if (two) {
          atomicAdd(&rec[3], q * (qy >> wt.h));
          atomicAdd(&rec[4], q * (qy & low));
        }
        atomicAdd(&rec[5], 1ull);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < 6 * G; e += BLOCK) {
      const unsigned long long v = table[e];
      const int plane = e / G, label = e - plane * G;
      if (v != 0ull) atomicAdd(&acc[8 * (int64_t)label + plane], v);
    }
  }
  const double s = spot_block_sum<WAVES>(pen, wsum);
  const long long c = spot_block_count<WAVES>(counting, wcnt);
  if (threadIdx.x == 0) {
    pen_partial[blockIdx.x] = s;
    cnt_partial[blockIdx.x] = c;
  }
}

template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_spot_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotGrid g,
    const long long* __restrict__ acc, double* __restrict__ grad, int64_t grad_stride,
    double* __restrict__ term_partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  const bool two = g.row_y >= 0;
  double terms = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    const SpotRay r = spot_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
    double gx = 0.0, gy = 0.0;
    if (r.kind == 2) {
      gx = g.oob * (2.0 * r.x) * r.dx;
      gy = g.oob * (2.0 * r.y) * r.dy;
    } else if (r.kind == 1) {
      // (this ray is in its own group's record: count >= 1)
      const long long* rec = acc + 4 * (int64_t)r.label;
      const double cnt = (double)rec[0];
      const double cx = g.x0 + ((double)rec[1] / cnt) / g.qsx;
      const double dx = r.x - cx;
      gx = 2.0 * dx;
      double t = dx * dx;
      if (two) {
        const double cy = g.y0 + ((double)rec[2] / cnt) / g.qsy;
        const double dy = r.y - cy;
        gy = 2.0 * dy;
        t = t + dy * dy;
      }
      terms += t;
    }
    if constexpr (DIM != 0) {
      // (every row of the column: a direction pulls on the start and on the end of the link)
      chain_fields<DIM>(link, r.kind == 1 || r.kind == 2, g.row_x, g.row_y, gx, gy, grad,
                   grad_stride, i);
    } else {
      grad[(int64_t)g.row_x * grad_stride + i] = gx;
      if (two) grad[(int64_t)g.row_y * grad_stride + i] = gy;
    }
  }
  const double s = spot_block_sum<WAVES>(terms, wsum);
  if (threadIdx.x == 0) term_partial[blockIdx.x] = s;
}

// tfrt_spot_error_weighted's seed: the centroid from the two limbs, everything times wr last.
template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_spot_seed_weighted(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotGrid g,
    SpotWeights wt, const long long* __restrict__ acc, double* __restrict__ grad,
    int64_t grad_stride, double* __restrict__ term_partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  const bool two = g.row_y >= 0;
  double terms = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq, wr;
    const SpotRay r =
        spot_classify_weighted<T, DIM>(rows, stride, mask, group, perm, i, g, wt, link, wq, wr);
    double gx = 0.0, gy = 0.0;
    if (r.kind == 2) {
      gx = (g.oob * (2.0 * r.x) * r.dx) * wr;
      gy = (g.oob * (2.0 * r.y) * r.dy) * wr;
    } else if (r.kind == 1) {
      // (this ray is in its own group's record: W >= wq >= 1)
      const long long* rec = acc + 8 * (int64_t)r.label;
      const double W = (double)rec[0];
      const double X = ldexp((double)rec[1], wt.h) + (double)rec[2];
      const double cx = g.x0 + (X / W) / g.qsx;
      const double dx = r.x - cx;
      gx = (2.0 * dx) * wr;
      double t = wr * (dx * dx);
      if (two) {
        const double Y = ldexp((double)rec[3], wt.h) + (double)rec[4];
        const double cy = g.y0 + (Y / W) / g.qsy;
        const double dy = r.y - cy;
        gy = (2.0 * dy) * wr;
        t = t + wr * (dy * dy);
      }
      terms += t;
    }
    if constexpr (DIM != 0) {
      chain_fields<DIM>(link, r.kind == 1 || r.kind == 2, g.row_x, g.row_y, gx, gy, grad,
                   grad_stride, i);
    } else {
      grad[(int64_t)g.row_x * grad_stride + i] = gx;
      if (two) grad[(int64_t)g.row_y * grad_stride + i] = gy;
    }
  }
  const double s = spot_block_sum<WAVES>(terms, wsum);
  if (threadIdx.x == 0) term_partial[blockIdx.x] = s;
}

// One workgroup.  Thread t owns partials t, t + 1024, ... (summed in that order), then the
// fixed-shape workgroup sum: the same bits on every run.
__global__ __launch_bounds__(FINISH_BLOCK) void k_spot_finish(
    const double* __restrict__ pen_partial, const long long* __restrict__ cnt_partial, int n_acc,
    const double* __restrict__ term_partial, int n_seed, int fields,
    double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FINISH_WAVES];
  __shared__ long long wcnt[FINISH_WAVES];
  const int t = threadIdx.x;
  double pen = 0.0, inside = 0.0;
  long long counting = 0;
  for (int b = t; b < n_acc; b += FINISH_BLOCK) {
    pen += pen_partial[b];
    counting += cnt_partial[b];
  }
  for (int b = t; b < n_seed; b += FINISH_BLOCK) inside += term_partial[b];
  inside = spot_block_sum<FINISH_WAVES>(inside, wsum);
  pen = spot_block_sum<FINISH_WAVES>(pen, wsum);
  counting = spot_block_count<FINISH_WAVES>(counting, wcnt);
  if (t == 0) {
    const double e = inside + pen;
    const double terms = (double)(counting * fields);
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = counting > 0 ? e / terms : __builtin_nan("");
  }
}

static int spot_grid(int64_t n) {
  if (n <= 0) return 0;
  const int64_t want = (n + SPOT_RAYS_PER_BLOCK - 1) / SPOT_RAYS_PER_BLOCK;
  return (int)(want < SPOT_MAX_GRID ? want : SPOT_MAX_GRID);
}

static int spot_seed_grid(int64_t n) {
  if (n <= 0) return 0;
  const int64_t want = (n + BLOCK - 1) / BLOCK;
  return (int)(want < SPOT_SEED_MAX_GRID ? want : SPOT_SEED_MAX_GRID);
}

}  // namespace tfrt

using namespace tfrt;

extern "C" size_t tfrt_spot_error_workspace_bytes(int64_t n, int32_t n_groups);

// The accumulate and seed launches of every entry (`wt` null: unweighted).
template <typename T, int DIM>
static void spot_launch(const T* r, int64_t stride, int64_t n, const int32_t* mask,
                        const int32_t* group, const int32_t* perm, const SpotGrid& g,
                        const SpotWeights* wt, bool lds, int grid, int sgrid,
                        unsigned long long* accu, double* pen_partial, long long* cnt_partial,
                        double* term_partial, double* grad, int64_t grad_stride, hipStream_t st) {
  const long long* acc = reinterpret_cast<const long long*>(accu);
  if (wt != nullptr) {
    if (lds)
      hipLaunchKernelGGL((k_spot_accumulate_weighted<T, true, DIM>), dim3(grid), dim3(BLOCK),
                         (size_t)g.n_groups * 6 * sizeof(unsigned long long), st, r, stride, n,
                         mask, group, perm, g, *wt, accu, pen_partial, cnt_partial);
    else
      hipLaunchKernelGGL((k_spot_accumulate_weighted<T, false, DIM>), dim3(grid), dim3(BLOCK), 0,
                         st, r, stride, n, mask, group, perm, g, *wt, accu, pen_partial,
                         cnt_partial);
    hipLaunchKernelGGL((k_spot_seed_weighted<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride,
                       n, mask, group, perm, g, *wt, acc, grad, grad_stride, term_partial);
    return;
  }
  if (lds)
    hipLaunchKernelGGL((k_spot_accumulate<T, true, DIM>), dim3(grid), dim3(BLOCK),
                       (size_t)g.n_groups * 3 * sizeof(unsigned long long), st, r, stride, n, mask,
                       group, perm, g, accu, pen_partial, cnt_partial);
  else
    hipLaunchKernelGGL((k_spot_accumulate<T, false, DIM>), dim3(grid), dim3(BLOCK), 0, st, r,
                       stride, n, mask, group, perm, g, accu, pen_partial, cnt_partial);
  hipLaunchKernelGGL((k_spot_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride, n, mask,
                     group, perm, g, acc, grad, grad_stride, term_partial);
}

// Every entry behind its own checks of the rows / codes: `dim` 2 or 3, codes below 3 * dim.
// `weight` null: records of four int64 and n * 2^qbits < 2^62; else records of eight, `wbits`
// and n * 2^wbits * 2^ceil(qbits / 2) < 2^62.
static int spot_error_run(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                          int32_t dim, const int32_t* mask, int32_t row_x, int32_t row_y,
                          const int32_t* group, int64_t n_source, const int32_t* perm,
                          int32_t n_groups, double x0, double x1, double qsx, double y0, double y1,
                          double qsy, int32_t qbits, double oob_weight, double* grad,
                          int64_t grad_stride, double* error_out, int64_t* acc, int32_t variant,
                          void* workspace, size_t workspace_bytes, void* stream,
                          const double* weight = nullptr, int32_t wbits = 0) {
  const bool weighted = weight != nullptr;
  if (n < 0 || n > INT32_MAX || n_source < 0 || n_source > INT32_MAX || n_groups < 1 ||
      n_groups > SPOT_MAX_GROUPS || qbits < 1 || qbits > 52 || row_x == row_y || !group ||
      !error_out || !acc || !workspace || variant < 0 || variant > 2)
    return TFRT_E_BADARG;
  if (weighted) {
    // every sum stays below n * 2^wbits * 2^ceil(qbits / 2) < 2^62
    if (wbits < 1 || wbits > SPOT_MAX_WBITS) return TFRT_E_BADARG;
    if (n >= ((int64_t)1 << (62 - wbits - (qbits + 1) / 2))) return TFRT_E_BADARG;
  } else if (n >= ((int64_t)1 << (62 - qbits))) {
    return TFRT_E_BADARG;   // n * 2^qbits must stay below 2^62
  }
  if (!(x1 > x0) || !(qsx > 0.0) || !isfinite(qsx) || !(oob_weight >= 0.0) ||
      !isfinite(oob_weight) || !isfinite(x0) || !isfinite(x1))
    return TFRT_E_BADARG;
  if (row_y >= 0 && (!(y1 > y0) || !(qsy > 0.0) || !isfinite(qsy) || !isfinite(y0) || !isfinite(y1)))
    return TFRT_E_BADARG;
  if (n > 0 && (!rows || !grad || stride < n || grad_stride < n)) return TFRT_E_BADARG;
  if (!state_dtype_ok(state_dtype)) return TFRT_E_BADARG;
  const int lds_groups = weighted ? SPOT_WEIGHTED_LDS_GROUPS : SPOT_LDS_GROUPS;
  if (variant == 1 && n_groups > lds_groups) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_spot_error_workspace_bytes(n, n_groups)) return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= lds_groups);
  const bool dir = row_x >= 2 * dim || row_y >= 2 * dim;

  SpotGrid g;
  g.x0 = x0, g.x1 = x1, g.qsx = qsx, g.oob = oob_weight;
  g.y0 = row_y >= 0 ? y0 : 0.0, g.y1 = row_y >= 0 ? y1 : 0.0, g.qsy = row_y >= 0 ? qsy : 0.0;
  g.qmax = ldexp(1.0, qbits);
  g.n_source = n_source, g.n_groups = n_groups, g.row_x = row_x, g.row_y = row_y;
  SpotWeights w;
  w.weight = weight, w.one = ldexp(1.0, wbits), w.inv = ldexp(1.0, -wbits), w.h = qbits / 2;
  const SpotWeights* wt = weighted ? &w : nullptr;
  const int record = weighted ? 8 : 4;
  char* ws = static_cast<char*>(workspace);
  double* pen_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial =
      reinterpret_cast<long long*>(ws + align_up(SPOT_MAX_GRID * sizeof(double)));
  double* term_partial =
      reinterpret_cast<double*>(ws + 2 * align_up(SPOT_MAX_GRID * sizeof(double)));
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = spot_grid(n);
  const int sgrid = spot_seed_grid(n);

  hipLaunchKernelGGL(k_spot_clear, dim3(cdiv(record * (int64_t)n_groups, BLOCK)), dim3(BLOCK), 0,
                     st, accu, record * n_groups);
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const T* r = static_cast<const T*>(rows);
    if (grid > 0) {
      if (!dir)
        spot_launch<T, 0>(r, stride, n, mask, group, perm, g, wt, lds, grid, sgrid, accu,
                          pen_partial, cnt_partial, term_partial, grad, grad_stride, st);
      else if (dim == 3)
        spot_launch<T, 3>(r, stride, n, mask, group, perm, g, wt, lds, grid, sgrid, accu,
                          pen_partial, cnt_partial, term_partial, grad, grad_stride, st);
      else
        spot_launch<T, 2>(r, stride, n, mask, group, perm, g, wt, lds, grid, sgrid, accu,
                          pen_partial, cnt_partial, term_partial, grad, grad_stride, st);
    }
    hipLaunchKernelGGL(k_spot_finish, dim3(1), dim3(FINISH_BLOCK), 0, st, pen_partial, cnt_partial,
                       grid, term_partial, sgrid, row_y >= 0 ? 2 : 1, error_out);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

extern "C" {

size_t tfrt_spot_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS) return 0;
  return 2 * align_up(SPOT_MAX_GRID * sizeof(double)) +
         align_up(SPOT_SEED_MAX_GRID * sizeof(double));
}

int tfrt_spot_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                    const int32_t* mask, int32_t row_x, int32_t row_y, const int32_t* group,
                    int64_t n_source, const int32_t* perm, int32_t n_groups, double x0, double x1,
                    double qsx, double y0, double y1, double qsy, int32_t qbits,
                    double oob_weight, double* grad, int64_t grad_stride, double* error_out,
                    int64_t* acc, int32_t variant, void* workspace, size_t workspace_bytes,
                    void* stream) {
  if (row_x < 0 || row_x > 5 || row_y < -1 || row_y > 5) return TFRT_E_BADARG;
  return spot_error_run(rows, stride, n, state_dtype, 3, mask, row_x, row_y, group, n_source, perm,
                        n_groups, x0, x1, qsx, y0, y1, qsy, qbits, oob_weight, grad, grad_stride,
                        error_out, acc, variant, workspace, workspace_bytes, stream);
}

int tfrt_spot_error_fields(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                           int32_t dimension, const int32_t* mask, int32_t field_x,
                           int32_t field_y, const int32_t* group, int64_t n_source,
                           const int32_t* perm, int32_t n_groups, double x0, double x1, double qsx,
                           double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                           double* grad, int64_t grad_stride, double* error_out, int64_t* acc,
                           int32_t variant, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  return spot_error_run(rows, stride, n, state_dtype, dimension, mask, field_x, field_y, group,
                        n_source, perm, n_groups, x0, x1, qsx, y0, y1, qsy, qbits, oob_weight, grad,
                        grad_stride, error_out, acc, variant, workspace, workspace_bytes, stream);
}

size_t tfrt_spot_error_weighted_workspace_bytes(int64_t n, int32_t n_groups) {
  return tfrt_spot_error_workspace_bytes(n, n_groups);
}

int tfrt_spot_error_weighted(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                             int32_t dimension, const int32_t* mask, int32_t field_x,
                             int32_t field_y, const int32_t* group, const double* weight,
                             int32_t wbits, int64_t n_source, const int32_t* perm,
                             int32_t n_groups, double x0, double x1, double qsx, double y0,
                             double y1, double qsy, int32_t qbits, double oob_weight, double* grad,
                             int64_t grad_stride, double* error_out, int64_t* acc, int32_t variant,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension || !weight)
    return TFRT_E_BADARG;
  return spot_error_run(rows, stride, n, state_dtype, dimension, mask, field_x, field_y, group,
                        n_source, perm, n_groups, x0, x1, qsx, y0, y1, qsy, qbits, oob_weight, grad,
                        grad_stride, error_out, acc, variant, workspace, workspace_bytes, stream,
                        weight, wbits);
}

}  // extern "C"
