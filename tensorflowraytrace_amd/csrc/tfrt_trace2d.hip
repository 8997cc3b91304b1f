// tfrt 2-D hot path for MI355X (gfx950): rays x (segments + arcs), nearest hit, stable
// classification/compaction, angle-form Snell, pass loop and reverse sweep.
//
// Reference: OpticalSystem2D.intersect / _segment_intersection / _arc_intersection /
// _seg_or_arc / _get_arc_norm (tfrt/engine.py:523-866), process_projection_2D
// (engine.py:1544-1986), geometry.snells_law_2D (geometry.py:565-653).
//
// 2-D scenes have few primitives (M ~ 1..1e3) and many rays, so one pass is per-ray work
// streaming over an LDS-resident primitive table: lane = ray, every primitive is decided
// exactly in float64 (trace_math2d.h), running minima in registers.  In a mixed system each
// pass emits, per class, segment-hit rays first and arc-hit rays second (engine.py:1955-1981),
// hence 7 compaction bins: {active, finished, stopped} x {segment, arc} + dead.
#include "tfrt_common.h"
#include "goal_finish.h"
#include "trace_math2d.h"
#include "trace_filter2d.h"

namespace tfrt {

constexpr int TILE2 = 256;
constexpr int NBIN = 8;
constexpr int BIN_DEAD = 6;

template <typename T>
__device__ __forceinline__ void load_ray2(const T* rays, int64_t stride, int64_t i, double s[2],
                                          double e[2]) {
  s[0] = ldd(rays, i);
  s[1] = ldd(rays, stride + i);
  e[0] = ldd(rays, 2 * stride + i);
  e[1] = ldd(rays, 3 * stride + i);
}

template <typename T>
__device__ __forceinline__ void store_ray2(T* rays, int64_t stride, int64_t i, const double s[2],
                                           const double e[2]) {
  rays[i] = static_cast<T>(s[0]);
  rays[stride + i] = static_cast<T>(s[1]);
  rays[2 * stride + i] = static_cast<T>(e[0]);
  rays[3 * stride + i] = static_cast<T>(e[1]);
}

__device__ __forceinline__ int cat_cls(int cat) {
  return cat == CAT_OPTICAL ? CLS_ACTIVE : (cat == CAT_TARGET ? CLS_FINISHED : CLS_STOPPED);
}

// Nearest segment and nearest arc for ray (s, e); then engine.py:652-657 seg-vs-arc.
// Returns merged primitive index (segments first) or -1.
// STATE_ULP: unit roundoff of the ray-state storage type (0 for float64 state)
template <int STATE_BITS>
__device__ __forceinline__ int nearest2d(const double s[2], const double e[2],
                                         const double* __restrict__ seg, int Ms,
                                         const double* __restrict__ arc, int Ma, double ei,
                                         double es, double er, int last_prim, double* lds,
                                         bool active, double* out_u, double* out_aux) {
  double su = INFINITY, au = INFINITY, aang = 0.0;
  int sj = -1, aj = -1;
  for (int t0 = 0; t0 < Ms; t0 += TILE2) {
    const int nt = min(TILE2, Ms - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * 4; k += BLOCK) lds[k] = seg[(int64_t)t0 * 4 + k];
    __syncthreads();
    if (active) {
      for (int j = 0; j < nt; ++j) {
        if (t0 + j == last_prim) continue;  // the segment the ray starts on
        const Hit2 h = exact_segment(s, e, lds + 4 * j, ei, es, er);
        if (h.valid && h.ray_u < su) {
          su = h.ray_u;
          sj = t0 + j;
        }
      }
    }
  }
  for (int t0 = 0; t0 < Ma; t0 += TILE2) {
    const int nt = min(TILE2, Ma - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * 5; k += BLOCK) lds[k] = arc[(int64_t)t0 * 5 + k];
    __syncthreads();
    if (active) {
      for (int j = 0; j < nt; ++j) {
        double er_j = er;
        if (STATE_BITS < 53 && Ms + t0 + j == last_prim) {
          // a rounded (float32 / float16) start sits up to ~1 ulp off the arc it left: do not
          // let the near root (u ~ 0) count as a new hit
          const double dl = sqrt((e[0] - s[0]) * (e[0] - s[0]) + (e[1] - s[1]) * (e[1] - s[1]));
          const double mag = fabs(s[0]) + fabs(s[1]) + fabs(lds[5 * j + 4]);
          er_j = fmax(er, 64.0 * ldexp(1.0, -STATE_BITS) * mag / fmax(dl, 1e-300));
        }
        const Hit2 h = exact_arc(s, e, lds + 5 * j, ei, er_j);
        if (h.valid && h.ray_u < au) {
          au = h.ray_u;
          aj = t0 + j;
          aang = h.prim_u;
        }
      }
    }
  }
  // engine.py:652-657
  if (sj >= 0 && aj >= 0) {
    if (su < au) aj = -1; else sj = -1;
  }
  if (sj >= 0) {
    *out_u = su;
    *out_aux = 0.0;
    return sj;
  }
  if (aj >= 0) {
    *out_u = au;
    *out_aux = aang;
    return Ms + aj;
  }
  *out_u = INFINITY;
  *out_aux = 0.0;
  return -1;
}

// ---------------------------------------------------------------------------------------
// Filtered nearest hit (the trace kernels; the seams keep the plain loop above).  The filter's
// arithmetic -- the bounding circles of primitives and clusters, the ray's float32 state and
// the two predicates, with their derivation -- is trace_filter2d.h; here are the tiling, the LDS
// staging, the per-lane queues and the wave-uniform flushes around it.
constexpr int NC2 = TILE2 / G2;           // clusters per tile

template <int STATE_BITS>
__device__ __forceinline__ int nearest2d_filtered(const double s[2], const double e[2],
                                                  const double* __restrict__ seg, int Ms,
                                                  const double* __restrict__ arc, int Ma,
                                                  double ei, double es, double er, int last_prim,
                                                  double* lds, float4* filt, int32_t* queue,
                                                  float4* cfilt, float* crq15, uint8_t* cqueue,
                                                  bool active, double* out_u, double* out_aux) {
  // float32 state of this lane's ray (a lane without a valid ray never passes the test)
  const RayFilter2 rf = ray_filter2(s, e, ei, active);
  const int tid = threadIdx.x;
  int cnt = 0;
  double su = INFINITY, au = INFINITY, aang = 0.0;
  int sj = -1, aj = -1;

  // the clusters of the tile in `filt` (nt primitives, padded to whole clusters)
  auto build_clusters = [&](int nt) {
    const int nc = (nt + G2 - 1) / G2;
    for (int k = tid; k < nc; k += BLOCK) cfilt[k] = cluster_filter(filt + G2 * k, crq15 + k);
    return nc;
  };
  // this lane's clusters, ascending (always store, count only hits: no branch per test)
  auto collect = [&](int nc) {
    int cc = 0;
    for (int c = 0; c < nc; ++c) {
      cqueue[cc * BLOCK + tid] = (uint8_t)c;
      cc += touches_cluster(rf, cfilt[c], crq15[c]) ? 1 : 0;
    }
    return cc;
  };

  for (int t0 = 0; t0 < Ms; t0 += TILE2) {
    const int nt = min(TILE2, Ms - t0);
    const int nt8 = (nt + G2 - 1) & ~(G2 - 1);
    __syncthreads();
    for (int k = tid; k < nt * 4; k += BLOCK) lds[k] = seg[(int64_t)t0 * 4 + k];
    __syncthreads();
    for (int k = tid; k < nt8; k += BLOCK)
      filt[k] = k < nt ? filter_segment(lds + 4 * k, es) : filter_padding();
    __syncthreads();
    const int nc = build_clusters(nt);
    __syncthreads();
    auto flush = [&]() {
      for (int k = 0; k < cnt; ++k) {
        const int j = queue[k * BLOCK + tid];
        if (t0 + j == last_prim) continue;  // the segment the ray starts on
        const Hit2 h = exact_segment(s, e, lds + 4 * j, ei, es, er);
        if (h.valid && h.ray_u < su) {
          su = h.ray_u;
          sj = t0 + j;
        }
      }
      cnt = 0;
    };
    const int cc = collect(nc);
    for (int k = 0; __any(k < cc); ++k) {
      if (k < cc) {
        const int j0 = G2 * (int)cqueue[k * BLOCK + tid];
#pragma unroll
        for (int g = 0; g < G2; ++g) {
          queue[cnt * BLOCK + tid] = j0 + g;
          cnt += touches(rf, filt[j0 + g]) ? 1 : 0;
        }
      }
      if (__any(cnt > KQ2 - G2)) flush();
    }
    flush();  // the queue refers to this tile's LDS copy
  }
  for (int t0 = 0; t0 < Ma; t0 += TILE2) {
    const int nt = min(TILE2, Ma - t0);
    const int nt8 = (nt + G2 - 1) & ~(G2 - 1);
    __syncthreads();
    for (int k = tid; k < nt * 5; k += BLOCK) lds[k] = arc[(int64_t)t0 * 5 + k];
    __syncthreads();
    for (int k = tid; k < nt8; k += BLOCK)
      filt[k] = k < nt ? filter_arc(lds + 5 * k) : filter_padding();
    __syncthreads();
    const int nc = build_clusters(nt);
    __syncthreads();
    auto flush = [&]() {
      for (int k = 0; k < cnt; ++k) {
        const int j = queue[k * BLOCK + tid];
        double er_j = er;
        if (STATE_BITS < 53 && Ms + t0 + j == last_prim) {
          // a rounded (float32 / float16) start sits up to ~1 ulp off the arc it left: do not
          // let the near root (u ~ 0) count as a new hit
          const double dl = sqrt((e[0] - s[0]) * (e[0] - s[0]) + (e[1] - s[1]) * (e[1] - s[1]));
          const double mag = fabs(s[0]) + fabs(s[1]) + fabs(lds[5 * j + 4]);
          er_j = fmax(er, 64.0 * ldexp(1.0, -STATE_BITS) * mag / fmax(dl, 1e-300));
        }
        const Hit2 h = exact_arc_hit(s, e, lds + 5 * j, ei, er_j);
        if (h.valid && h.ray_u < au) {
          au = h.ray_u;
          aj = t0 + j;
          aang = h.prim_u;
        }
      }
      cnt = 0;
    };
    const int cc = collect(nc);
    for (int k = 0; __any(k < cc); ++k) {
      if (k < cc) {
        const int j0 = G2 * (int)cqueue[k * BLOCK + tid];
#pragma unroll
        for (int g = 0; g < G2; ++g) {
          queue[cnt * BLOCK + tid] = j0 + g;
          cnt += touches(rf, filt[j0 + g]) ? 1 : 0;
        }
      }
      if (__any(cnt > KQ2 - G2)) flush();
    }
    flush();
  }
  // engine.py:652-657
  if (sj >= 0 && aj >= 0) {
    if (su < au) aj = -1; else sj = -1;
  }
  if (sj >= 0) {
    *out_u = su;
    *out_aux = 0.0;
    return sj;
  }
  if (aj >= 0) {
    *out_u = au;
    *out_aux = aang;
    return Ms + aj;
  }
  *out_u = INFINITY;
  *out_aux = 0.0;
  return -1;
}

// 39.7 KB of LDS per workgroup leave room for 4 wavefronts per SIMD; the compiler's own choice is
// 152 VGPRs (3 wavefronts).  Pinned to 4 (128 VGPRs, 18 spilled to scratch in the exact tests):
// cfg5b forward + backward 2.93 -> 2.82 ms, results unchanged.
#ifndef TFRT_I2D_WAVES
#define TFRT_I2D_WAVES 4
#endif
#define TFRT_I2D_ATTR __attribute__((amdgpu_waves_per_eu(TFRT_I2D_WAVES, TFRT_I2D_WAVES)))
template <typename T>
__global__ __launch_bounds__(BLOCK) TFRT_I2D_ATTR void k_intersect2d(
    const T* __restrict__ rays, int64_t stride, const int32_t* __restrict__ n_ptr,
    const int32_t* __restrict__ last_prim, tfrt_scene2d sc, int32_t* __restrict__ rec_prim,
    double* __restrict__ rec_u, double* __restrict__ rec_aux, uint8_t* __restrict__ rec_bin,
    int32_t* __restrict__ blockcnt) {
  const int n = *n_ptr;
  const int base = blockIdx.x * BLOCK;
  if (base >= n) return;
  __shared__ double lds[TILE2 * 5];
  __shared__ float4 filt[TILE2];
  __shared__ int32_t queue[KQ2 * BLOCK];
  __shared__ float4 cfilt[NC2];
  __shared__ float crq15[NC2];
  __shared__ uint8_t cqueue[NC2 * BLOCK];
  __shared__ int wc[WAVES][NBIN];
  const int i = base + threadIdx.x;
  const bool active = i < n;
  double s[2] = {0, 0}, e[2] = {0, 0};
  if (active) load_ray2(rays, stride, i, s, e);
  const int lp = (active && last_prim) ? last_prim[i] : -1;
  const int Ms = (int)sc.n_segments, Ma = (int)sc.n_arcs;
  double u, aux;
  const int prim = nearest2d_filtered<(sizeof(T) == 8 ? 53 : (sizeof(T) == 4 ? 24 : 11))>(
      s, e, sc.seg, Ms, sc.arc, Ma, sc.intersect_epsilion, sc.size_epsilion,
      sc.ray_start_epsilion, lp, lds, filt, queue, cfilt, crq15, cqueue, active, &u, &aux);
  int bin = -1;
  if (active) {
    if (prim < 0) {
      bin = BIN_DEAD;
    } else if (prim < Ms) {
      bin = cat_cls(sc.seg_cat[prim]) * 2;
    } else {
      bin = cat_cls(sc.arc_cat[prim - Ms]) * 2 + 1;
    }
    rec_prim[i] = prim;
    rec_u[i] = u;
    rec_aux[i] = aux;
    rec_bin[i] = (uint8_t)bin;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NBIN; ++c) {
    const unsigned long long m = __ballot(bin == c);
    if (lane_id() == 0) wc[wave][c] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < NBIN) {
    int t = 0;
    for (int w = 0; w < WAVES; ++w) t += wc[w][threadIdx.x];
    blockcnt[blockIdx.x * NBIN + threadIdx.x] = t;
  }
}

// One block of 1024 threads scans every ray block's histogram (up to SCAN_GRID_MIN_ROWS rows;
// the offsets it writes are global, k_react2d gets no rowbase).
__global__ __launch_bounds__(1024) void k_scan2d_one(const int32_t* __restrict__ n_ptr,
                                                 const int32_t* __restrict__ blockcnt,
                                                 int32_t* __restrict__ blockoff,
                                                 int32_t* __restrict__ pass_counts,
                                                 int32_t* __restrict__ bin_counts,
                                                 int32_t* __restrict__ totals,
                                                 int32_t* __restrict__ n_next,
                                                 unsigned long long* __restrict__ n_tests,
                                                 int M) {
  const int n = *n_ptr;
  const int nblk = (n + BLOCK - 1) / BLOCK;
  __shared__ int total[NBIN];
  scan_rows_one<NBIN>(blockcnt, blockoff, nblk, total);
  if (threadIdx.x < NBIN) bin_counts[threadIdx.x] = total[threadIdx.x];
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    const int t = (c == CLS_DEAD) ? total[BIN_DEAD] : total[2 * c] + total[2 * c + 1];
    pass_counts[c] = t;
    pass_counts[4 + c] = totals[c];
    totals[c] += t;
    if (c == CLS_ACTIVE) *n_next = t;
  }
  if (threadIdx.x == 0) *n_tests += (unsigned long long)n * (unsigned long long)M;
}

// From SCAN_GRID_MIN_ROWS ray blocks on (its ticket and fences cost ~13 us whatever the size; the
// single block takes 54 us for the 15.6k rows of a 4M-ray pass, this 20 us):
constexpr int SCAN_GRID_MIN_ROWS = 8192;
__global__ __launch_bounds__(1024) void k_scan2d(const int32_t* __restrict__ n_ptr,
                                                 const int32_t* __restrict__ blockcnt,
                                                 int32_t* __restrict__ blockoff,
                                                 int32_t* __restrict__ rowtot,
                                                 int32_t* __restrict__ rowbase,
                                                 unsigned int* __restrict__ ticket,
                                                 int32_t* __restrict__ pass_counts,
                                                 int32_t* __restrict__ bin_counts,
                                                 int32_t* __restrict__ totals,
                                                 int32_t* __restrict__ n_next,
                                                 unsigned long long* __restrict__ n_tests,
                                                 int M) {
  // grid of 1024-thread workgroups, one ray block per thread (scan_rows_grid); the workgroup
  // that finishes last closes the pass
  const int n = *n_ptr;
  const int nblk = (n + BLOCK - 1) / BLOCK;
  __shared__ int total[NBIN];
  if (!scan_rows_grid<NBIN>(blockcnt, blockoff, nblk, rowtot, rowbase, ticket, total)) return;
  if (threadIdx.x < NBIN) bin_counts[threadIdx.x] = total[threadIdx.x];
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    const int t = (c == CLS_DEAD) ? total[BIN_DEAD] : total[2 * c] + total[2 * c + 1];
    pass_counts[c] = t;
    pass_counts[4 + c] = totals[c];
    totals[c] += t;
    if (c == CLS_ACTIVE) *n_next = t;
  }
  if (threadIdx.x == 0) *n_tests += (unsigned long long)n * (unsigned long long)M;
}

__device__ __forceinline__ void prim_indices(const tfrt_scene2d& sc, int prim, int rid,
                                             double* n_in, double* n_out) {
  const int Ms = (int)sc.n_segments;
  const bool is_arc = prim >= Ms;
  const int k = is_arc ? prim - Ms : prim;
  const int32_t* mi = is_arc ? sc.arc_mat_in : sc.seg_mat_in;
  const int32_t* mo = is_arc ? sc.arc_mat_out : sc.seg_mat_out;
  if (sc.n_table != nullptr && mi != nullptr && mo != nullptr) {
    *n_in = sc.n_table[(int64_t)mi[k] * sc.n_table_stride + rid];
    *n_out = sc.n_table[(int64_t)mo[k] * sc.n_table_stride + rid];
  } else {
    *n_in = (is_arc ? sc.arc_n_in : sc.seg_n_in)[k];
    *n_out = (is_arc ? sc.arc_n_out : sc.seg_n_out)[k];
  }
}

template <typename T>
__device__ __forceinline__ bool emit2(const tfrt_ray_out& o, int64_t slot, const double s[2],
                                      const double e[2], int rid, int face) {
  if (o.rays == nullptr) return true;
  if (slot >= o.capacity) return false;
  store_ray2(static_cast<T*>(o.rays), o.capacity, slot, s, e);
  if (o.ray_id) o.ray_id[slot] = rid;
  if (o.face) o.face[slot] = face;
  return true;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_react2d(
    const T* __restrict__ rays_in, int64_t stride_in, const int32_t* __restrict__ n_ptr,
    const int32_t* __restrict__ ray_id_in, const int32_t* __restrict__ rec_prim,
    const double* __restrict__ rec_u, const double* __restrict__ rec_aux,
    const uint8_t* __restrict__ rec_bin, const int32_t* __restrict__ blockoff,
    const int32_t* __restrict__ rowbase,
    const int32_t* __restrict__ pass_counts, const int32_t* __restrict__ bin_counts,
    tfrt_scene2d sc, double L, double dead_len, uint32_t flags, T* __restrict__ rays_out,
    int64_t stride_out, int32_t* __restrict__ ray_id_out, int32_t* __restrict__ last_prim_out,
    int32_t* __restrict__ rec_slot, tfrt_ray_out fin, tfrt_ray_out act, tfrt_ray_out stp,
    tfrt_ray_out dead, int32_t* __restrict__ err) {
  const int n = *n_ptr;
  const int base = blockIdx.x * BLOCK;
  if (base >= n) return;
  const int i = base + threadIdx.x;
  const int bin = (i < n) ? (int)rec_bin[i] : -1;
  __shared__ int wc[WAVES][NBIN];
  const int wave = threadIdx.x >> 6;
  int rank = 0;
#pragma unroll
  for (int c = 0; c < NBIN; ++c) {
    const unsigned long long m = __ballot(bin == c);
    if (bin == c) rank = rank_below(m);
    if (lane_id() == 0) wc[wave][c] = __popcll(m);
  }
  __syncthreads();
  if (i >= n) return;
  for (int w = 0; w < wave; ++w) rank += wc[w][bin];
  const int cls = (bin == BIN_DEAD) ? CLS_DEAD : (bin >> 1);
  const int kind = bin & 1;
  int slot = blockoff[blockIdx.x * NBIN + bin] +
             (rowbase != nullptr ? rowbase[(blockIdx.x >> 10) * NBIN + bin] : 0) + rank;
  if (cls != CLS_DEAD && kind == 1) slot += bin_counts[2 * cls];  // arcs after segments
  const int64_t gslot = (int64_t)pass_counts[4 + cls] + slot;

  double s[2], e[2];
  load_ray2(rays_in, stride_in, i, s, e);
  const int rid = ray_id_in ? ray_id_in[i] : i;
  const int prim = rec_prim[i];
  bool ok = true;
  if (cls == CLS_DEAD) {
    if (flags & TFRT_COMPILE_DEAD) {
      double e2[2] = {e[0], e[1]};
      if (dead_len != 0.0)
        for (int k = 0; k < 2; ++k) e2[k] = advance_between(s[k], dead_len, e[k]);
      ok = emit2<T>(dead, gslot, s, e2, rid, -1);
    }
    rec_slot[i] = (int32_t)gslot;
  } else {
    const double u = rec_u[i];
    const double h[2] = {s[0] + u * (e[0] - s[0]), s[1] + u * (e[1] - s[1])};
    if (cls == CLS_FINISHED) {
      if (flags & TFRT_COMPILE_FINISHED) ok = emit2<T>(fin, gslot, s, h, rid, prim);
      rec_slot[i] = (int32_t)gslot;
    } else if (cls == CLS_STOPPED) {
      if (flags & TFRT_COMPILE_STOPPED) ok = emit2<T>(stp, gslot, s, h, rid, prim);
      rec_slot[i] = (int32_t)gslot;
    } else {
      if (flags & TFRT_COMPILE_ACTIVE) ok = emit2<T>(act, gslot, s, h, rid, prim);
      const int Ms = (int)sc.n_segments;
      double norm;
      if (prim >= Ms) {
        norm = arc_norm(sc.arc[(int64_t)(prim - Ms) * 5 + 4], rec_aux[i]);
      } else {
        norm = segment_norm(sc.seg + (int64_t)prim * 4);
      }
      double n_in, n_out;
      prim_indices(sc, prim, rid, &n_in, &n_out);
      const double a = snell2d_angle(s[0], s[1], h[0], h[1], norm, n_in, n_out);
      const double e2[2] = {advance(h[0], L, cos(a)), advance(h[1], L, sin(a))};
      store_ray2(rays_out, stride_out, slot, h, e2);
      ray_id_out[slot] = rid;
      last_prim_out[slot] = prim;
      rec_slot[i] = slot;
    }
  }
  if (!ok) atomicOr(err, 1);
}

__device__ __forceinline__ void add4(const double* g, int64_t cap, int64_t slot, double a[2],
                                     double b[2]) {
  if (g == nullptr) return;
  for (int k = 0; k < 2; ++k) {
    a[k] += g[k * cap + slot];
    b[k] += g[(2 + k) * cap + slot];
  }
}

// Index gradient of one link ("value" mode): adds gn = {d / d n_in, d / d n_out} into the link's
// primitive's rows of tfrt_scene2d.grad_{seg,arc}_n_{in,out} (those given).
__device__ __forceinline__ void add_index_grads(const tfrt_scene2d& sc, int prim, const double gn[2]) {
  const int Ms = (int)sc.n_segments;
  const bool is_arc = prim >= Ms;
  const int k = is_arc ? prim - Ms : prim;
  double* gi = is_arc ? sc.grad_arc_n_in : sc.grad_seg_n_in;
  double* go = is_arc ? sc.grad_arc_n_out : sc.grad_seg_n_out;
  if (gi != nullptr && gn[0] != 0.0) unsafeAtomicAdd(gi + k, gn[0]);
  if (go != nullptr && gn[1] != 0.0) unsafeAtomicAdd(go + k, gn[1]);
}

// ---- ordered (deterministic) accumulation: tfrt_scene2d.deterministic
// The 3-D rule (tfrt_trace3d.hip, k_face_accumulate_fixed) carried over to every 2-D sweep, with
// one scale per output entry instead of one per pass.  A sweep runs twice: ORD_MAX only reduces
// the largest finite |term| of every entry (integer atomicMax on the bit pattern), ORD_ACC rounds
// each term to round(term * scale) in 64 bits -- scale = 2^(bits - e), the entry's largest term
// = f 2^e, f in [0.5, 1) -- and sums those integers (in the wavefront, then with integer
// atomics): exact, hence independent of the order and of which rays share a wavefront.  A
// non-finite term flags its entry instead.  k_fixed_finish2 then adds sum / scale (NaN where
// flagged) into the outputs in entry order and clears the accumulators.
//
// Headroom: every term is at most 2^bits after rounding, and an entry receives at most `terms`
// of them (rays per launch x passes per launch), so bits = min(40, 62 - ceil(log2 terms)) keeps
// every sum below 2^62 (fixed_bits2).  40 bits (2^-40 of the entry's largest term) up to 2^22
// terms per entry, one bit less for every doubling beyond.
//
// Entries (6 Ms + 7 Ma): grad_seg (Ms,4), grad_arc (Ma,5), then grad_seg_n_in, grad_seg_n_out,
// grad_arc_n_in, grad_arc_n_out.
constexpr int ORD_NONE = 0, ORD_MAX = 1, ORD_ACC = 2;
constexpr int FIXED_BITS2 = 40;

struct Fixed2 {
  unsigned long long* maxbits;  // per entry: bit pattern of the largest finite |term|
  unsigned long long* acc;      // per entry: two's complement sum of the rounded terms
  uint8_t* flag;                // per entry: a non-finite term was seen
  int bits;
};

static int fixed_bits2(int64_t terms) {
  int lg = 0;
  while (lg < 62 && (int64_t(1) << lg) < terms) ++lg;
  return min(FIXED_BITS2, 62 - lg);
}

__device__ __forceinline__ double fixed_scale2(unsigned long long maxbits, int bits) {
  if (maxbits == 0ull) return 0.0;
  int e;
  (void)frexp(__longlong_as_double((long long)maxbits), &e);
  // (an entry whose largest term lies below 2^-960 would need a scale beyond the float64 range:
  // its terms round to zero)
  int shift = bits - e;
  if (shift > 1000) shift = 1000;
  return ldexp(1.0, shift);
}

__device__ __forceinline__ int64_t geo_entry2(int prim, int q, int Ms) {
  return prim < Ms ? 4 * (int64_t)prim + q : 4 * (int64_t)Ms + 5 * (int64_t)(prim - Ms) + q;
}

// q = 0: d / d n_in, 1: d / d n_out
__device__ __forceinline__ int64_t index_entry2(int prim, int q, int Ms, int Ma) {
  const int64_t base = 4 * (int64_t)Ms + 5 * (int64_t)Ma;
  return prim < Ms ? base + (q ? Ms : 0) + prim
                   : base + 2 * (int64_t)Ms + (q ? Ma : 0) + (prim - Ms);
}

// One lane's term x of entry `at`.
template <int ORD>
__device__ __forceinline__ void fixed_term(const Fixed2& fx, int64_t at, double x) {
  const double a = fabs(x);
  if (ORD == ORD_MAX) {
    // non-negative doubles order like their bit patterns; NaN compares false
    if (a > 0.0 && a < INFINITY) atomicMax(fx.maxbits + at, (unsigned long long)__double_as_longlong(a));
  } else if (!(a < INFINITY)) {
    fx.flag[at] = 1;
  } else {
    const long long q = llrint(x * fixed_scale2(fx.maxbits[at], fx.bits));
    if (q != 0) atomicAdd(fx.acc + at, (unsigned long long)q);  // two's complement
  }
}

__global__ __launch_bounds__(BLOCK) void k_fixed_finish2(Fixed2 fx, int Ms, int Ma,
                                                         double* __restrict__ g_seg,
                                                         double* __restrict__ g_arc,
                                                         tfrt_scene2d sc) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const int64_t s4 = 4 * (int64_t)Ms, a5 = 5 * (int64_t)Ma;
  if (i >= s4 + a5 + 2 * (int64_t)(Ms + Ma)) return;
  double* out;
  if (i < s4) {
    out = g_seg ? g_seg + i : nullptr;
  } else if (i < s4 + a5) {
    out = g_arc ? g_arc + (i - s4) : nullptr;
  } else {
    int64_t j = i - s4 - a5;
    double* g;
    if (j < Ms) {
      g = sc.grad_seg_n_in;
    } else if (j < 2 * (int64_t)Ms) {
      g = sc.grad_seg_n_out;
      j -= Ms;
    } else if (j < 2 * (int64_t)Ms + Ma) {
      g = sc.grad_arc_n_in;
      j -= 2 * (int64_t)Ms;
    } else {
      g = sc.grad_arc_n_out;
      j -= 2 * (int64_t)Ms + Ma;
    }
    out = g ? g + j : nullptr;
  }
  const long long q = (long long)fx.acc[i];
  if (out != nullptr) {
    if (fx.flag[i] != 0) *out = __builtin_nan("");
    else if (q != 0) *out += (double)q / fixed_scale2(fx.maxbits[i], fx.bits);
  }
  fx.acc[i] = 0ull;
  fx.flag[i] = 0;
  fx.maxbits[i] = 0ull;
}

// GN: the index gradients are asked for (index_grads2d(sc)); false compiles none of their terms.
// ORD: ORD_NONE float64 atomics; ORD_MAX / ORD_ACC the two launches of the ordered sum (ORD_MAX
// writes no ray gradient).
template <typename T, bool GN, int ORD = ORD_NONE>
__global__ __launch_bounds__(BLOCK) void k_backward2d(
    const T* __restrict__ rays_in, int64_t stride_in, const int32_t* __restrict__ n_ptr,
    const int32_t* __restrict__ ray_id_in, const int32_t* __restrict__ rec_prim,
    const double* __restrict__ rec_u, const uint8_t* __restrict__ rec_bin,
    const int32_t* __restrict__ rec_slot, const int32_t* __restrict__ pass_counts,
    tfrt_scene2d sc, double L, double dead_len, const double* __restrict__ g_child,
    int64_t child_stride, const double* __restrict__ g_fin, int64_t cap_fin,
    const double* __restrict__ g_act, int64_t cap_act, const double* __restrict__ g_stp,
    int64_t cap_stp, const double* __restrict__ g_dead, int64_t cap_dead,
    double* __restrict__ g_out, int64_t out_stride, double* __restrict__ g_seg,
    double* __restrict__ g_arc, Fixed2 fx) {
  const int n = *n_ptr;
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const int bin = rec_bin[i];
  const int cls = (bin == BIN_DEAD) ? CLS_DEAD : (bin >> 1);
  const int slot = rec_slot[i];
  double s[2], e[2];
  load_ray2(rays_in, stride_in, i, s, e);
  double gs[2] = {0, 0}, ge[2] = {0, 0};
  if (cls == CLS_DEAD) {
    if (g_dead != nullptr) {
      double a[2] = {0, 0}, b[2] = {0, 0};
      add4(g_dead, cap_dead, slot, a, b);
      const double dl = (dead_len != 0.0) ? dead_len : 1.0;
      for (int k = 0; k < 2; ++k) {
        gs[k] = a[k] + (1.0 - dl) * b[k];
        ge[k] = dl * b[k];
      }
    }
  } else {
    double g_s[2] = {0, 0}, g_h[2] = {0, 0}, g_ce[2] = {0, 0};
    bool has_child = false;
    if (cls == CLS_FINISHED) {
      add4(g_fin, cap_fin, slot, g_s, g_h);
    } else if (cls == CLS_STOPPED) {
      add4(g_stp, cap_stp, slot, g_s, g_h);
    } else {
      // active-history slot: base + (arcs after segments) handled at forward time: the
      // child slot IS the within-pass active slot
      add4(g_act, cap_act, (int64_t)pass_counts[4 + CLS_ACTIVE] + slot, g_s, g_h);
      if (g_child != nullptr) {
        has_child = true;
        add4(g_child, child_stride, slot, g_h, g_ce);
      }
    }
    bool nz = has_child;
    for (int k = 0; k < 2; ++k) nz = nz || g_s[k] != 0.0 || g_h[k] != 0.0;
    if (nz) {
      const int prim = rec_prim[i];
      const int Ms = (int)sc.n_segments;
      const bool is_arc = prim >= Ms;
      const int rid = ray_id_in ? ray_id_in[i] : i;
      double n_in = 1.0, n_out = 1.0, gp[5];
      if (has_child) prim_indices(sc, prim, rid, &n_in, &n_out);
      const double* pp = is_arc ? sc.arc + (int64_t)(prim - Ms) * 5 : sc.seg + (int64_t)prim * 4;
      double gn[2];
      adjoint2d(s, e, pp, is_arc, rec_u[i], has_child, n_in, n_out, L, g_s, g_h, g_ce, gs, ge, gp,
                sc.finite_tir_gradient != 0, GN ? gn : nullptr);
      if constexpr (ORD == ORD_NONE) {
        if (GN && has_child) add_index_grads(sc, prim, gn);
        if (is_arc) {
          if (g_arc != nullptr)
            for (int q = 0; q < 5; ++q)
              if (gp[q] != 0.0) unsafeAtomicAdd(g_arc + (int64_t)(prim - Ms) * 5 + q, gp[q]);
        } else if (g_seg != nullptr) {
          for (int q = 0; q < 4; ++q)
            if (gp[q] != 0.0) unsafeAtomicAdd(g_seg + (int64_t)prim * 4 + q, gp[q]);
        }
      } else {
        const int Ma = (int)sc.n_arcs;
        if (GN && has_child) {
          if ((is_arc ? sc.grad_arc_n_in : sc.grad_seg_n_in) != nullptr)
            fixed_term<ORD>(fx, index_entry2(prim, 0, Ms, Ma), gn[0]);
          if ((is_arc ? sc.grad_arc_n_out : sc.grad_seg_n_out) != nullptr)
            fixed_term<ORD>(fx, index_entry2(prim, 1, Ms, Ma), gn[1]);
        }
        if (is_arc ? g_arc != nullptr : g_seg != nullptr)
          for (int q = 0; q < (is_arc ? 5 : 4); ++q) fixed_term<ORD>(fx, geo_entry2(prim, q, Ms), gp[q]);
      }
    }
  }
  if (ORD == ORD_MAX) return;
  for (int k = 0; k < 2; ++k) {
    g_out[k * out_stride + i] = gs[k];
    g_out[(2 + k) * out_stride + i] = ge[k];
  }
}

// seam kernels: one primitive kind, nearest per ray
template <typename T, bool ARC>
__global__ __launch_bounds__(BLOCK) void k_seam2d(const T* __restrict__ rays, int64_t stride, int n,
                                                  const double* __restrict__ prim, int M, double ei,
                                                  double es, double er, double* x, double* y,
                                                  uint8_t* valid, double* ray_u, double* prim_u,
                                                  int32_t* gather) {
  __shared__ double lds[TILE2 * 5];
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  const bool active = i < n;
  double s[2] = {0, 0}, e[2] = {0, 0};
  if (active) load_ray2(rays, stride, i, s, e);
  constexpr int W = ARC ? 5 : 4;
  Hit2 best;
  best.valid = false;
  best.ray_u = INFINITY;
  best.prim_u = best.x = best.y = 0.0;
  int bj = 0;
  Hit2 first = best;
  for (int t0 = 0; t0 < M; t0 += TILE2) {
    const int nt = min(TILE2, M - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * W; k += BLOCK) lds[k] = prim[(int64_t)t0 * W + k];
    __syncthreads();
    if (active) {
      for (int j = 0; j < nt; ++j) {
        Hit2 h;
        if (ARC) h = exact_arc(s, e, lds + 5 * j, ei, er);
        else h = exact_segment(s, e, lds + 4 * j, ei, es, er);
        if (t0 + j == 0) first = h;
        if (h.valid && h.ray_u < best.ray_u) {
          best = h;
          bj = t0 + j;
        }
      }
    }
  }
  if (!active) return;
  const Hit2& o = best.valid ? best : first;  // argmin of an all-sentinel column is 0
  x[i] = o.x;
  y[i] = o.y;
  valid[i] = best.valid;
  ray_u[i] = best.valid ? best.ray_u : INFINITY;
  prim_u[i] = o.prim_u;
  gather[i] = best.valid ? bj : 0;
}

struct Layout2 {
  size_t nrays, blockcnt, blockoff, rowtot, rowbase, ticket, bincnt, rays, rayid, lastprim, rec_prim, rec_slot, rec_u,
      rec_aux, rec_bin, gbuf, total;
  // ordered reverse sweeps (tfrt_scene2d.deterministic) only: per-entry accumulators behind the
  // rest, O(primitives); total_ordered covers them
  size_t fix_max, fix_acc, fix_flag, total_ordered;
  int nblk;
};

// (Ms, Ma size only the ordered sweeps' region at the end: every other offset is the same
// whatever they are)
static Layout2 make_layout2(int64_t N, int P, int dtype, int64_t Ms = 0, int64_t Ma = 0) {
  Layout2 L;
  const size_t esz = state_bytes(dtype);
  const size_t n = N > 0 ? N : 1;
  L.nblk = cdiv(n, BLOCK);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o = align_up(o + bytes);
    return at;
  };
  L.nrays = take((P + 2) * sizeof(int32_t));
  L.blockcnt = take((size_t)L.nblk * NBIN * sizeof(int32_t));
  L.blockoff = take((size_t)L.nblk * NBIN * sizeof(int32_t));
  L.rowtot = take((size_t)cdiv(L.nblk, 1024) * NBIN * sizeof(int32_t));
  L.rowbase = take((size_t)cdiv(L.nblk, 1024) * NBIN * sizeof(int32_t));
  L.ticket = take(sizeof(unsigned int));
  L.bincnt = take((size_t)(P + 1) * NBIN * sizeof(int32_t));
  L.rays = take((size_t)P * 4 * n * esz);
  L.rayid = take((size_t)P * n * sizeof(int32_t));
  L.lastprim = take((size_t)P * n * sizeof(int32_t));
  L.rec_prim = take((size_t)P * n * sizeof(int32_t));
  L.rec_slot = take((size_t)P * n * sizeof(int32_t));
  L.rec_u = take((size_t)P * n * sizeof(double));
  L.rec_aux = take((size_t)P * n * sizeof(double));
  L.rec_bin = take((size_t)P * n);
  L.gbuf = take((size_t)2 * 4 * n * sizeof(double));
  L.total = o;
  const size_t E = (size_t)(6 * Ms + 7 * Ma);
  L.fix_max = take(E * sizeof(unsigned long long));
  L.fix_acc = take(E * sizeof(unsigned long long));
  L.fix_flag = take(E);
  L.total_ordered = o;
  return L;
}

// Typed view of the record a 2-D trace leaves in its workspace (Layout2), per-pass rows `n` slots
// apart: the forward writes it through a Tape2<T>, the sweeps and tfrt_trace2d_rows read it
// through a Tape2<const T>.
template <typename T>
struct Tape2 {
  template <typename U>
  using as = std::conditional_t<std::is_const_v<T>, const U, U>;
  using E = std::remove_const_t<T>;
  as<char>* ws;
  const Layout2& lay;
  size_t n;
  template <typename U>
  as<U>* at(size_t offset) const { return reinterpret_cast<as<U>*>(ws + offset); }
  Tape2(as<void>* workspace, const Layout2& layout, int64_t N)
      : ws(static_cast<as<char>*>(workspace)), lay(layout), n(N > 0 ? N : 1) {}

  as<int32_t>* nrays = at<int32_t>(lay.nrays);   // rays entering pass 1..P, and P + 1
  // pass p's output rays, their ids and last primitives; its records
  T* rays_out(int p) const { return at<E>(lay.rays) + (size_t)p * 4 * n; }
  as<int32_t>* ids(int p) const { return at<int32_t>(lay.rayid) + (size_t)p * n; }
  as<int32_t>* last(int p) const { return at<int32_t>(lay.lastprim) + (size_t)p * n; }
  as<int32_t>* rec_prim(int p) const { return at<int32_t>(lay.rec_prim) + (size_t)p * n; }
  as<int32_t>* rec_slot(int p) const { return at<int32_t>(lay.rec_slot) + (size_t)p * n; }
  as<double>* rec_u(int p) const { return at<double>(lay.rec_u) + (size_t)p * n; }
  as<double>* rec_aux(int p) const { return at<double>(lay.rec_aux) + (size_t)p * n; }
  as<uint8_t>* rec_bin(int p) const { return at<uint8_t>(lay.rec_bin) + (size_t)p * n; }
  PassIn<E> input(int p, const void* src, int64_t src_stride) const {
    if (p == 0) return {static_cast<const E*>(src), src_stride, nullptr, nullptr};
    return {rays_out(p - 1), (int64_t)n, ids(p - 1), last(p - 1)};
  }
};

// The ordered sweeps' accumulators in the workspace, cleared (inside the call, so that a captured
// sequence replays correctly); bits for at most `terms` terms per entry.
static Fixed2 fixed_region2(const Layout2& lay, char* ws, int64_t terms, hipStream_t st) {
  Fixed2 fx;
  fx.maxbits = reinterpret_cast<unsigned long long*>(ws + lay.fix_max);
  fx.acc = reinterpret_cast<unsigned long long*>(ws + lay.fix_acc);
  fx.flag = reinterpret_cast<uint8_t*>(ws + lay.fix_flag);
  fx.bits = fixed_bits2(terms > 0 ? terms : 1);
  (void)hipMemsetAsync(ws + lay.fix_max, 0, lay.total_ordered - lay.fix_max, st);
  return fx;
}

static bool scene2_ok(const tfrt_scene2d* sc) {
  if (!sc || sc->n_segments < 0 || sc->n_arcs < 0) return false;
  if (sc->n_segments > 0 && (!sc->seg || !sc->seg_cat)) return false;
  if (sc->n_arcs > 0 && (!sc->arc || !sc->arc_cat)) return false;
  if (sc->n_segments + sc->n_arcs >= (1ll << 30)) return false;
  const bool table = sc->n_table != nullptr;
  if (sc->n_segments > 0 && !((table && sc->seg_mat_in && sc->seg_mat_out) ||
                              (sc->seg_n_in && sc->seg_n_out)))
    return false;
  if (sc->n_arcs > 0 && !((table && sc->arc_mat_in && sc->arc_mat_out) ||
                          (sc->arc_n_in && sc->arc_n_out)))
    return false;
  return true;
}

// The reverse sweeps compile the index terms in only when a gradient of the per-primitive indices
// is asked for, in "value" mode (n_table NULL): tfrt_scene2d.grad_{seg,arc}_n_{in,out}.
static bool index_grads2d(const tfrt_scene2d* sc) {
  if (sc->n_table != nullptr) return false;
  return (sc->n_segments > 0 && (sc->grad_seg_n_in || sc->grad_seg_n_out)) ||
         (sc->n_arcs > 0 && (sc->grad_arc_n_in || sc->grad_arc_n_out));
}

// What the 2-D reverse sweeps hand on (tfrt_trace2d_backward: the class gradients; the goal and
// rows sweeps: the forward's finished block, their seed apart).
struct SweepCall2 {
  const void* src;
  int64_t src_stride, N;
  const tfrt_scene2d* sc;
  double L, dead_len;
  int P, dtype;
  const int32_t* counts;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t st;
  // what differs between them, set by name (null / 0 where an entry has none)
  const double *g_fin, *g_act, *g_stp, *g_dead;
  int64_t cap_fin, cap_act, cap_stp, cap_dead;
  double *g_seg, *g_arc, *g_src;
  const tfrt_ray_out* fin;   // goal and rows sweeps only
};

template <typename T>
static int trace2d_forward_t(const TraceCall<tfrt_scene2d>& c) {
  const tfrt_scene2d* sc = c.sc;
  const int64_t N = c.N;
  const int P = c.P;
  hipStream_t st = c.st;
  const Layout2 lay = make_layout2(N, P, c.dtype);
  if (c.workspace_bytes < lay.total) return TFRT_E_WORKSPACE;
  const Tape2<T> tape(c.workspace, lay, N);
  // (the forward's own regions: nobody else reads them)
  char* ws = static_cast<char*>(c.workspace);
  int32_t* blockcnt = reinterpret_cast<int32_t*>(ws + lay.blockcnt);
  int32_t* blockoff = reinterpret_cast<int32_t*>(ws + lay.blockoff);
  int32_t* rowtot = reinterpret_cast<int32_t*>(ws + lay.rowtot);
  int32_t* rowbase = reinterpret_cast<int32_t*>(ws + lay.rowbase);
  unsigned int* ticket = reinterpret_cast<unsigned int*>(ws + lay.ticket);
  int32_t* bincnt_all = reinterpret_cast<int32_t*>(ws + lay.bincnt);
  int32_t* nrays = tape.nrays;
  int32_t* tail = c.counts + (size_t)P * TFRT_COUNTS_PER_PASS;
  const int64_t n = (int64_t)tape.n;
  const int M = (int)(sc->n_segments + sc->n_arcs);
  hipLaunchKernelGGL(k_init<>, dim3(1), dim3(64), 0, st, nrays, (int)N, tail, ticket);
  const tfrt_ray_out none = {nullptr, nullptr, nullptr, 0};
  for (int p = 0; p < P; ++p) {
    const PassIn<T> in = tape.input(p, c.src, c.src_stride);
    int32_t* pass_counts = c.counts + (size_t)p * TFRT_COUNTS_PER_PASS;
    int32_t* bincnt = bincnt_all + (size_t)p * NBIN;
    hipLaunchKernelGGL((k_intersect2d<T>), dim3(lay.nblk), dim3(BLOCK), 0, st, in.rays, in.stride,
                       nrays + p, in.last, *sc, tape.rec_prim(p), tape.rec_u(p), tape.rec_aux(p),
                       tape.rec_bin(p), blockcnt);
    const bool grid_scan = lay.nblk >= SCAN_GRID_MIN_ROWS;
    if (grid_scan)
      hipLaunchKernelGGL(k_scan2d, dim3(cdiv(lay.nblk, 1024)), dim3(1024), 0, st, nrays + p,
                         blockcnt, blockoff, rowtot, rowbase, ticket, pass_counts,
                         bincnt, tail, nrays + p + 1,
                         reinterpret_cast<unsigned long long*>(tail + 4), M);
    else
      hipLaunchKernelGGL(k_scan2d_one, dim3(1), dim3(1024), 0, st, nrays + p, blockcnt,
                         blockoff, pass_counts, bincnt, tail, nrays + p + 1,
                         reinterpret_cast<unsigned long long*>(tail + 4), M);
    hipLaunchKernelGGL((k_react2d<T>), dim3(lay.nblk), dim3(BLOCK), 0, st, in.rays, in.stride,
                       nrays + p, in.ids, tape.rec_prim(p), tape.rec_u(p), tape.rec_aux(p),
                       tape.rec_bin(p), blockoff,
                       grid_scan ? rowbase : static_cast<int32_t*>(nullptr), pass_counts, bincnt,
                       *sc, c.L, c.dead_len, c.flags, tape.rays_out(p), n, tape.ids(p),
                       tape.last(p), tape.rec_slot(p), c.fin ? *c.fin : none,
                       c.act ? *c.act : none, c.stp ? *c.stp : none, c.dead ? *c.dead : none,
                       tail + 6);
  }
  if (c.unfinished != nullptr && P > 0) {
    hipLaunchKernelGGL((k_copy_rays<T, 4>), dim3(lay.nblk), dim3(BLOCK), 0, st, tape.rays_out(P - 1),
                       n, tape.ids(P - 1), nrays + P, static_cast<T*>(c.unfinished), (int64_t)N,
                       c.unfinished_id);
  }
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

template <typename T>
static int trace2d_backward_t(const SweepCall2& c) {
  const tfrt_scene2d* sc = c.sc;
  const int64_t N = c.N;
  const int P = c.P;
  double *g_seg = c.g_seg, *g_arc = c.g_arc;
  hipStream_t st = c.st;
  const int Ms = (int)sc->n_segments, Ma = (int)sc->n_arcs;
  const Layout2 lay = make_layout2(N, P, c.dtype, Ms, Ma);
  if (c.workspace_bytes < lay.total) return TFRT_E_WORKSPACE;
  const Tape2<const T> tape(c.workspace, lay, N);
  char* ws = static_cast<char*>(c.workspace);
  double* gbuf = reinterpret_cast<double*>(ws + lay.gbuf);   // (the sweep's own)
  const int64_t n = (int64_t)tape.n;
  const bool gn = index_grads2d(sc);
  // ordered: per pass ORD_MAX, ORD_ACC and k_fixed_finish2 (the pass's sums are added into the
  // outputs pass by pass, last pass first); at most one term per ray and entry in a pass
  const bool ordered = sc->deterministic != 0 && Ms + Ma > 0 && (g_seg || g_arc || gn);
  Fixed2 fx = {nullptr, nullptr, nullptr, 0};
  if (ordered) {
    if (c.workspace_bytes < lay.total_ordered) return TFRT_E_WORKSPACE;
    fx = fixed_region2(lay, ws, N, st);
  }
  for (int p = P - 1; p >= 0; --p) {
    const PassIn<T> in = tape.input(p, c.src, c.src_stride);
    const double* g_child = (p == P - 1) ? nullptr : gbuf + (size_t)((p + 1) & 1) * 4 * n;
    double* g_out = (p == 0 && c.g_src != nullptr) ? c.g_src : gbuf + (size_t)(p & 1) * 4 * n;
    const int64_t out_stride = (p == 0 && c.g_src != nullptr) ? N : n;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(lay.nblk), dim3(BLOCK), 0, st, in.rays, in.stride,
                         tape.nrays + p, in.ids, tape.rec_prim(p), tape.rec_u(p), tape.rec_bin(p),
                         tape.rec_slot(p), c.counts + (size_t)p * TFRT_COUNTS_PER_PASS, *sc, c.L,
                         c.dead_len, g_child, n, c.g_fin, c.cap_fin, c.g_act, c.cap_act, c.g_stp,
                         c.cap_stp, c.g_dead, c.cap_dead, g_out, out_stride, g_seg, g_arc, fx);
    };
    if (!ordered) {
      if (gn) launch(k_backward2d<T, true>);
      else launch(k_backward2d<T, false>);
      continue;
    }
    if (gn) {
      launch(k_backward2d<T, true, ORD_MAX>);
      launch(k_backward2d<T, true, ORD_ACC>);
    } else {
      launch(k_backward2d<T, false, ORD_MAX>);
      launch(k_backward2d<T, false, ORD_ACC>);
    }
    hipLaunchKernelGGL(k_fixed_finish2, dim3(cdiv(6 * (int64_t)Ms + 7 * (int64_t)Ma, BLOCK)),
                       dim3(BLOCK), 0, st, fx, Ms, Ma, g_seg, g_arc, *sc);
  }
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

// ---------------------------------------------------------------------------------------
// The goal error folded into the reverse sweep (tfrt_trace2d_backward_goal).
//
// A 2-D trace keeps its rays in natural order, so lane i IS source ray i (and goal row i) and
// walks its chain forward through the tape: an ACTIVE ray's rec_slot is its child's index in
// the next pass's input, every other class's rec_slot is the global slot in that class's block
// (k_react2d).  A chain that finishes reads its output row at that slot, forms r = out - goal,
// seeds 2 r and runs the chain's adjoint from the last link back to pass 0 -- the very calls of
// adjoint2d k_backward2d makes for this ray, link by link, including the parent links of chains
// that do not finish (their zero child gradient still carries the NaN of a totally reflected
// link, geometry.py:640-646, as it does there).  The chain's indices live in an LDS ring of
// CHAIN2 links per lane; a chain longer than that re-walks the tape from pass 0 for every
// further CHAIN2 links (one code path for any max_passes).
//
// The links of a wave are processed in lockstep (link k of every lane together), so that the
// primitive gradients can be combined inside the wave before the global atomics: in a scene of
// few primitives (dev/optimize_single_arc.py: one arc) every lane adds into the same row.
//
// The seed is a template parameter of the kernel: SeedGoal2 forms it from the goal (and sums the
// error), SeedRows2 reads it from a buffer of row gradients (tfrt_trace2d_backward_rows: the
// gradient of any row-wise error over the columns tfrt_trace2d_rows made).
constexpr int CHAIN2 = 16;

struct ChainGoal2 {
  GoalFields gf;
  const double* goal;
  int64_t goal_stride, goal_ray_stride;
};

// Walks source ray i's chain forward through the tape.  keep(p, idx) is told every link's index
// into its pass's input; returns the last link's pass (-1: P == 0) and leaves how the chain ended
// in end_cls / end_slot (-1 / 0 while it is still active after pass P-1) and that last link's
// index in `last`.
template <typename Keep>
__device__ __forceinline__ int walk_chain2(int i, const uint8_t* __restrict__ rec_bin,
                                           const int32_t* __restrict__ rec_slot, int64_t n, int P,
                                           Keep keep, int& end_cls, int& end_slot, int& last) {
  int top = -1;
  int idx = i;
  for (int p = 0; p < P; ++p) {
    keep(p, idx);
    top = p;
    last = idx;
    const int bin = rec_bin[(size_t)p * n + idx];
    const int slot = rec_slot[(size_t)p * n + idx];
    const int cls = (bin == BIN_DEAD) ? CLS_DEAD : (bin >> 1);
    if (cls != CLS_ACTIVE) {
      end_cls = cls;
      end_slot = slot;
      break;
    }
    idx = slot;
  }
  return top;
}

// Per-wavefront partial sum of `acc`, lanes in a fixed butterfly order (called by all 64 lanes).
__device__ __forceinline__ void wave_partial(double acc, int N, double* __restrict__ partial) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
  const int64_t wave_g = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  if (lane_id() == 0 && wave_g * 64 < N) partial[wave_g] = acc;
}

// The goal residual: seeds 2 (out - goal) on the goal's rows and returns the squared residuals'
// sum; sum() leaves the wave's partial error sum.
struct SeedGoal2 {
  ChainGoal2 cg;
  double* partial;

  template <typename T>
  __device__ __forceinline__ double seed(const tfrt_ray_out& fin, int end_slot, int i,
                                         double sd[4]) const {
    // the reference's squared_difference and reduce_sum are separate ops: no contraction (the
    // adjoint's own arithmetic is compiled as in k_backward2d)
#pragma clang fp contract(off)
    double acc = 0.0;
    const T* out = static_cast<const T*>(fin.rays);
    for (int c = 0; c < cg.gf.n; ++c) {
      const int row = cg.gf.row[c];
      const double r = ldd(out, (int64_t)row * fin.capacity + end_slot) -
                       cg.goal[(int64_t)c * cg.goal_stride + (int64_t)i * cg.goal_ray_stride];
      sd[row] = 2.0 * r;
      acc += r * r;
    }
    return acc;
  }

  __device__ __forceinline__ void sum(double acc, int N) const { wave_partial(acc, N, partial); }
};

// Row gradients d error / d (x_start, y_start, x_end, y_end) of source ray i's column, rows
// `stride` apart (NULL: zero), and ray i's n_terms error terms, summed like SeedGoal2's.
struct SeedRows2 {
  const double* g;
  int64_t stride;
  const double* err;
  int64_t err_stride, err_ray_stride;
  int n_terms;
  double* partial;

  template <typename T>
  __device__ __forceinline__ double seed(const tfrt_ray_out&, int, int i, double sd[4]) const {
#pragma clang fp contract(off)
    if (g != nullptr)
      for (int r = 0; r < 4; ++r) sd[r] = g[(int64_t)r * stride + i];
    double acc = 0.0;
    for (int c = 0; c < n_terms; ++c) acc += err[(int64_t)c * err_stride + (int64_t)i * err_ray_stride];
    return acc;
  }

  __device__ __forceinline__ void sum(double acc, int N) const {
    wave_partial(acc, N, partial);
  }
};

// Adds the gradient rows of the lanes with `has` set into g_seg / g_arc: one atomic per entry
// and distinct primitive of the wave (a wave-wide sum over the lanes that share the primitive;
// a primitive only one lane touched is added by that lane directly).  Called by all 64 lanes.
__device__ __forceinline__ void add_prim_grads(bool has, int prim, const double gp[5], int Ms,
                                               double* __restrict__ g_seg,
                                               double* __restrict__ g_arc) {
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int key = __shfl(prim, leader, 64);
    const bool mine = has && prim == key;
    const unsigned long long grp = __ballot(mine);
    const bool is_arc = key >= Ms;
    double* row = is_arc ? (g_arc ? g_arc + (int64_t)(key - Ms) * 5 : nullptr)
                         : (g_seg ? g_seg + (int64_t)key * 4 : nullptr);
    if (row != nullptr) {
      // (adjoint2d leaves an arc's angle columns 2, 3 at zero: they only feed comparisons)
      constexpr int seg_q[4] = {0, 1, 2, 3};
      constexpr int arc_q[3] = {0, 1, 4};
      const int nq = is_arc ? 3 : 4;
      if (__popcll(grp) == 1) {
        if (mine)
          for (int k = 0; k < nq; ++k) {
            const int q = is_arc ? arc_q[k] : seg_q[k];
            if (gp[q] != 0.0) unsafeAtomicAdd(row + q, gp[q]);
          }
      } else {
        for (int k = 0; k < nq; ++k) {
          const int q = is_arc ? arc_q[k] : seg_q[k];
          double v = mine ? gp[q] : 0.0;
#pragma unroll
          for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
          if ((int)lane_id() == leader && v != 0.0) unsafeAtomicAdd(row + q, v);
        }
      }
    }
    has = has && !mine;
    todo &= ~grp;
  }
}

// add_prim_grads for the index gradients gn = {d / d n_in, d / d n_out} of the lanes with `has`
// set (tfrt_scene2d.grad_{seg,arc}_n_{in,out}, those given).  Called by all 64 lanes.
__device__ __forceinline__ void add_prim_index_grads(bool has, int prim, const double gn[2],
                                                     const tfrt_scene2d& sc) {
  const int Ms = (int)sc.n_segments;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int key = __shfl(prim, leader, 64);
    const bool mine = has && prim == key;
    const unsigned long long grp = __ballot(mine);
    const bool is_arc = key >= Ms;
    const int k = is_arc ? key - Ms : key;
    double* const rows[2] = {is_arc ? sc.grad_arc_n_in : sc.grad_seg_n_in,
                             is_arc ? sc.grad_arc_n_out : sc.grad_seg_n_out};
    const bool single = __popcll(grp) == 1;
    for (int q = 0; q < 2; ++q) {
      if (rows[q] == nullptr) continue;
      if (single) {
        if (mine && gn[q] != 0.0) unsafeAtomicAdd(rows[q] + k, gn[q]);
      } else {
        double v = mine ? gn[q] : 0.0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((int)lane_id() == leader && v != 0.0) unsafeAtomicAdd(rows[q] + k, v);
      }
    }
    has = has && !mine;
    todo &= ~grp;
  }
}

// The terms x of the lanes with `mine` set into entry `at` (wave-uniform), ORD_MAX or ORD_ACC:
// one atomic per entry and wavefront.  The rounded terms are summed as integers, so the result
// does not depend on which lanes share the wavefront.  Called by all 64 lanes.
template <int ORD>
__device__ __forceinline__ void fixed_group(const Fixed2& fx, int64_t at, bool mine, bool single,
                                            int leader, double x) {
  if (single) {
    if (mine) fixed_term<ORD>(fx, at, x);
    return;
  }
  const double a = fabs(x);
  if (ORD == ORD_MAX) {
    double m = (mine && a < INFINITY) ? a : 0.0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    if ((int)lane_id() == leader && m > 0.0)
      atomicMax(fx.maxbits + at, (unsigned long long)__double_as_longlong(m));
  } else {
    const double scale = fixed_scale2(fx.maxbits[at], fx.bits);
    unsigned long long q = 0ull;
    if (mine) {
      if (a < INFINITY) q = (unsigned long long)llrint(x * scale);
      else fx.flag[at] = 1;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) q += __shfl_xor(q, d, 64);  // (two's complement)
    if ((int)lane_id() == leader && q != 0ull) atomicAdd(fx.acc + at, q);
  }
}

// add_prim_grads + add_prim_index_grads of the ordered sweep.  Called by all 64 lanes.
template <int ORD, bool GN>
__device__ __forceinline__ void add_prim_grads_fixed(bool has, int prim, const double gp[5],
                                                     const double gn[2], const tfrt_scene2d& sc,
                                                     double* g_seg, double* g_arc,
                                                     const Fixed2& fx) {
  const int Ms = (int)sc.n_segments, Ma = (int)sc.n_arcs;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int key = __shfl(prim, leader, 64);
    const bool mine = has && prim == key;
    const unsigned long long grp = __ballot(mine);
    const bool single = __popcll(grp) == 1;
    const bool is_arc = key >= Ms;
    if (is_arc ? g_arc != nullptr : g_seg != nullptr) {
      // (adjoint2d leaves an arc's angle columns 2, 3 at zero: they only feed comparisons)
      constexpr int seg_q[4] = {0, 1, 2, 3};
      constexpr int arc_q[3] = {0, 1, 4};
      const int nq = is_arc ? 3 : 4;
      for (int k = 0; k < nq; ++k) {
        const int q = is_arc ? arc_q[k] : seg_q[k];
        fixed_group<ORD>(fx, geo_entry2(key, q, Ms), mine, single, leader, gp[q]);
      }
    }
    if (GN) {
      double* const rows[2] = {is_arc ? sc.grad_arc_n_in : sc.grad_seg_n_in,
                               is_arc ? sc.grad_arc_n_out : sc.grad_seg_n_out};
      for (int q = 0; q < 2; ++q)
        if (rows[q] != nullptr)
          fixed_group<ORD>(fx, index_entry2(key, q, Ms, Ma), mine, single, leader, gn[q]);
    }
    has = has && !mine;
    todo &= ~grp;
  }
}

template <typename T, typename Seed, bool GN, int ORD = ORD_NONE>
__global__ __launch_bounds__(BLOCK) void k_backward2d_goal(
    const T* __restrict__ src, int64_t src_stride, int N, const T* __restrict__ rays_ws,
    int64_t n, const int32_t* __restrict__ rec_prim, const double* __restrict__ rec_u,
    const uint8_t* __restrict__ rec_bin, const int32_t* __restrict__ rec_slot, int P,
    tfrt_scene2d sc, double L, tfrt_ray_out fin, Seed seed, double* __restrict__ g_seg,
    double* __restrict__ g_arc, Fixed2 fx) {
  __shared__ int32_t chain[CHAIN2 * BLOCK];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * BLOCK + tid;
  const bool lane_ok = i < N;
  const int Ms = (int)sc.n_segments;
  auto link_at = [&](int p) -> int32_t& { return chain[(p % CHAIN2) * BLOCK + tid]; };

  // walk forward: every link's index into its pass's input (the last CHAIN2 kept), the end class
  int top = -1, end_cls = -1, end_slot = 0, last = 0;
  if (lane_ok)
    top = walk_chain2(i, rec_bin, rec_slot, n, P, [&](int p, int idx) { link_at(p) = idx; },
                      end_cls, end_slot, last);
  // the seed of a finished chain (rows 0, 1 -> start, rows 2, 3 -> hit), read for no other chain
  double acc = 0.0;
  double sd[4] = {0.0, 0.0, 0.0, 0.0};
  if (end_cls == CLS_FINISHED && end_slot < fin.capacity)
    acc = seed.template seed<T>(fin, end_slot, i, sd);
  if (ORD != ORD_MAX) seed.sum(acc, N);  // (the ordered sweep's first launch leaves the error)

  // reverse: link `top` is the chain's end (seeded when finished, no child), every link below it
  // is an active parent whose child gradient is (gc_s, gc_e)
  int p = top;
  int lo = top - CHAIN2 + 1;          // links [max(lo, 0), top] are in the ring
  double gc_s[2] = {0.0, 0.0}, gc_e[2] = {0.0, 0.0};
  while (__any(p >= 0)) {
    bool has = false;
    int prim = -1;
    double gp[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double gn[2] = {0.0, 0.0};
    if (p >= 0) {
      if (p < lo) {                   // past the ring: re-walk the tape for links [lo, p]
        lo = max(0, p - CHAIN2 + 1);
        int idx = i;
        for (int q = 0; q < lo; ++q) idx = rec_slot[(size_t)q * n + idx];
        for (int q = lo; q <= p; ++q) {
          link_at(q) = idx;
          idx = rec_slot[(size_t)q * n + idx];
        }
      }
      const int idx = link_at(p);
      const bool has_child = p < top;
      double g_s[2] = {0, 0}, g_h[2] = {0, 0}, g_ce[2] = {0, 0};
      if (has_child) {
        // (k_backward2d: g_h, g_ce start at zero and the child's gradient is added)
        for (int k = 0; k < 2; ++k) {
          g_h[k] += gc_s[k];
          g_ce[k] += gc_e[k];
        }
      } else if (end_cls == CLS_FINISHED) {
        for (int k = 0; k < 2; ++k) {
          g_s[k] += sd[k];
          g_h[k] += sd[2 + k];
        }
      }
      bool nz = has_child;
      for (int k = 0; k < 2; ++k) nz = nz || g_s[k] != 0.0 || g_h[k] != 0.0;
      double gs[2] = {0, 0}, ge[2] = {0, 0};
      if (nz) {
        double s[2], e[2];
        if (p == 0) load_ray2(src, src_stride, idx, s, e);
        else load_ray2(rays_ws + (size_t)(p - 1) * 4 * n, n, idx, s, e);
        prim = rec_prim[(size_t)p * n + idx];
        const bool is_arc = prim >= Ms;
        double n_in = 1.0, n_out = 1.0;
        if (has_child) prim_indices(sc, prim, i, &n_in, &n_out);
        const double* pp = is_arc ? sc.arc + (int64_t)(prim - Ms) * 5 : sc.seg + (int64_t)prim * 4;
        adjoint2d(s, e, pp, is_arc, rec_u[(size_t)p * n + idx], has_child, n_in, n_out, L, g_s,
                  g_h, g_ce, gs, ge, gp, sc.finite_tir_gradient != 0, GN ? gn : nullptr);
        has = true;
      }
      for (int k = 0; k < 2; ++k) {
        gc_s[k] = gs[k];
        gc_e[k] = ge[k];
      }
      --p;
    }
    if constexpr (ORD == ORD_NONE) {
      add_prim_grads(has, prim, gp, Ms, g_seg, g_arc);
      if (GN) add_prim_index_grads(has, prim, gn, sc);
    } else {
      add_prim_grads_fixed<ORD, GN>(has, prim, gp, gn, sc, g_seg, g_arc, fx);
    }
  }
}

template <typename T, typename Seed>
static int trace2d_backward_goal_t(const SweepCall2& c, const Seed& seed) {
  const tfrt_scene2d* sc = c.sc;
  const int64_t N = c.N;
  const int P = c.P;
  double *g_seg = c.g_seg, *g_arc = c.g_arc;
  hipStream_t st = c.st;
  const int Ms = (int)sc->n_segments, Ma = (int)sc->n_arcs;
  const Layout2 lay = make_layout2(N, P, c.dtype, Ms, Ma);
  if (c.workspace_bytes < lay.total) return TFRT_E_WORKSPACE;
  const bool gn = index_grads2d(sc);
  // ordered: ORD_MAX, ORD_ACC over all passes, then k_fixed_finish2; at most one term per ray,
  // pass and entry
  const bool ordered = sc->deterministic != 0 && Ms + Ma > 0 && (g_seg || g_arc || gn);
  if (ordered && c.workspace_bytes < lay.total_ordered) return TFRT_E_WORKSPACE;
  if (N == 0) return 0;
  const Tape2<const T> tape(c.workspace, lay, N);
  Fixed2 fx = {nullptr, nullptr, nullptr, 0};
  if (ordered)
    fx = fixed_region2(lay, static_cast<char*>(c.workspace), N * (int64_t)(P > 0 ? P : 1), st);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(cdiv(N, BLOCK)), dim3(BLOCK), 0, st,
                       static_cast<const T*>(c.src), c.src_stride, (int)N, tape.rays_out(0),
                       (int64_t)tape.n, tape.rec_prim(0), tape.rec_u(0), tape.rec_bin(0),
                       tape.rec_slot(0), P, *sc, c.L, *c.fin, seed, g_seg, g_arc, fx);
  };
  if (!ordered) {
    if (gn) launch(k_backward2d_goal<T, Seed, true>);
    else launch(k_backward2d_goal<T, Seed, false>);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  }
  if (gn) {
    launch(k_backward2d_goal<T, Seed, true, ORD_MAX>);
    launch(k_backward2d_goal<T, Seed, true, ORD_ACC>);
  } else {
    launch(k_backward2d_goal<T, Seed, false, ORD_MAX>);
    launch(k_backward2d_goal<T, Seed, false, ORD_ACC>);
  }
  hipLaunchKernelGGL(k_fixed_finish2, dim3(cdiv(6 * (int64_t)Ms + 7 * (int64_t)Ma, BLOCK)),
                     dim3(BLOCK), 0, st, fx, Ms, Ma, g_seg, g_arc, *sc);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

// tfrt_trace2d_rows: every source ray's column of fixed-shape rows.  Lane i walks ray i's chain
// as k_backward2d_goal does; a chain that finished copies its row of the `finished` block (the
// state dtype, bit for bit) and its primitive, any other chain the source ray itself and -1.
// Every column is written once.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_rows2d(
    const T* __restrict__ src, int64_t src_stride, int N, int64_t n,
    const int32_t* __restrict__ rec_prim, const uint8_t* __restrict__ rec_bin,
    const int32_t* __restrict__ rec_slot, int P, tfrt_ray_out fin, T* __restrict__ rows,
    int64_t rows_stride, int32_t* __restrict__ row_face) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= N) return;
  int end_cls = -1, end_slot = 0, last = 0;
  const int top = walk_chain2(i, rec_bin, rec_slot, n, P, [](int, int) {}, end_cls, end_slot,
                              last);
  const T* from = src;
  int64_t stride = src_stride, col = i;
  int face = -1;
  if (end_cls == CLS_FINISHED && end_slot < fin.capacity) {
    from = static_cast<const T*>(fin.rays);
    stride = fin.capacity;
    col = end_slot;
    face = rec_prim[(size_t)top * n + last];
  }
  for (int r = 0; r < 4; ++r) rows[r * rows_stride + i] = from[r * stride + col];
  row_face[i] = face;
}

template <typename T>
static int trace2d_rows_t(const void* src_rays, int64_t src_stride, int64_t N, int P, int dtype,
                          const tfrt_ray_out& fin, void* rows, int64_t rows_stride,
                          int32_t* row_face, void* workspace, size_t workspace_bytes,
                          hipStream_t st) {
  const Layout2 lay = make_layout2(N, P, dtype);
  if (workspace_bytes < lay.total) return TFRT_E_WORKSPACE;
  if (N == 0) return 0;
  const Tape2<const T> tape(workspace, lay, N);
  hipLaunchKernelGGL((k_rows2d<T>), dim3(cdiv(N, BLOCK)), dim3(BLOCK), 0, st,
                     static_cast<const T*>(src_rays), src_stride, (int)N, (int64_t)tape.n,
                     tape.rec_prim(0), tape.rec_bin(0), tape.rec_slot(0), P, fin,
                     static_cast<T*>(rows), rows_stride, row_face);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

// The second stage of a 2-D error sum (per-wavefront partials): {sum, terms = finished rays x
// n_terms, mean} and the trace's test count, from the trailing counters of the trace
// {total_active, total_finished, ..., n_tests_lo, n_tests_hi}.
static tfrt_goal_pending goal_pending2(double* partial, int64_t n_rays, const int32_t* counts,
                                       int max_passes, int n_terms, double* error_out,
                                       int64_t* tests_total) {
  const int32_t* tail = counts + (size_t)max_passes * TFRT_COUNTS_PER_PASS;
  tfrt_goal_pending g = {};
  g.partial = partial;
  g.n_partial = n_rays > 0 ? cdiv(n_rays, 64) : 0;
  g.n_finished = tail + 1;
  g.n_fields = n_terms;
  g.error_out = error_out;
  g.tests_lo_hi = tail + 4;
  g.tests_total = tests_total;
  return g;
}

template <bool ARC>
static int seam2d(const void* rays, int64_t stride, int64_t n_rays, int32_t dtype,
                  const double* prim, int64_t M, double ei, double es, double er, double* x,
                  double* y, uint8_t* valid, double* ray_u, double* prim_u, int32_t* gather,
                  void* stream) {
  if (n_rays < 0 || M < 0 || stride < n_rays || (M > 0 && !prim)) return TFRT_E_BADARG;
  if (n_rays == 0) return 0;
  if (!rays || !x || !y || !valid || !ray_u || !prim_u || !gather) return TFRT_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(n_rays, BLOCK));
  return dispatch_state(dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((k_seam2d<T, ARC>), grid, dim3(BLOCK), 0, st, static_cast<const T*>(rays),
                       stride, (int)n_rays, prim, (int)M, ei, es, er, x, y, valid, ray_u, prim_u,
                       gather);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

int tfrt_segment_intersection(const void* rays, int64_t stride, int64_t n_rays,
                              int32_t state_dtype, const double* seg, int64_t n_segments,
                              double intersect_epsilion, double size_epsilion,
                              double ray_start_epsilion, double* x, double* y, uint8_t* valid,
                              double* ray_u, double* seg_u, int32_t* gather_segment,
                              void* stream) {
  return seam2d<false>(rays, stride, n_rays, state_dtype, seg, n_segments, intersect_epsilion,
                       size_epsilion, ray_start_epsilion, x, y, valid, ray_u, seg_u,
                       gather_segment, stream);
}

int tfrt_arc_intersection(const void* rays, int64_t stride, int64_t n_rays, int32_t state_dtype,
                          const double* arc, int64_t n_arcs, double intersect_epsilion,
                          double size_epsilion, double ray_start_epsilion, double* x, double* y,
                          uint8_t* valid, double* ray_u, double* arc_u, int32_t* gather_arc,
                          void* stream) {
  return seam2d<true>(rays, stride, n_rays, state_dtype, arc, n_arcs, intersect_epsilion,
                      size_epsilion, ray_start_epsilion, x, y, valid, ray_u, arc_u, gather_arc,
                      stream);
}

size_t tfrt_trace2d_workspace_bytes(int64_t n_rays, int64_t n_segments, int64_t n_arcs,
                                    int32_t max_passes, int32_t state_dtype) {
  if (n_rays < 0 || n_segments < 0 || n_arcs < 0 || max_passes < 0) return 0;
  // (the segments and arcs size the ordered reverse sweeps' accumulators)
  return make_layout2(n_rays, max_passes, state_dtype, n_segments, n_arcs).total_ordered;
}

int tfrt_trace2d_forward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                         const tfrt_scene2d* scene, double new_ray_length,
                         double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                         uint32_t flags, tfrt_ray_out* finished, tfrt_ray_out* active,
                         tfrt_ray_out* stopped, tfrt_ray_out* dead, void* unfinished,
                         int32_t* unfinished_id, int32_t* counts, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (!scene2_ok(scene) || n_rays < 0 || n_rays >= (1ll << 31) - 4096 || max_passes < 0 ||
      !counts || !workspace || (n_rays > 0 && !src_rays) || src_stride < n_rays)
    return TFRT_E_BADARG;
  const TraceCall<tfrt_scene2d> c = {
      src_rays, src_stride, n_rays, scene, new_ray_length, dead_ray_length, max_passes,
      state_dtype, flags, finished, active, stopped, dead, unfinished, unfinished_id, counts,
      workspace, workspace_bytes, static_cast<hipStream_t>(stream)};
  return dispatch_state(state_dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    return trace2d_forward_t<typename decltype(tag)::type>(c);
  });
}

int tfrt_trace2d_backward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                          const tfrt_scene2d* scene, double new_ray_length,
                          double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                          const double* grad_finished, int64_t cap_finished,
                          const double* grad_active, int64_t cap_active,
                          const double* grad_stopped, int64_t cap_stopped,
                          const double* grad_dead, int64_t cap_dead, double* grad_seg,
                          double* grad_arc, double* grad_src_rays, const int32_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!scene2_ok(scene) || n_rays < 0 || max_passes < 0 || !counts || !workspace)
    return TFRT_E_BADARG;
  SweepCall2 c = {src_rays, src_stride, n_rays, scene, new_ray_length, dead_ray_length,
                  max_passes, state_dtype, counts, workspace, workspace_bytes,
                  static_cast<hipStream_t>(stream)};
  c.g_fin = grad_finished, c.cap_fin = cap_finished;
  c.g_act = grad_active, c.cap_act = cap_active;
  c.g_stp = grad_stopped, c.cap_stp = cap_stopped;
  c.g_dead = grad_dead, c.cap_dead = cap_dead;
  c.g_seg = grad_seg, c.g_arc = grad_arc, c.g_src = grad_src_rays;
  return dispatch_state(state_dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    return trace2d_backward_t<typename decltype(tag)::type>(c);
  });
}

size_t tfrt_trace2d_backward_goal_workspace_bytes(int64_t n_rays) {
  if (n_rays < 0) return 0;
  // one partial error sum per 64 rays
  return align_up((size_t)cdiv(n_rays > 0 ? n_rays : 1, 64) * sizeof(double));
}

int tfrt_trace2d_backward_goal(const void* src_rays, int64_t src_stride, int64_t n_rays,
                               const tfrt_scene2d* scene, double new_ray_length,
                               int32_t max_passes, int32_t state_dtype,
                               const tfrt_ray_out* finished, const int32_t* fields,
                               int32_t n_fields, const double* goal, int64_t goal_stride,
                               int64_t goal_ray_stride, double* error_out, int64_t* tests_total,
                               void* goal_workspace, size_t goal_workspace_bytes,
                               tfrt_goal_pending* pending, double* grad_seg, double* grad_arc,
                               const int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!scene2_ok(scene) || n_rays < 0 || n_rays >= (1ll << 31) - 4096 || max_passes < 0 ||
      !counts || !workspace || !finished || !fields || n_fields < 1 || n_fields > 4 ||
      !error_out || !pending || !goal_workspace || goal_stride < 0 || goal_ray_stride < 0 ||
      goal_workspace_bytes < tfrt_trace2d_backward_goal_workspace_bytes(n_rays))
    return TFRT_E_BADARG;
  // (a forward compiled without finished rays left nothing to compare with the goal)
  if (n_rays > 0 && (!src_rays || src_stride < n_rays || !goal || !finished->rays ||
                     finished->capacity <= 0))
    return TFRT_E_BADARG;
  if (!state_dtype_ok(state_dtype)) return TFRT_E_UNSUPPORTED;
  ChainGoal2 cg;
  cg.gf.n = n_fields;
  for (int c = 0; c < 6; ++c) {
    cg.gf.row[c] = c < n_fields ? fields[c] : 0;
    if (cg.gf.row[c] < 0 || cg.gf.row[c] > 3) return TFRT_E_BADARG;
  }
  cg.goal = goal;
  cg.goal_stride = goal_stride;
  cg.goal_ray_stride = goal_ray_stride;
  double* partial = static_cast<double*>(goal_workspace);
  const SeedGoal2 seed = {cg, partial};
  SweepCall2 c = {src_rays, src_stride, n_rays, scene, new_ray_length, /*dead_len=*/0.0,
                  max_passes, state_dtype, counts, workspace, workspace_bytes,
                  static_cast<hipStream_t>(stream)};
  c.g_seg = grad_seg, c.g_arc = grad_arc, c.fin = finished;
  const int rc = dispatch_state(state_dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    return trace2d_backward_goal_t<typename decltype(tag)::type>(c, seed);
  });
  if (rc != 0) return rc;
  *pending = goal_pending2(partial, n_rays, counts, max_passes, n_fields, error_out, tests_total);
  return 0;
}

int tfrt_trace2d_rows(const void* src_rays, int64_t src_stride, int64_t n_rays,
                      int32_t max_passes, int32_t state_dtype, const tfrt_ray_out* finished,
                      void* rows, int64_t rows_stride, int32_t* row_face, const int32_t* counts,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (n_rays < 0 || n_rays >= (1ll << 31) - 4096 || max_passes < 0 || !counts || !workspace ||
      !finished)
    return TFRT_E_BADARG;
  if (n_rays > 0 && (!src_rays || src_stride < n_rays || !rows || rows_stride < n_rays ||
                     !row_face || !finished->rays || finished->capacity <= 0))
    return TFRT_E_BADARG;
  return dispatch_state(state_dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    return trace2d_rows_t<typename decltype(tag)::type>(
        src_rays, src_stride, n_rays, max_passes, state_dtype, *finished, rows, rows_stride,
        row_face, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  });
}

int tfrt_trace2d_backward_rows(const void* src_rays, int64_t src_stride, int64_t n_rays,
                               const tfrt_scene2d* scene, double new_ray_length,
                               int32_t max_passes, int32_t state_dtype,
                               const tfrt_ray_out* finished, const double* err_terms,
                               int32_t n_terms, int64_t err_stride, int64_t err_ray_stride,
                               const double* grad_rows, int64_t grad_stride, double* error_out,
                               int64_t* tests_total, void* goal_workspace,
                               size_t goal_workspace_bytes, tfrt_goal_pending* pending,
                               double* grad_seg, double* grad_arc, const int32_t* counts,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!scene2_ok(scene) || n_rays < 0 || n_rays >= (1ll << 31) - 4096 || max_passes < 0 ||
      !counts || !workspace || !finished || n_terms < 1 || err_stride < 0 ||
      err_ray_stride < 0 || !error_out || !pending || !goal_workspace ||
      goal_workspace_bytes < tfrt_trace2d_backward_goal_workspace_bytes(n_rays))
    return TFRT_E_BADARG;
  if (n_rays > 0 && (!src_rays || src_stride < n_rays || !err_terms ||
                     (grad_rows && grad_stride < n_rays) || !finished->rays ||
                     finished->capacity <= 0))
    return TFRT_E_BADARG;
  double* partial = static_cast<double*>(goal_workspace);
  const SeedRows2 seed = {grad_rows, grad_stride, err_terms, err_stride, err_ray_stride, n_terms,
                          partial};
  SweepCall2 c = {src_rays, src_stride, n_rays, scene, new_ray_length, /*dead_len=*/0.0,
                  max_passes, state_dtype, counts, workspace, workspace_bytes,
                  static_cast<hipStream_t>(stream)};
  c.g_seg = grad_seg, c.g_arc = grad_arc, c.fin = finished;
  const int rc = dispatch_state(state_dtype, TFRT_E_UNSUPPORTED, [&](auto tag) {
    return trace2d_backward_goal_t<typename decltype(tag)::type>(c, seed);
  });
  if (rc != 0) return rc;
  *pending = goal_pending2(partial, n_rays, counts, max_passes, n_terms, error_out, tests_total);
  return 0;
}

}  // extern "C"
