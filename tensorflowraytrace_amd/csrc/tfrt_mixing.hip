// MixingError: every group of rays must land with the SAME density on the target, whatever that
// density is -- the dies of an LED behind a mixing rod, the input zones of a homogeniser, the
// beams of a combiner.
//
// Every source ray carries a group label.  The finished rays are spread bilinearly over the
// centres of an (ny x nx) grid of bins exactly as DensityError spreads them (density_rays.h), each
// into its own group's plane of the int64 histogram Hq[G][ny][nx].  With nq_g the mass of a group,
// Pq_b the mass of a bin over all groups and Nq the mass of the pool -- integer sums --, the error
// is the mass-weighted mean over the groups of B sum_b (Hq_gb / nq_g - Pq_b / Nq)^2, plus
// DensityError's penalty for rays outside the domain.  The definition, operation by operation, is
// in include/tfrt_hip.h at tfrt_mixing_error; the per-group and per-bin arithmetic is in
// mixing_math.h; tests/mixing_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: every bilinear weight enters its cell as the integer
// rint(b * 2^32), the margins are integer sums (free of order), every floating-point sum has a
// fixed shape and order.  No float atomics, nothing waits on another workgroup.
//
// The gradient needs no derivative of the pooled density, of a group's mass or of the pool's: the
// pooled density is the mass-weighted mean of the groups' and so minimises the error, and a ray
// inside carries total weight 1 wherever it stands.
//
// Six launches:
//
//   k_error_clear      zeroes Hq (error_sums.h says why it is a launch).
//   k_mixing_splat     one lane per column (DensityError's grid, grid-stride): the label of the
//                      column's source ray, weights -> its group's plane of Hq, and the
//                      out-of-domain penalty as one partial sum per workgroup.  Two variants:
//                      <true>  G * bins <= DENSITY_LDS_BINS cells: the whole table as int64 in LDS
//                              (32 KiB at most), flushed with one global atomic per non-zero cell;
//                      <false> more cells: global 64-bit atomics per weight.
//   k_mixing_margins   the integer margins WITHOUT atomics (so nothing has to be cleared for
//                      them): workgroup g < G sums the bins of group g into nq[g]; the workgroups
//                      behind them take one bin per lane and sum it over the groups into Pq[b].
//   k_mixing_pulls     one workgroup per group: Nq from nq, then thread t owns the bins t,
//                      t + 1024, ... of its group (their squares summed in that order), writes
//                      their pulls D and, after the fixed-shape workgroup sum, the group's e_g.
//   k_mixing_finish    ONE workgroup: E_mix over the groups in k_centroid_table's order, the
//                      splat's partials in index order, {sum, 1, mean} and {groups_used, N}.
//   k_mixing_seed      one lane per column: the gradient rows of EVERY column (zeros where a ray
//                      does not count) from its group's plane of D and the splat's classification.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "density_rays.h"
#include "mixing_math.h"

namespace tfrt {

constexpr int MIXING_BLOCK = 1024;
constexpr int MIXING_WAVES = MIXING_BLOCK / 64;

// The labels of a launch: one int32 per SOURCE ray; column i is source ray perm[i] (perm null: i).
struct MixingLabels {
  const int32_t* group;
  const int32_t* perm;
  int64_t n_source;
  int32_t n_groups;
};

// DensityError's classification, then the label: a column that counts (kinds 1 and 2) without a
// source ray or with a label outside [0, G) does not count (kind 0).  Nothing is read out of
// bounds, whatever perm and the labels hold.
template <typename T, int DIM, bool WEIGHTED>
__device__ __forceinline__ DensityRay mixing_classify(const T* __restrict__ rows, int64_t stride,
                                                      const int32_t* __restrict__ mask, int64_t i,
                                                      const DensityArgs<WEIGHTED>& g,
                                                      const MixingLabels& lab, LinkDir<DIM>& link,
                                                      double& w, int& label) {
  DensityRay r = density_classify<T, DIM, WEIGHTED>(rows, stride, mask, i, g, link, w);
  label = 0;
  if (r.kind != 0) {
    const int64_t s = lab.perm != nullptr ? (int64_t)lab.perm[i] : i;
    const bool has = s >= 0 && s < lab.n_source;
    const int32_t l = has ? lab.group[s] : -1;
    if (mixing_label_ok(l, lab.n_groups))
      label = l;
    else
      r.kind = 0;
  }
  return r;
}

// WEIGHTED: every bilinear weight and the penalty times w last.
template <typename T, bool LDS, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_mixing_splat(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    DensityArgs<WEIGHTED> g, MixingLabels lab, unsigned long long* __restrict__ hq,
    double* __restrict__ partial) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long hist[];
  __shared__ double wsum[WAVES];
  const int bins = g.nx * g.ny;
  const int cells = bins * lab.n_groups;
  if (LDS) {
    for (int c = threadIdx.x; c < cells; c += BLOCK) hist[c] = 0ull;
    __syncthreads();
  }
  double pen = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double w = 0.0;
    int label;
    const DensityRay r =
        mixing_classify<T, DIM, WEIGHTED>(rows, stride, mask, i, g, lab, link, w, label);
    if (r.kind == 2) {
      pen += weighed<WEIGHTED>(g.oob * (r.tx * r.tx + r.ty * r.ty), w);
    } else if (r.kind == 1) {
      unsigned long long* dst = (LDS ? hist : hq) + (int64_t)label * bins;
      const double wx0 = 1.0 - r.tx, wx1 = r.tx;
      if (g.row_y >= 0) {
        const double wy0 = 1.0 - r.ty, wy1 = r.ty;
        atomicAdd(&dst[r.ja * g.nx + r.ia], density_fixed(weighed<WEIGHTED>(wy0 * wx0, w)));
        atomicAdd(&dst[r.ja * g.nx + r.ib], density_fixed(weighed<WEIGHTED>(wy0 * wx1, w)));
        atomicAdd(&dst[r.jb * g.nx + r.ia], density_fixed(weighed<WEIGHTED>(wy1 * wx0, w)));
        atomicAdd(&dst[r.jb * g.nx + r.ib], density_fixed(weighed<WEIGHTED>(wy1 * wx1, w)));
      } else {
        atomicAdd(&dst[r.ia], density_fixed(weighed<WEIGHTED>(wx0, w)));
        atomicAdd(&dst[r.ib], density_fixed(weighed<WEIGHTED>(wx1, w)));
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += BLOCK) {
      const unsigned long long v = hist[c];
      if (v != 0ull) atomicAdd(&hq[c], v);
    }
  }
  const double s = error_block_sum<WAVES>(pen, wsum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// Workgroup g < G: nq[g], the integer sum of the bins of group g.  The workgroups from G on: one
// bin per lane, Pq[b], the integer sum of the bin over the groups (consecutive lanes read
// consecutive cells of a plane).  Integer sums: their order does not show.
__global__ __launch_bounds__(BLOCK) void k_mixing_margins(const long long* __restrict__ hq,
                                                          int n_groups, int bins,
                                                          long long* __restrict__ nq,
                                                          long long* __restrict__ pq) {
  __shared__ long long wcnt[WAVES];
  if ((int)blockIdx.x < n_groups) {
    const long long* plane = hq + (int64_t)blockIdx.x * bins;
    long long s = 0;
    for (int b = threadIdx.x; b < bins; b += BLOCK) s += plane[b];
    s = error_block_sum<WAVES>(s, wcnt);
    if (threadIdx.x == 0) nq[blockIdx.x] = s;
    return;
  }
  const int b = ((int)blockIdx.x - n_groups) * BLOCK + threadIdx.x;
  if (b >= bins) return;
  long long s = 0;
  for (int k = 0; k < n_groups; ++k) s += hq[(int64_t)k * bins + b];
  pq[b] = s;
}

// The mass of the pool: the integer sum of nq over the groups, in every thread of a workgroup of
// MIXING_BLOCK (every thread must call it).
__device__ __forceinline__ long long mixing_pool_mass(const long long* __restrict__ nq,
                                                      int n_groups, long long* wcnt) {
  long long s = 0;
  for (int k = threadIdx.x; k < n_groups; k += MIXING_BLOCK) s += nq[k];
  return error_block_sum<MIXING_WAVES>(s, wcnt);
}

// One workgroup per group.  Thread t owns the bins t, t + 1024, ... of the group (summed in that
// order), then the fixed-shape workgroup sum: the same bits on every run.
__global__ __launch_bounds__(MIXING_BLOCK) void k_mixing_pulls(
    const long long* __restrict__ hq, const long long* __restrict__ nq,
    const long long* __restrict__ pq, int n_groups, int bins, double* __restrict__ pull,
    double* __restrict__ group_errors) {
#pragma clang fp contract(off)
  __shared__ double wsum[MIXING_WAVES];
  __shared__ long long wcnt[MIXING_WAVES];
  const int t = threadIdx.x;
  const int k = blockIdx.x;
  const MixingPool pool = mixing_pool(mixing_pool_mass(nq, n_groups, wcnt), bins);
  const long long nq_g = nq[k];
  const bool used = nq_g > 0;   // (then the pool has rays)
  const long long* plane = hq + (int64_t)k * bins;
  double* out = pull + (int64_t)k * bins;
  double sum = 0.0;
  for (int b = t; b < bins; b += MIXING_BLOCK) {
    double D = 0.0;
    if (used) sum += mixing_cell(plane[b], nq_g, pq[b], pool, &D);
    out[b] = D;
  }
  sum = error_block_sum<MIXING_WAVES>(sum, wsum);
  if (t == 0) group_errors[k] = mixing_group_error(used, bins, sum);
}

// One workgroup.  Thread t owns the groups (and then the partials) t, t + 1024, ... (summed in
// that order), then the fixed-shape workgroup sum of k_centroid_table.
__global__ __launch_bounds__(MIXING_BLOCK) void k_mixing_finish(
    const long long* __restrict__ nq, const double* __restrict__ group_errors, int n_groups,
    int bins, const double* __restrict__ partial, int n_partial, double* __restrict__ used_out,
    double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[MIXING_WAVES];
  __shared__ long long wcnt[MIXING_WAVES];
  __shared__ double tsum;
  __shared__ long long tcnt;
  const int t = threadIdx.x;
  const MixingPool pool = mixing_pool(mixing_pool_mass(nq, n_groups, wcnt), bins);
  double e = 0.0;
  long long used = 0;
  for (int k = t; k < n_groups; k += MIXING_BLOCK) {
    const long long nq_g = nq[k];
    if (nq_g > 0) {
      e += mixing_term(nq_g, pool, group_errors[k]);
      used += 1;
    }
  }
  e = error_block_total<MIXING_WAVES>(e, wsum, &tsum);
  used = error_block_total<MIXING_WAVES>(used, wcnt, &tcnt);
  // the splat's partials, in index order
  double pen = 0.0;
  for (int b = t; b < n_partial; b += MIXING_BLOCK) pen += partial[b];
  pen = error_block_total<MIXING_WAVES>(pen, wsum, &tsum);
  if (t == 0) {
    const double total = e + pen;
    error_out[0] = total;
    error_out[1] = 1.0;   // one error term: the reported mean is the sum
    error_out[2] = total;
    used_out[0] = (double)used;
    used_out[1] = pool.n;
  }
}

// WEIGHTED: gx, gy times w last, in front of the chain rule.
template <typename T, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_mixing_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    DensityArgs<WEIGHTED> g, MixingLabels lab, const double* __restrict__ pull,
    double* __restrict__ grad, int64_t grad_stride) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  LinkDir<DIM> link;
  double w = 0.0;
  int label;
  const DensityRay r =
      mixing_classify<T, DIM, WEIGHTED>(rows, stride, mask, i, g, lab, link, w, label);
  const bool two = g.row_y >= 0;
  double gx = 0.0, gy = 0.0;
  if (r.kind == 2) {
    gx = weighed<WEIGHTED>(g.oob * (2.0 * r.tx) * r.dx, w);
    gy = weighed<WEIGHTED>(g.oob * (2.0 * r.ty) * r.dy, w);
  } else if (r.kind == 1) {
    const double* D = pull + (int64_t)label * (g.nx * g.ny);
    if (two) {
      const double d00 = D[r.ja * g.nx + r.ia], d01 = D[r.ja * g.nx + r.ib];
      const double d10 = D[r.jb * g.nx + r.ia], d11 = D[r.jb * g.nx + r.ib];
      gx = weighed<WEIGHTED>(g.sx * ((1.0 - r.ty) * (d01 - d00) + r.ty * (d11 - d10)), w);
      gy = weighed<WEIGHTED>(g.sy * ((1.0 - r.tx) * (d10 - d00) + r.tx * (d11 - d01)), w);
    } else {
      gx = weighed<WEIGHTED>(g.sx * (D[r.ib] - D[r.ia]), w);
    }
  }
  if constexpr (DIM != 0) {
    // (every row of the column: a direction pulls on the start and on the end of the link)
    chain_fields<DIM>(link, r.kind != 0, g.row_x, g.row_y, gx, gy, grad, grad_stride, i);
  } else {
    grad[(int64_t)g.row_x * grad_stride + i] = gx;
    if (two) grad[(int64_t)g.row_y * grad_stride + i] = gy;
  }
}

static bool mixing_shape_ok(int32_t n_groups, int32_t nx, int32_t ny) {
  return n_groups >= 1 && n_groups <= MIXING_MAX_GROUPS && nx >= 1 && ny >= 1 &&
         (int64_t)nx * ny <= DENSITY_MAX_BINS &&
         (int64_t)n_groups * nx * ny <= MIXING_MAX_CELLS;
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_mixing_error_workspace_bytes(int64_t n, int32_t n_groups, int32_t nx, int32_t ny) {
  if (n < 0 || n > INT32_MAX || !mixing_shape_ok(n_groups, nx, ny)) return 0;
  return align_up((size_t)nx * ny * sizeof(long long)) +
         align_up((size_t)n_groups * sizeof(long long)) +
         align_up(DENSITY_MAX_GRID * sizeof(double));
}

int tfrt_mixing_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                      int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                      const int32_t* group, int64_t n_source, const int32_t* perm,
                      int32_t n_groups, const double* weight, int32_t nx, int32_t ny, double x0,
                      double x1, double sx, double y0, double y1, double sy, double oob_weight,
                      double* grad, int64_t grad_stride, double* error_out, double* used_out,
                      double* group_errors, double* pull, int64_t* hq, int32_t variant,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  if (!mixing_shape_ok(n_groups, nx, ny) || (field_y < 0 && ny != 1) || !group || n_source < 0 ||
      n_source > INT32_MAX || !used_out || !group_errors || !pull ||
      !error_args_ok(rows, stride, n, state_dtype, field_x, field_y, x0, x1, sx, y0, y1, sy,
                     oob_weight, grad, grad_stride, error_out, hq, variant, workspace))
    return TFRT_E_BADARG;
  const int bins = nx * ny;
  const int cells = bins * n_groups;
  if (variant == 1 && cells > DENSITY_LDS_BINS) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_mixing_error_workspace_bytes(n, n_groups, nx, ny))
    return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && cells <= DENSITY_LDS_BINS);
  const bool two = field_y >= 0;

  DensityGrid g;
  g.x0 = x0, g.x1 = x1, g.sx = sx, g.oob = oob_weight;
  g.y0 = two ? y0 : 0.0, g.y1 = two ? y1 : 0.0, g.sy = two ? sy : 0.0;
  g.nx = nx, g.ny = ny, g.row_x = field_x, g.row_y = field_y;
  MixingLabels lab;
  lab.group = group, lab.perm = perm, lab.n_source = n_source, lab.n_groups = n_groups;
  DensityWeights wt;
  wt.weight = weight, wt.perm = perm, wt.n_source = n_source;

  char* ws = static_cast<char*>(workspace);
  long long* pq = reinterpret_cast<long long*>(ws);
  long long* nq = reinterpret_cast<long long*>(ws + align_up((size_t)bins * sizeof(long long)));
  double* partial = reinterpret_cast<double*>(ws + align_up((size_t)bins * sizeof(long long)) +
                                              align_up((size_t)n_groups * sizeof(long long)));
  unsigned long long* hqu = reinterpret_cast<unsigned long long*>(hq);
  const long long* hqs = reinterpret_cast<const long long*>(hq);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, DENSITY_RAYS_PER_BLOCK, DENSITY_MAX_GRID);
  const int nblk = cdiv(n, BLOCK);

  hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(cells, BLOCK)), dim3(BLOCK), 0, st, hqu, cells);
  auto launch = [&](auto tag, auto d, auto c) {
    using T = typename decltype(tag)::type;
    constexpr int DIM = decltype(d)::value;
    constexpr bool WEIGHTED = decltype(c)::weighted;
    const T* r = static_cast<const T*>(rows);
    if (grid > 0 && lds)
      hipLaunchKernelGGL((k_mixing_splat<T, true, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK),
                         (size_t)cells * sizeof(unsigned long long), st, r, stride, n, mask, c, lab,
                         hqu, partial);
    else if (grid > 0)
      hipLaunchKernelGGL((k_mixing_splat<T, false, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK), 0, st,
                         r, stride, n, mask, c, lab, hqu, partial);
    hipLaunchKernelGGL(k_mixing_margins, dim3(n_groups + cdiv(bins, BLOCK)), dim3(BLOCK), 0, st,
                       hqs, n_groups, bins, nq, pq);
    hipLaunchKernelGGL(k_mixing_pulls, dim3(n_groups), dim3(MIXING_BLOCK), 0, st, hqs, nq, pq,
                       n_groups, bins, pull, group_errors);
    hipLaunchKernelGGL(k_mixing_finish, dim3(1), dim3(MIXING_BLOCK), 0, st, nq, group_errors,
                       n_groups, bins, partial, grid, used_out, error_out);
    if (nblk > 0)
      hipLaunchKernelGGL((k_mixing_seed<T, DIM, WEIGHTED>), dim3(nblk), dim3(BLOCK), 0, st, r,
                         stride, n, mask, c, lab, pull, grad, grad_stride);
  };
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    dispatch_fields(dimension, field_x, field_y, [&](auto d) {
      if (weight != nullptr)
        launch(tag, d, DensityArgs<true>{g, wt});
      else
        launch(tag, d, DensityArgs<false>{g});
    });
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
