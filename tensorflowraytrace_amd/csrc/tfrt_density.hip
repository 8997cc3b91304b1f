// DensityError: the finished rays, taken together, must land with a given density on the target.
//
// The rays' end points are spread bilinearly over the centres of an (ny x nx) grid of bins -- a
// soft histogram H --, both H and the goal are L2-normalised, and the error is the sum of squared
// differences (tfrt/analyze.py:134-290, DistributionDifferential, is the same on hard bins: it has
// no gradient).  The definition, operation by operation, is in include/tfrt_hip.h at
// tfrt_density_error; tests/density_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: every weight w is added to its bin as the INTEGER
// rint(w * 2^32) (int64; n < 2^31 rays of total weight 1 each stay below 2^63).  Integer addition
// is associative, so the histogram does not depend on the order in which the atomics land; every
// floating-point reduction has a fixed shape and order.  No float atomics anywhere.
//
// Four launches:
//
//   k_error_clear     zeroes Hq.  A launch, not a memset node: why, at the kernel (error_sums.h).
//   k_density_splat   one lane per column (a fixed grid for n, grid-stride): weights -> Hq, and the
//                     out-of-domain penalty as one partial sum per workgroup.  Two variants:
//                     <true>  bins <= DENSITY_LDS_BINS: a per-workgroup int64 histogram in LDS
//                             (ds_add_u64; 8 B per bin, at most 32 KiB of the CU's 160 KiB: with
//                             the 32 B of the penalty sum four workgroups -- 4 waves per SIMD --
//                             still fit a CU), flushed with one global atomic per non-zero bin.
//                             Many rays hit few bins: the contention stays in LDS.
//                     <false> more bins: global 64-bit atomics (global_atomic_add_x2) per weight.
//   k_density_bins    ONE workgroup of 1024: s = ||H||, E_hist, the pull D on every bin (up to
//                     65,536 of them), the penalty partials in index order, {sum, terms, mean}.
//   k_density_seed    one lane per column: both gradient rows of EVERY column (zeros where a ray
//                     does not count) from D and the same classification as the splat.
//
// A field is a row of the ray block or a direction cosine of the finished ray's last link
// (tfrt_density_error_fields; the codes, the direction and the chain rule of its gradient:
// direction_fields.h).  The splat and the seed are templated on "has a direction field": without
// one they are the kernels of position fields, load for load; with one they recompute the
// direction from the rows they stream, and the seed writes EVERY row of the column.
//
// The penalty is summed where the rays are first classified (the splat) and finished by the one
// workgroup that runs anyway (the bins): a sum formed by the seed would need a fourth, dependent
// launch (~4.5 us) or a "last workgroup finishes" fence (what that costs: tfrt_error.hip).
//
// Weighted (tfrt_density_error_weighted): every source ray carries a radiant power w in [0, 1],
// looked up once per column through `perm`; a bilinear weight enters its bin as
// rint((b * w) * 2^32), gradient and penalty are multiplied by w last, and the bins launch is the
// unweighted one on the weighted histogram.  The splat, the seed and the classification they share
// have a `bool WEIGHTED` template parameter: everything that touches w stands under
// `if constexpr (WEIGHTED)`, and the weights are a base of the kernels' constants that is empty
// without them (DensityArgs), so the unweighted instantiations neither receive nor read a weight.
//
// What this file shares with tfrt_spot.hip -- the fixed-shape workgroup sum, the clear kernel, the
// out-of-domain axis, the grid size, the argument checks, the dispatch on the direction fields --
// is in error_sums.h; what it shares with tfrt_mixing.hip -- the constants of a launch, the
// classification of a column, the fixed point of a weight -- in density_rays.h.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "density_rays.h"

namespace tfrt {

constexpr int BINS_BLOCK = 1024;
constexpr int BINS_WAVES = BINS_BLOCK / 64;

// WEIGHTED: every bilinear weight and the penalty times w last.
template <typename T, bool LDS, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_density_splat(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    DensityArgs<WEIGHTED> g, unsigned long long* __restrict__ hq, double* __restrict__ partial) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long hist[];
  __shared__ double wsum[WAVES];
  const int bins = g.nx * g.ny;
  if (LDS) {
    for (int b = threadIdx.x; b < bins; b += BLOCK) hist[b] = 0ull;
    __syncthreads();
  }
  unsigned long long* dst = LDS ? hist : hq;
  double pen = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double w = 0.0;
    const DensityRay r = density_classify<T, DIM, WEIGHTED>(rows, stride, mask, i, g, link, w);
    if (r.kind == 2) {
      pen += weighed<WEIGHTED>(g.oob * (r.tx * r.tx + r.ty * r.ty), w);
    } else if (r.kind == 1) {
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
    for (int b = threadIdx.x; b < bins; b += BLOCK) {
      const unsigned long long v = hist[b];
      if (v != 0ull) atomicAdd(&hq[b], v);
    }
  }
  const double s = error_block_sum<WAVES>(pen, wsum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup.  Thread t owns bins t, t + 1024, ... (summed in that order), then the fixed-shape
// workgroup sum: the same bits on every run.
__global__ __launch_bounds__(BINS_BLOCK) void k_density_bins(
    const long long* __restrict__ hq, const double* __restrict__ goal, int bins,
    const double* __restrict__ partial, int n_partial, double* __restrict__ pull,
    double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[BINS_WAVES];
  const int t = threadIdx.x;
  double hh = 0.0, gg = 0.0, pen = 0.0;
  for (int b = t; b < bins; b += BINS_BLOCK) {
    const double H = (double)hq[b] / 4294967296.0;
    const double gb = goal[b];
    hh += H * H;
    gg += gb * gb;
  }
  for (int b = t; b < n_partial; b += BINS_BLOCK) pen += partial[b];
  hh = error_block_sum<BINS_WAVES>(hh, wsum);
  gg = error_block_sum<BINS_WAVES>(gg, wsum);
  pen = error_block_sum<BINS_WAVES>(pen, wsum);
  const double s = sqrt(hh);
  double e_hist;
  if (s == 0.0) {
    for (int b = t; b < bins; b += BINS_BLOCK) pull[b] = 0.0;
    e_hist = gg;
  } else {
    double rr = 0.0, hr = 0.0;
    for (int b = t; b < bins; b += BINS_BLOCK) {
      const double h = ((double)hq[b] / 4294967296.0) / s;
      const double r = h - goal[b];
      rr += r * r;
      hr += h * r;
    }
    rr = error_block_sum<BINS_WAVES>(rr, wsum);
    hr = error_block_sum<BINS_WAVES>(hr, wsum);
    const double k = 2.0 / s;
    for (int b = t; b < bins; b += BINS_BLOCK) {
      const double h = ((double)hq[b] / 4294967296.0) / s;
      const double r = h - goal[b];
      pull[b] = k * (r - h * hr);
    }
    e_hist = rr;
  }
  if (t == 0) {
    const double e = e_hist + pen;
    error_out[0] = e;
    error_out[1] = 1.0;   // one error term: the reported mean is the sum
    error_out[2] = e;
  }
}

// WEIGHTED: gx, gy times w last, in front of the chain rule.
template <typename T, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_density_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    DensityArgs<WEIGHTED> g, const double* __restrict__ pull, double* __restrict__ grad,
    int64_t grad_stride) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  LinkDir<DIM> link;
  double w = 0.0;
  const DensityRay r = density_classify<T, DIM, WEIGHTED>(rows, stride, mask, i, g, link, w);
  const bool two = g.row_y >= 0;
  double gx = 0.0, gy = 0.0;
  if (r.kind == 2) {
    gx = weighed<WEIGHTED>(g.oob * (2.0 * r.tx) * r.dx, w);
    gy = weighed<WEIGHTED>(g.oob * (2.0 * r.ty) * r.dy, w);
  } else if (r.kind == 1) {
    if (two) {
      const double d00 = pull[r.ja * g.nx + r.ia], d01 = pull[r.ja * g.nx + r.ib];
      const double d10 = pull[r.jb * g.nx + r.ia], d11 = pull[r.jb * g.nx + r.ib];
      gx = weighed<WEIGHTED>(g.sx * ((1.0 - r.ty) * (d01 - d00) + r.ty * (d11 - d10)), w);
      gy = weighed<WEIGHTED>(g.sy * ((1.0 - r.tx) * (d10 - d00) + r.tx * (d11 - d01)), w);
    } else {
      gx = weighed<WEIGHTED>(g.sx * (pull[r.ib] - pull[r.ia]), w);
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

}  // namespace tfrt

using namespace tfrt;

extern "C" size_t tfrt_density_error_workspace_bytes(int64_t n, int32_t nx, int32_t ny);

// Every entry behind its own checks of the rows / codes: `dim` 2 or 3, codes below 3 * dim.
// `wt` null: unweighted.
static int density_error_run(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                             int32_t dim, const int32_t* mask, int32_t row_x, int32_t row_y,
                             const double* goal, int32_t nx, int32_t ny, double x0, double x1,
                             double sx, double y0, double y1, double sy, double oob_weight,
                             double* grad, int64_t grad_stride, double* error_out, int64_t* hq,
                             int32_t splat_variant, void* workspace, size_t workspace_bytes,
                             void* stream, const DensityWeights* wt = nullptr) {
  if (nx < 1 || ny < 1 || (int64_t)nx * ny > DENSITY_MAX_BINS || !goal || (row_y < 0 && ny != 1) ||
      !error_args_ok(rows, stride, n, state_dtype, row_x, row_y, x0, x1, sx, y0, y1, sy,
                     oob_weight, grad, grad_stride, error_out, hq, splat_variant, workspace))
    return TFRT_E_BADARG;
  const int bins = nx * ny;
  if (splat_variant == 1 && bins > DENSITY_LDS_BINS) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_density_error_workspace_bytes(n, nx, ny)) return TFRT_E_WORKSPACE;
  const bool lds = splat_variant == 1 || (splat_variant == 0 && bins <= DENSITY_LDS_BINS);

  DensityGrid g;
  g.x0 = x0, g.x1 = x1, g.sx = sx, g.oob = oob_weight;
  g.y0 = row_y >= 0 ? y0 : 0.0, g.y1 = row_y >= 0 ? y1 : 0.0, g.sy = row_y >= 0 ? sy : 0.0;
  g.nx = nx, g.ny = ny, g.row_x = row_x, g.row_y = row_y;
  double* pull = static_cast<double*>(workspace);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) +
                                              align_up((size_t)bins * sizeof(double)));
  unsigned long long* hqu = reinterpret_cast<unsigned long long*>(hq);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, DENSITY_RAYS_PER_BLOCK, DENSITY_MAX_GRID);
  const int nblk = cdiv(n, BLOCK);

  hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(bins, BLOCK)), dim3(BLOCK), 0, st, hqu, bins);
  // the splat, the bins and the seed: rows of T, direction fields of a DIM-D block (0: none),
  // the constants `c` with or without weights
  auto launch = [&](auto tag, auto d, auto c) {
    using T = typename decltype(tag)::type;
    constexpr int DIM = decltype(d)::value;
    constexpr bool WEIGHTED = decltype(c)::weighted;
    const T* r = static_cast<const T*>(rows);
    if (grid > 0 && lds)
      hipLaunchKernelGGL((k_density_splat<T, true, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK),
                         (size_t)bins * sizeof(unsigned long long), st, r, stride, n, mask, c, hqu,
                         partial);
    else if (grid > 0)
      hipLaunchKernelGGL((k_density_splat<T, false, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK), 0, st,
                         r, stride, n, mask, c, hqu, partial);
    hipLaunchKernelGGL(k_density_bins, dim3(1), dim3(BINS_BLOCK), 0, st,
                       reinterpret_cast<const long long*>(hqu), goal, bins, partial, grid, pull,
                       error_out);
    if (nblk > 0)
      hipLaunchKernelGGL((k_density_seed<T, DIM, WEIGHTED>), dim3(nblk), dim3(BLOCK), 0, st, r,
                         stride, n, mask, c, pull, grad, grad_stride);
  };
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    dispatch_fields(dim, row_x, row_y, [&](auto d) {
      if (wt != nullptr)
        launch(tag, d, DensityArgs<true>{g, *wt});
      else
        launch(tag, d, DensityArgs<false>{g});
    });
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

extern "C" {

size_t tfrt_density_error_workspace_bytes(int64_t n, int32_t nx, int32_t ny) {
  if (n < 0 || nx < 1 || ny < 1 || (int64_t)nx * ny > DENSITY_MAX_BINS) return 0;
  return align_up((size_t)nx * ny * sizeof(double)) + align_up(DENSITY_MAX_GRID * sizeof(double));
}

int tfrt_density_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                       const int32_t* mask, int32_t row_x, int32_t row_y, const double* goal,
                       int32_t nx, int32_t ny, double x0, double x1, double sx, double y0,
                       double y1, double sy, double oob_weight, double* grad, int64_t grad_stride,
                       double* error_out, int64_t* hq, int32_t splat_variant, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (row_x < 0 || row_x > 5 || row_y < -1 || row_y > 5) return TFRT_E_BADARG;
  return density_error_run(rows, stride, n, state_dtype, 3, mask, row_x, row_y, goal, nx, ny, x0,
                           x1, sx, y0, y1, sy, oob_weight, grad, grad_stride, error_out, hq,
                           splat_variant, workspace, workspace_bytes, stream);
}

int tfrt_density_error_fields(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                              int32_t dimension, const int32_t* mask, int32_t field_x,
                              int32_t field_y, const double* goal, int32_t nx, int32_t ny,
                              double x0, double x1, double sx, double y0, double y1, double sy,
                              double oob_weight, double* grad, int64_t grad_stride,
                              double* error_out, int64_t* hq, int32_t splat_variant,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  return density_error_run(rows, stride, n, state_dtype, dimension, mask, field_x, field_y, goal,
                           nx, ny, x0, x1, sx, y0, y1, sy, oob_weight, grad, grad_stride,
                           error_out, hq, splat_variant, workspace, workspace_bytes, stream);
}

int tfrt_density_error_weighted(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                                int32_t dimension, const int32_t* mask, int32_t field_x,
                                int32_t field_y, const double* goal, const double* weight,
                                int64_t n_source, const int32_t* perm, int32_t nx, int32_t ny,
                                double x0, double x1, double sx, double y0, double y1, double sy,
                                double oob_weight, double* grad, int64_t grad_stride,
                                double* error_out, int64_t* hq, int32_t splat_variant,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension || !weight || n_source < 0 || n_source > INT32_MAX)
    return TFRT_E_BADARG;
  DensityWeights wt;
  wt.weight = weight, wt.perm = perm, wt.n_source = n_source;
  return density_error_run(rows, stride, n, state_dtype, dimension, mask, field_x, field_y, goal,
                           nx, ny, x0, x1, sx, y0, y1, sy, oob_weight, grad, grad_stride,
                           error_out, hq, splat_variant, workspace, workspace_bytes, stream, &wt);
}

}  // extern "C"
