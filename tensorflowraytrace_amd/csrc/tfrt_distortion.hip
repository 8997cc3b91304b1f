// DistortionError: the centroids of the groups must be a scaled (or affine) copy of the object --
// at whatever magnification and offset the lens gives.
//
// Every source ray carries a group label and every group an object point p_g.  The finished rays
// of a group have the centroid c_g of SpotError; a least-squares fit c ~ A p + t over the groups
// (weights: the groups' ray counts; A = M I, or a free k x k matrix) gives every group a target
// A p_g + t, and the error is the sum over the rays of the squared distance of their group's
// centroid from its target, plus SpotError's penalty for rays outside the domain.  The definition,
// operation by operation, is in include/tfrt_hip.h at tfrt_distortion_error; the per-group
// arithmetic is in distortion_math.h; tests/distortion_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: the records are SpotError's int64 sums, and every
// floating-point sum over the groups has a fixed shape and order (thread j of the one workgroup
// takes the groups j, j + B, ... in ascending order, then error_block_sum).  No float atomics,
// nothing waits on another workgroup.
//
// The gradient needs no derivative of the fit, because (A, t) minimises the error: a ray of group
// g gets 2 r_g, r_g = c_g - (A p_g + t), as d/dx_i of count_g |c_g - target_g|^2 with
// d c_g / d x_i = 1 / count_g.
//
// Four launches:
//
//   k_error_clear       zeroes the records (error_sums.h says why it is a launch).
//   k_spot_accumulate   spot_records.h: tfrt_spot_error's unweighted accumulate launch, the same
//                       two variants.
//   k_distortion_fit    ONE workgroup, three passes over the groups, each group recomputed from
//                       its record: the weighted means; the moments Spp, Scp and the fit; the
//                       (G, 2) residual table and the inside error.  Then the accumulate launch's
//                       partials in index order, {sum, terms, mean} and the fit's parameters.
//   k_distortion_seed   residual_seed.h (shared with tfrt_centroid.hip): one lane per column (a
//                       fixed grid for n, grid-stride): the same classification, one 16-byte load
//                       of the group's residual, the gradient rows of EVERY column (zeros where a
//                       ray does not count).
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "spot_records.h"
#include "distortion_math.h"
#include "residual_seed.h"

namespace tfrt {

struct DistortionFitArgs {
  DistortionGrid grid;
  double min_cond;
  int32_t n_groups, k, fit_kind, fields;
};

// the group `k` from its record and its row of `points`
__device__ __forceinline__ DistortionGroup distortion_load(const long long* __restrict__ acc,
                                                           const double* __restrict__ points,
                                                           int k, const DistortionFitArgs& a) {
  int64_t rec[3];
  const long long* at = acc + SpotRecord<false>::SLOTS * (int64_t)k;
  rec[0] = at[0], rec[1] = at[1], rec[2] = at[2];
  return distortion_group(rec, points + (int64_t)a.k * k, a.grid);
}

// One workgroup of FINISH_BLOCK threads.  Thread t owns the groups (and then the partials) t,
// t + 1024, ... (summed in that order), then the fixed-shape workgroup sum: the same bits on every
// run, and every thread holds the same sums.
__global__ __launch_bounds__(FINISH_BLOCK) void k_distortion_fit(
    const long long* __restrict__ acc, const double* __restrict__ points, DistortionFitArgs a,
    const double* __restrict__ pen_partial, const long long* __restrict__ cnt_partial, int n_acc,
    double* __restrict__ residual, double* __restrict__ fit_out, double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FINISH_WAVES];
  __shared__ long long wcnt[FINISH_WAVES];
  const int t = threadIdx.x;
  const int G = a.n_groups;

  // first pass: the weighted means
  double mean[DISTORTION_MEAN_SUMS];
  for (int e = 0; e < DISTORTION_MEAN_SUMS; ++e) mean[e] = 0.0;
  long long used = 0;
  for (int k = t; k < G; k += FINISH_BLOCK) {
    const DistortionGroup q = distortion_load(acc, points, k, a);
    if (!q.used) continue;
    distortion_mean_terms(q, mean);
    used += 1;
  }
  for (int e = 0; e < DISTORTION_MEAN_SUMS; ++e)
    mean[e] = error_block_sum<FINISH_WAVES>(mean[e], wsum);
  used = error_block_sum<FINISH_WAVES>(used, wcnt);
  double m[4];
  distortion_means(mean, m);

  // second pass: the moments about the means, and the fit
  double S[DISTORTION_MOMENT_SUMS];
  for (int e = 0; e < DISTORTION_MOMENT_SUMS; ++e) S[e] = 0.0;
  for (int k = t; k < G; k += FINISH_BLOCK) {
    const DistortionGroup q = distortion_load(acc, points, k, a);
    if (q.used) distortion_moment_terms(q, m, S);
  }
  for (int e = 0; e < DISTORTION_MOMENT_SUMS; ++e) S[e] = error_block_sum<FINISH_WAVES>(S[e], wsum);
  double fit[DISTORTION_FIT_OUT];
  const bool valid = distortion_fit(S, m, used, a.fit_kind, a.grid.two, a.min_cond, fit);

  // third pass: the residual table and the inside error
  double inside[2] = {0.0, 0.0};
  for (int k = t; k < G; k += FINISH_BLOCK) {
    const DistortionGroup q = distortion_load(acc, points, k, a);
    double r[2];
    distortion_residual(q, m, fit, valid, r, inside);
    residual[2 * (int64_t)k] = r[0];
    residual[2 * (int64_t)k + 1] = r[1];
  }
  const double ex = error_block_sum<FINISH_WAVES>(inside[0], wsum);
  const double ey = error_block_sum<FINISH_WAVES>(inside[1], wsum);

  // the accumulate launch's partials, in index order
  double pen = 0.0;
  long long counting = 0;
  for (int b = t; b < n_acc; b += FINISH_BLOCK) {
    pen += pen_partial[b];
    counting += cnt_partial[b];
  }
  pen = error_block_sum<FINISH_WAVES>(pen, wsum);
  counting = error_block_sum<FINISH_WAVES>(counting, wcnt);
  if (t == 0) {
    const double e = (ex + ey) + pen;
    const double terms = (double)(counting * a.fields);
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = counting > 0 ? e / terms : __builtin_nan("");
    for (int p = 0; p < DISTORTION_FIT_OUT; ++p) fit_out[p] = fit[p];
  }
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_distortion_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS) return 0;
  return 2 * align_up(SPOT_MAX_GRID * sizeof(double));
}

int tfrt_distortion_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                          int32_t dimension, const int32_t* mask, int32_t field_x,
                          int32_t field_y, const int32_t* group, int64_t n_source,
                          const int32_t* perm, int32_t n_groups, const double* points,
                          int32_t fit_kind, double min_cond, double x0, double x1, double qsx,
                          double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                          double* grad, int64_t grad_stride, double* error_out, double* fit_out,
                          double* residual, int64_t* acc, int32_t variant, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  if (n_source < 0 || n_source > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS ||
      qbits < 1 || qbits > 52 || !group || !points || !fit_out || !residual ||
      (reinterpret_cast<uintptr_t>(residual) & 15u) != 0 ||
      (fit_kind != DISTORTION_FIT_SCALE && fit_kind != DISTORTION_FIT_AFFINE) ||
      !(min_cond >= 0.0) || !isfinite(min_cond) ||
      !error_args_ok(rows, stride, n, state_dtype, field_x, field_y, x0, x1, qsx, y0, y1, qsy,
                     oob_weight, grad, grad_stride, error_out, acc, variant, workspace))
    return TFRT_E_BADARG;
  if (n >= ((int64_t)1 << (62 - qbits))) return TFRT_E_BADARG;   // n * 2^qbits stays below 2^62
  if (variant == 1 && n_groups > SPOT_LDS_GROUPS) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_distortion_error_workspace_bytes(n, n_groups))
    return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= SPOT_LDS_GROUPS);
  const bool two = field_y >= 0;

  SpotGrid sg;
  sg.x0 = x0, sg.x1 = x1, sg.qsx = qsx, sg.oob = oob_weight;
  sg.y0 = two ? y0 : 0.0, sg.y1 = two ? y1 : 0.0, sg.qsy = two ? qsy : 0.0;
  sg.qmax = ldexp(1.0, qbits);
  sg.n_source = n_source, sg.n_groups = n_groups, sg.row_x = field_x, sg.row_y = field_y;
  const SpotArgs<false> g{sg};
  DistortionFitArgs fa;
  fa.grid.x0 = sg.x0, fa.grid.qsx = sg.qsx, fa.grid.y0 = sg.y0, fa.grid.qsy = sg.qsy;
  fa.grid.two = two;
  fa.min_cond = min_cond;
  fa.n_groups = n_groups, fa.k = two ? 2 : 1, fa.fit_kind = fit_kind, fa.fields = two ? 2 : 1;

  char* ws = static_cast<char*>(workspace);
  double* pen_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial =
      reinterpret_cast<long long*>(ws + align_up(SPOT_MAX_GRID * sizeof(double)));
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  const long long* accs = reinterpret_cast<const long long*>(acc);
  const double2* res2 = reinterpret_cast<const double2*>(residual);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, SPOT_RAYS_PER_BLOCK, SPOT_MAX_GRID);
  const int sgrid = error_grid(n, BLOCK, DISTORTION_SEED_MAX_GRID);
  constexpr int slots = SpotRecord<false>::SLOTS;

  hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(slots * (int64_t)n_groups, BLOCK)), dim3(BLOCK), 0,
                     st, accu, slots * n_groups);
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const T* r = static_cast<const T*>(rows);
    dispatch_fields(dimension, field_x, field_y, [&](auto d) {
      constexpr int DIM = decltype(d)::value;
      if (grid > 0) {
        if (lds)
          hipLaunchKernelGGL((k_spot_accumulate<T, true, DIM, false>), dim3(grid), dim3(BLOCK),
                             (size_t)n_groups * SpotRecord<false>::PLANES *
                                 sizeof(unsigned long long),
                             st, r, stride, n, mask, group, perm, g, accu, pen_partial,
                             cnt_partial);
        else
          hipLaunchKernelGGL((k_spot_accumulate<T, false, DIM, false>), dim3(grid), dim3(BLOCK), 0,
                             st, r, stride, n, mask, group, perm, g, accu, pen_partial,
                             cnt_partial);
      }
      hipLaunchKernelGGL(k_distortion_fit, dim3(1), dim3(FINISH_BLOCK), 0, st, accs, points, fa,
                         pen_partial, cnt_partial, grid, residual, fit_out, error_out);
      if (sgrid > 0)
        hipLaunchKernelGGL((k_distortion_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride,
                           n, mask, group, perm, g, res2, grad, grad_stride);
    });
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
