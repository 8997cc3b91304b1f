// CentroidError: the centroid of every group of rays must lie at a given target (`targets`), or the
// centroids of the groups of one parent must coincide, wherever they do (`parents`) -- without
// charging the spread of a group.
//
// Every source ray carries a group label.  The finished rays of a group have the centroid c_g of
// SpotError; its target t_g is its row of `targets`, or the centroid C_p of its parent's record --
// the INTEGER sum of the records of the parent's groups.  The error is the sum over the rays of the
// squared distance of their group's centroid from its target, plus SpotError's penalty for rays
// outside the domain.  The definition, operation by operation, is in include/tfrt_hip.h at
// tfrt_centroid_error; the per-group arithmetic is in centroid_math.h;
// tests/centroid_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: the records and the parents' records are int64 sums (integer
// addition is associative: atomics in any order give the same bits), and every floating-point sum
// over the groups has the fixed shape and order of k_distortion_fit.  No float atomics, nothing
// waits on another workgroup.
//
// The gradient needs no derivative of a centroid: a ray of group g gets 2 r_g, r_g = c_g - t_g, as
// d/dx_i of count_g |c_g - t_g|^2 with d c_g / d x_i = 1 / count_g; and C_p minimises the sum of
// its groups' terms, so its own derivative drops out.
//
// Four launches with `targets`, five with `parents`:
//
//   k_error_clear       zeroes the records (error_sums.h says why it is a launch); with parents
//                       k_centroid_clear, the same store over both tables in one launch.
//   k_spot_accumulate   spot_records.h: tfrt_spot_error's unweighted accumulate launch, the same
//                       two variants.
//   k_centroid_parents  parents only.  One lane per group: the record of a group with rays and a
//                       legal parent label is added to its parent's record by int64 atomics.  A
//                       launch of its own: the kernel boundary makes the sums visible to the next.
//   k_centroid_table    ONE workgroup, one pass over the groups, each from its record: the (G, 2)
//                       residual table and the inside error.  Then the accumulate launch's partials
//                       in index order, {sum, terms, mean} and {groups_used, parents_used}.
//   k_distortion_seed   residual_seed.h (shared with tfrt_distortion.hip): one 16-byte load of the
//                       group's residual per ray inside, the gradient rows of EVERY column.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "spot_records.h"
#include "centroid_math.h"
#include "residual_seed.h"

namespace tfrt {

constexpr int CENTROID_SLOTS = SpotRecord<false>::SLOTS;   // a parent's record has a group's layout

struct CentroidTableArgs {
  CentroidGrid grid;
  int32_t n_groups, n_parents, k, fields;
};

// k_error_clear over two tables in one launch (parents mode: the groups' and the parents' records)
__global__ __launch_bounds__(BLOCK) void k_centroid_clear(unsigned long long* __restrict__ a,
                                                          int entries_a,
                                                          unsigned long long* __restrict__ b,
                                                          int entries_b) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e < entries_a)
    a[e] = 0ull;
  else if (e - entries_a < entries_b)
    b[e - entries_a] = 0ull;
}

// One lane per group: {count, Sx, Sy} of a group with rays and a legal parent label -> the record
// of its parent.  Nothing is read or written out of bounds, whatever `parents` holds.
__global__ __launch_bounds__(BLOCK) void k_centroid_parents(
    const long long* __restrict__ acc, const int32_t* __restrict__ parents, int n_groups,
    int n_parents, bool two, unsigned long long* __restrict__ parent_acc) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n_groups) return;
  const long long* at = acc + CENTROID_SLOTS * (int64_t)k;
  const long long count = at[0];
  if (count <= 0) return;
  const int32_t p = parents[k];
  if (!centroid_parent_ok(p, n_parents)) return;
  unsigned long long* to = parent_acc + CENTROID_SLOTS * (int64_t)p;
  atomicAdd(to + 0, (unsigned long long)count);
  atomicAdd(to + 1, (unsigned long long)at[1]);
  if (two) atomicAdd(to + 2, (unsigned long long)at[2]);
}

__device__ __forceinline__ CentroidRecord centroid_load(const long long* __restrict__ table,
                                                        int k, const CentroidGrid& g) {
  int64_t rec[3];
  const long long* at = table + CENTROID_SLOTS * (int64_t)k;
  rec[0] = at[0], rec[1] = at[1], rec[2] = at[2];
  return centroid_record(rec, g);
}

// One workgroup of FINISH_BLOCK threads.  Thread t owns the groups (and then the parents and the
// partials) t, t + 1024, ... (summed in that order), then the fixed-shape workgroup sum: the same
// bits on every run.  `targets` or (`parents`, `parent_acc`): the mode.
__global__ __launch_bounds__(FINISH_BLOCK) void k_centroid_table(
    const long long* __restrict__ acc, const double* __restrict__ targets,
    const int32_t* __restrict__ parents, const long long* __restrict__ parent_acc,
    CentroidTableArgs a, const double* __restrict__ pen_partial,
    const long long* __restrict__ cnt_partial, int n_acc, double* __restrict__ residual,
    double* __restrict__ used_out, double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FINISH_WAVES];
  __shared__ long long wcnt[FINISH_WAVES];
  __shared__ double tsum;
  __shared__ long long tcnt;
  const int t = threadIdx.x;
  const int G = a.n_groups;

  double inside[2] = {0.0, 0.0};
  long long used = 0;
  for (int k = t; k < G; k += FINISH_BLOCK) {
    const CentroidRecord q = centroid_load(acc, k, a.grid);
    double tg[2] = {0.0, 0.0};
    bool has = false;
    if (q.rays) {
      if (targets != nullptr) {
        has = centroid_target(targets + (int64_t)a.k * k, a.grid.two, tg);
      } else {
        const int32_t p = parents[k];
        if (centroid_parent_ok(p, a.n_parents)) {
          // (this group is in its parent's record: the parent has rays)
          const CentroidRecord Q = centroid_load(parent_acc, p, a.grid);
          has = Q.rays;
          tg[0] = Q.cx, tg[1] = Q.cy;
        }
      }
    }
    double r[2];
    used += centroid_residual(q, has, tg, r, inside) ? 1 : 0;
    residual[2 * (int64_t)k] = r[0];
    residual[2 * (int64_t)k + 1] = r[1];
  }
  const double ex = error_block_total<FINISH_WAVES>(inside[0], wsum, &tsum);
  const double ey = error_block_total<FINISH_WAVES>(inside[1], wsum, &tsum);
  used = error_block_total<FINISH_WAVES>(used, wcnt, &tcnt);

  long long parents_used = 0;
  if (targets == nullptr)
    for (int p = t; p < a.n_parents; p += FINISH_BLOCK)
      parents_used += parent_acc[CENTROID_SLOTS * (int64_t)p] > 0 ? 1 : 0;
  parents_used = error_block_total<FINISH_WAVES>(parents_used, wcnt, &tcnt);

  // the accumulate launch's partials, in index order
  double pen = 0.0;
  long long counting = 0;
  for (int b = t; b < n_acc; b += FINISH_BLOCK) {
    pen += pen_partial[b];
    counting += cnt_partial[b];
  }
  pen = error_block_total<FINISH_WAVES>(pen, wsum, &tsum);
  counting = error_block_total<FINISH_WAVES>(counting, wcnt, &tcnt);
  if (t == 0) {
    const double e = (ex + ey) + pen;
    const double terms = (double)(counting * a.fields);
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = counting > 0 ? e / terms : __builtin_nan("");
    used_out[0] = (double)used;
    used_out[1] = (double)parents_used;
  }
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_centroid_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS) return 0;
  return 2 * align_up(SPOT_MAX_GRID * sizeof(double));
}

int tfrt_centroid_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                        int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                        const int32_t* group, int64_t n_source, const int32_t* perm,
                        int32_t n_groups, const double* targets, const int32_t* parents,
                        int32_t n_parents, int64_t* parent_acc, double x0, double x1, double qsx,
                        double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                        double* grad, int64_t grad_stride, double* error_out, double* used_out,
                        double* residual, int64_t* acc, int32_t variant, void* workspace,
                        size_t workspace_bytes, void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  // exactly one mode: `targets`, or `parents` with its count and its record table
  if ((targets != nullptr) == (parents != nullptr)) return TFRT_E_BADARG;
  if (parents != nullptr && (!parent_acc || n_parents < 1 || n_parents > SPOT_MAX_GROUPS))
    return TFRT_E_BADARG;
  if (n_source < 0 || n_source > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS ||
      qbits < 1 || qbits > 52 || !group || !used_out || !residual ||
      (reinterpret_cast<uintptr_t>(residual) & 15u) != 0 ||
      !error_args_ok(rows, stride, n, state_dtype, field_x, field_y, x0, x1, qsx, y0, y1, qsy,
                     oob_weight, grad, grad_stride, error_out, acc, variant, workspace))
    return TFRT_E_BADARG;
  if (n >= ((int64_t)1 << (62 - qbits))) return TFRT_E_BADARG;   // n * 2^qbits stays below 2^62
  if (variant == 1 && n_groups > SPOT_LDS_GROUPS) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_centroid_error_workspace_bytes(n, n_groups))
    return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= SPOT_LDS_GROUPS);
  const bool two = field_y >= 0;
  const bool by_parent = parents != nullptr;

  SpotGrid sg;
  sg.x0 = x0, sg.x1 = x1, sg.qsx = qsx, sg.oob = oob_weight;
  sg.y0 = two ? y0 : 0.0, sg.y1 = two ? y1 : 0.0, sg.qsy = two ? qsy : 0.0;
  sg.qmax = ldexp(1.0, qbits);
  sg.n_source = n_source, sg.n_groups = n_groups, sg.row_x = field_x, sg.row_y = field_y;
  const SpotArgs<false> g{sg};
  CentroidTableArgs ta;
  ta.grid.x0 = sg.x0, ta.grid.qsx = sg.qsx, ta.grid.y0 = sg.y0, ta.grid.qsy = sg.qsy;
  ta.grid.two = two;
  ta.n_groups = n_groups, ta.n_parents = by_parent ? n_parents : 0;
  ta.k = two ? 2 : 1, ta.fields = two ? 2 : 1;

  char* ws = static_cast<char*>(workspace);
  double* pen_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial =
      reinterpret_cast<long long*>(ws + align_up(SPOT_MAX_GRID * sizeof(double)));
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  const long long* accs = reinterpret_cast<const long long*>(acc);
  unsigned long long* paccu = reinterpret_cast<unsigned long long*>(parent_acc);
  const long long* paccs = reinterpret_cast<const long long*>(parent_acc);
  const double2* res2 = reinterpret_cast<const double2*>(residual);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, SPOT_RAYS_PER_BLOCK, SPOT_MAX_GRID);
  const int sgrid = error_grid(n, BLOCK, DISTORTION_SEED_MAX_GRID);
  constexpr int slots = CENTROID_SLOTS;

  if (by_parent)
    hipLaunchKernelGGL(k_centroid_clear,
                       dim3(cdiv(slots * ((int64_t)n_groups + n_parents), BLOCK)), dim3(BLOCK), 0,
                       st, accu, slots * n_groups, paccu, slots * n_parents);
  else
    hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(slots * (int64_t)n_groups, BLOCK)), dim3(BLOCK),
                       0, st, accu, slots * n_groups);
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
      if (by_parent)
        hipLaunchKernelGGL(k_centroid_parents, dim3(cdiv((int64_t)n_groups, BLOCK)), dim3(BLOCK),
                           0, st, accs, parents, n_groups, n_parents, two, paccu);
      hipLaunchKernelGGL(k_centroid_table, dim3(1), dim3(FINISH_BLOCK), 0, st, accs, targets,
                         parents, paccs, ta, pen_partial, cnt_partial, grid, residual, used_out,
                         error_out);
      if (sgrid > 0)
        hipLaunchKernelGGL((k_distortion_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride,
                           n, mask, group, perm, g, res2, grad, grad_stride);
    });
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
