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
//   k_error_clear      zeroes the records.  A launch, not a memset node: why, at the kernel
//                      (error_sums.h).
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
// {W, Xhi, Xlo, Yhi, Ylo, count, 0, 0}.  The accumulate, the seed and the classification they share
// have a `bool WEIGHTED` template parameter: everything that touches the weight stands under
// `if constexpr (WEIGHTED)`, the weights are a base of the kernels' constants that is empty without
// them (SpotArgs), so the unweighted instantiations neither receive nor read a weight, and
// SpotRecord<WEIGHTED> says once how many slots a record has and where slot p of a group lies, in
// the LDS table and in global memory.  The weight is read once per column through `perm`, behind
// the index check that the label lookup needs anyway.  The table in LDS has six planes of G
// int64: SPOT_WEIGHTED_LDS_GROUPS = 512 keeps it at the 24 KiB of the unweighted table at 1,024
// groups -- six workgroups, 24 waves, share a CU's 160 KiB; twice the table would leave three, too
// few to hide the latency of the ds_add_u64 behind other waves' loads.  More groups: six global
// 64-bit atomics, all in the ray's one line.
//
// What this file shares with tfrt_density.hip -- the fixed-shape workgroup sums, the clear kernel,
// the out-of-domain axis, the grid sizes, the argument checks, the dispatch on the direction
// fields -- is in error_sums.h.  What it shares with tfrt_distortion.hip -- the records, the
// classification and the accumulate launch -- is in spot_records.h.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "spot_records.h"

namespace tfrt {

// WEIGHTED: the centroid from the two limbs, everything times wr last.
template <typename T, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_spot_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotArgs<WEIGHTED> g,
    const long long* __restrict__ acc, double* __restrict__ grad, int64_t grad_stride,
    double* __restrict__ term_partial) {
#pragma clang fp contract(off)
  using Record = SpotRecord<WEIGHTED>;
  __shared__ double wsum[WAVES];
  const bool two = g.row_y >= 0;
  double terms = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq = 0.0, wr = 0.0;
    const SpotRay r =
        spot_classify<T, DIM, WEIGHTED>(rows, stride, mask, group, perm, i, g, link, wq, wr);
    double gx = 0.0, gy = 0.0;
    if (r.kind == 2) {
      gx = weighed<WEIGHTED>(g.oob * (2.0 * r.x) * r.dx, wr);
      gy = weighed<WEIGHTED>(g.oob * (2.0 * r.y) * r.dy, wr);
    } else if (r.kind == 1) {
      // (this ray is in its own group's record: its mass is >= 1)
      const long long* rec = acc + Record::SLOTS * (int64_t)r.label;
      const double mass = (double)rec[0];
      const double cx = g.x0 + (Record::moment(rec, 0, g) / mass) / g.qsx;
      const double dx = r.x - cx;
      gx = weighed<WEIGHTED>(2.0 * dx, wr);
      double t = weighed<WEIGHTED>(dx * dx, wr);
      if (two) {
        const double cy = g.y0 + (Record::moment(rec, 1, g) / mass) / g.qsy;
        const double dy = r.y - cy;
        gy = weighed<WEIGHTED>(2.0 * dy, wr);
        t = t + weighed<WEIGHTED>(dy * dy, wr);
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
  const double s = error_block_sum<WAVES>(terms, wsum);
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
  inside = error_block_sum<FINISH_WAVES>(inside, wsum);
  pen = error_block_sum<FINISH_WAVES>(pen, wsum);
  counting = error_block_sum<FINISH_WAVES>(counting, wcnt);
  if (t == 0) {
    const double e = inside + pen;
    const double terms = (double)(counting * fields);
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = counting > 0 ? e / terms : __builtin_nan("");
  }
}

}  // namespace tfrt

using namespace tfrt;

extern "C" size_t tfrt_spot_error_workspace_bytes(int64_t n, int32_t n_groups);

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
  if (n_source < 0 || n_source > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS ||
      qbits < 1 || qbits > 52 || !group ||
      !error_args_ok(rows, stride, n, state_dtype, row_x, row_y, x0, x1, qsx, y0, y1, qsy,
                     oob_weight, grad, grad_stride, error_out, acc, variant, workspace))
    return TFRT_E_BADARG;
  if (weighted) {
    // every sum stays below n * 2^wbits * 2^ceil(qbits / 2) < 2^62
    if (wbits < 1 || wbits > SPOT_MAX_WBITS) return TFRT_E_BADARG;
    if (n >= ((int64_t)1 << (62 - wbits - (qbits + 1) / 2))) return TFRT_E_BADARG;
  } else if (n >= ((int64_t)1 << (62 - qbits))) {
    return TFRT_E_BADARG;   // n * 2^qbits must stay below 2^62
  }
  const int lds_groups = weighted ? SPOT_WEIGHTED_LDS_GROUPS : SPOT_LDS_GROUPS;
  if (variant == 1 && n_groups > lds_groups) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_spot_error_workspace_bytes(n, n_groups)) return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= lds_groups);

  SpotGrid g;
  g.x0 = x0, g.x1 = x1, g.qsx = qsx, g.oob = oob_weight;
  g.y0 = row_y >= 0 ? y0 : 0.0, g.y1 = row_y >= 0 ? y1 : 0.0, g.qsy = row_y >= 0 ? qsy : 0.0;
  g.qmax = ldexp(1.0, qbits);
  g.n_source = n_source, g.n_groups = n_groups, g.row_x = row_x, g.row_y = row_y;
  SpotWeights w;
  w.weight = weight, w.one = ldexp(1.0, wbits), w.inv = ldexp(1.0, -wbits), w.h = qbits / 2;
  const int slots = weighted ? SpotRecord<true>::SLOTS : SpotRecord<false>::SLOTS;
  char* ws = static_cast<char*>(workspace);
  double* pen_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial =
      reinterpret_cast<long long*>(ws + align_up(SPOT_MAX_GRID * sizeof(double)));
  double* term_partial =
      reinterpret_cast<double*>(ws + 2 * align_up(SPOT_MAX_GRID * sizeof(double)));
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, SPOT_RAYS_PER_BLOCK, SPOT_MAX_GRID);
  const int sgrid = error_grid(n, BLOCK, SPOT_SEED_MAX_GRID);   // one column per lane up to 2M

  hipLaunchKernelGGL(k_error_clear<>, dim3(cdiv(slots * (int64_t)n_groups, BLOCK)), dim3(BLOCK), 0,
                     st, accu, slots * n_groups);
  // the accumulate and the seed: rows of T, direction fields of a DIM-D block (0: none), the
  // constants `c` with or without weights
  auto launch = [&](auto tag, auto d, auto c) {
    using T = typename decltype(tag)::type;
    constexpr int DIM = decltype(d)::value;
    constexpr bool WEIGHTED = decltype(c)::weighted;
    const T* r = static_cast<const T*>(rows);
    if (lds)
      hipLaunchKernelGGL((k_spot_accumulate<T, true, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK),
                         (size_t)n_groups * SpotRecord<WEIGHTED>::PLANES * sizeof(unsigned long long),
                         st, r, stride, n, mask, group, perm, c, accu, pen_partial, cnt_partial);
    else
      hipLaunchKernelGGL((k_spot_accumulate<T, false, DIM, WEIGHTED>), dim3(grid), dim3(BLOCK), 0,
                         st, r, stride, n, mask, group, perm, c, accu, pen_partial, cnt_partial);
    hipLaunchKernelGGL((k_spot_seed<T, DIM, WEIGHTED>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride,
                       n, mask, group, perm, c, reinterpret_cast<const long long*>(accu), grad,
                       grad_stride, term_partial);
  };
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    if (grid > 0)
      dispatch_fields(dim, row_x, row_y, [&](auto d) {
        if (weighted)
          launch(tag, d, SpotArgs<true>{g, w});
        else
          launch(tag, d, SpotArgs<false>{g});
      });
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
