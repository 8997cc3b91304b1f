// FocusError: rays that left the same object point, taken as LINES, must pass through one common
// point of space -- wherever along the beam that is.
//
// Every source ray carries a group label; the finished ray's last link is a line (its end point e
// and the direction u of direction_fields.h).  The point x that minimises the sum over a group's
// lines of the squared distance |P (e - x)|^2, P = I - u u^T, solves (sum P) x = sum P e: a d x d
// system per group.  The error is the sum over the rays of that squared distance to the FOCUS of
// the ray's own group.  The definition, operation by operation, is in include/tfrt_hip.h at
// tfrt_focus_error; the arithmetic is in focus_math.h; tests/focus_error_reference.py restates it
// in numpy.
//
// Bit-reproducible by construction: the entries of P and of t = P m (m the end point, normalised
// into the unit box) enter the group's record as the INTEGERS rint(. * 2^pbits) with
// n * 2^pbits <= 2^60: int64 sums that cannot overflow and do not depend on the order in which
// the atomics land.  Every floating-point reduction has a fixed shape and order.  No float
// atomics and no compare-and-swap loop anywhere; nothing waits on another workgroup.
//
// The gradient needs no derivative of the focus, because the focus minimises the group's sum: it
// is the lever rule of the foot point e - alpha u along the link.
//
// Five launches:
//
//   k_error_clear      zeroes the records (error_sums.h says why it is a launch).
//   k_focus_accumulate focus_records.h (tfrt_flatfield.hip fills the same records): one lane per
//                      column (a fixed grid for n, grid-stride): the ten slots of focus_record ->
//                      the record of the ray's group.  Two variants:
//                      <true>  G <= FOCUS_LDS_GROUPS: a per-workgroup table in LDS (ds_add_u64),
//                              ten planes of G int64 (80 B x 256 = 20 KiB, inside the 24 KiB that
//                              tfrt_spot.hip argues for), flushed with one global atomic per
//                              non-zero entry.
//                      <false> more groups: ten global 64-bit atomics (six plus the count in 2-D),
//                              all in the ray's own 80-byte record.
//   k_focus_solve      one lane per group: focus_solve -> the (G, 4) table {x, y, z, has_focus}.
//   k_focus_seed       one lane per column (a fixed grid for n, grid-stride): the same
//                      classification, the focus of the ray's own group from the table, all 2 d
//                      gradient rows of EVERY column (zeros where a ray has no term), the terms and
//                      their number as one partial each per workgroup.
//   k_focus_finish     ONE workgroup: the partials in index order, {sum, terms, mean}.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "focus_math.h"
#include "focus_records.h"

namespace tfrt {

constexpr int FOCUS_SEED_MAX_GRID = 2048;   // workgroups of the seed launch
constexpr int FOCUS_FINISH_BLOCK = 1024;
constexpr int FOCUS_FINISH_WAVES = FOCUS_FINISH_BLOCK / 64;

template <int DIM>
__global__ __launch_bounds__(BLOCK) void k_focus_solve(const long long* __restrict__ acc, int G,
                                                       double inv, double min_det,
                                                       double* __restrict__ foci) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= G) return;
  int64_t rec[FOCUS_SLOTS];
#pragma unroll
  for (int p = 0; p < FOCUS_SLOTS; ++p) rec[p] = acc[FOCUS_SLOTS * (int64_t)k + p];
  double x[3];
  bool has;
  focus_solve<DIM>(rec, inv, min_det, x, has);
  foci[4 * (int64_t)k + 0] = x[0];
  foci[4 * (int64_t)k + 1] = x[1];
  foci[4 * (int64_t)k + 2] = x[2];
  foci[4 * (int64_t)k + 3] = has ? 1.0 : 0.0;
}

template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_focus_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, FocusArgs g,
    const double* __restrict__ foci, double* __restrict__ grad, int64_t grad_stride,
    double* __restrict__ term_partial, long long* __restrict__ cnt_partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  double terms = 0.0;
  long long count = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    const int label = focus_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
    double gs[DIM], ge[DIM];
#pragma unroll
    for (int b = 0; b < DIM; ++b) gs[b] = ge[b] = 0.0;
    if (label >= 0) {
      const double* f = foci + 4 * (int64_t)label;
      if (f[3] != 0.0) {
        double m[DIM], x[3];
        x[0] = f[0], x[1] = f[1], x[2] = f[2];
        focus_normalise<DIM>(link.e, g.box, m);
        terms += focus_term<DIM>(link.d, m, x, g.box.R, link.L, gs, ge);
        count += 1;
      }
    }
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      grad[(int64_t)b * grad_stride + i] = gs[b];
      grad[(int64_t)(DIM + b) * grad_stride + i] = ge[b];
    }
  }
  const double s = error_block_sum<WAVES>(terms, wsum);
  const long long c = error_block_sum<WAVES>(count, wcnt);
  if (threadIdx.x == 0) {
    term_partial[blockIdx.x] = s;
    cnt_partial[blockIdx.x] = c;
  }
}

// One workgroup.  Thread t owns partials t, t + 1024, ... (summed in that order), then the
// fixed-shape workgroup sum: the same bits on every run.
__global__ __launch_bounds__(FOCUS_FINISH_BLOCK) void k_focus_finish(
    const double* __restrict__ term_partial, const long long* __restrict__ cnt_partial, int n_seed,
    double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FOCUS_FINISH_WAVES];
  __shared__ long long wcnt[FOCUS_FINISH_WAVES];
  const int t = threadIdx.x;
  double e = 0.0;
  long long count = 0;
  for (int b = t; b < n_seed; b += FOCUS_FINISH_BLOCK) {
    e += term_partial[b];
    count += cnt_partial[b];
  }
  e = error_block_sum<FOCUS_FINISH_WAVES>(e, wsum);
  count = error_block_sum<FOCUS_FINISH_WAVES>(count, wcnt);
  if (t == 0) {
    const double terms = (double)count;
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = count > 0 ? e / terms : __builtin_nan("");
  }
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_focus_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > FOCUS_MAX_GROUPS) return 0;
  return 2 * align_up(FOCUS_SEED_MAX_GRID * sizeof(double));
}

int tfrt_focus_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                     int32_t dimension, const int32_t* mask, const int32_t* group,
                     int64_t n_source, const int32_t* perm, int32_t n_groups, double x0, double x1,
                     double y0, double y1, double z0, double z1, int32_t pbits, double min_det,
                     double* grad, int64_t grad_stride, double* error_out, int64_t* acc,
                     double* foci, int32_t variant, void* workspace, size_t workspace_bytes,
                     void* stream) {
  const double domain[6] = {x0, x1, y0, y1, z0, z1};
  FocusArgs g;
  if (focus_args(rows, stride, n, state_dtype, dimension, group, n_source, n_groups, domain, pbits,
                 min_det, grad, grad_stride, error_out, acc, foci, variant, workspace, g) != 0)
    return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_focus_error_workspace_bytes(n, n_groups)) return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= FOCUS_LDS_GROUPS);
  const double inv = ldexp(1.0, -pbits);

  char* ws = static_cast<char*>(workspace);
  double* term_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial =
      reinterpret_cast<long long*>(ws + align_up(FOCUS_SEED_MAX_GRID * sizeof(double)));
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  const long long* accs = reinterpret_cast<const long long*>(acc);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int sgrid = error_grid(n, BLOCK, FOCUS_SEED_MAX_GRID);

  auto launch = [&](auto tag, auto d) {
    using T = typename decltype(tag)::type;
    constexpr int DIM = decltype(d)::value;
    const T* r = static_cast<const T*>(rows);
    focus_fill_records<T, DIM>(r, stride, n, mask, group, perm, g, lds, accu, st);
    hipLaunchKernelGGL((k_focus_solve<DIM>), dim3(cdiv(n_groups, BLOCK)), dim3(BLOCK), 0, st, accs,
                       n_groups, inv, min_det, foci);
    if (sgrid > 0)
      hipLaunchKernelGGL((k_focus_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride, n,
                         mask, group, perm, g, foci, grad, grad_stride, term_partial, cnt_partial);
  };
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    if (dimension == 3)
      launch(tag, dim_tag<3>{});
    else
      launch(tag, dim_tag<2>{});
    hipLaunchKernelGGL(k_focus_finish, dim3(1), dim3(FOCUS_FINISH_BLOCK), 0, st, term_partial,
                       cnt_partial, sgrid, error_out);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
