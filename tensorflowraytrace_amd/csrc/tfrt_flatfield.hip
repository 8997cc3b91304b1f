// FlatFieldError: the foci of all groups must lie in ONE plane with a given normal -- wherever
// along the normal that plane has to stand.
//
// Every group of rays has FocusError's focus x_g = A_g^-1 b_g (the records, the classification and
// the cofactor solve are FocusError's, bit for bit).  With the unit normal a, a group's height is
// h_g = a . x_g; the plane's height hbar is the mean of the heights weighted by the groups' ray
// counts, and the error is the sum over the counting rays of the squared distance of their group's
// focus from that plane, in the scene's units.  The definition, operation by operation, is in
// include/tfrt_hip.h at tfrt_flatfield_error; the arithmetic is in flatfield_math.h;
// tests/flatfield_error_reference.py restates it in numpy.
//
// The gradient goes THROUGH the solved focus (the focus does not minimise this error): per group
// one adjoint vector mu_g = 2 R r_g A_g^-1 a, from which every ray of the group takes the lever
// rule of the part of mu across the ray plus a term from turning the ray.  The height hbar needs
// no derivative, because it minimises the sum.
//
// Bit-reproducible by construction: the records are FocusError's int64 sums, and every
// floating-point sum over the groups has a fixed shape and order (thread j of the one workgroup
// takes the groups j, j + B, ... in ascending order, then error_block_sum).  No float atomics,
// nothing waits on another workgroup, no finishing launch.
//
// Four launches:
//
//   k_error_clear      zeroes the records (error_sums.h says why it is a launch).
//   k_focus_accumulate focus_records.h: tfrt_focus_error's accumulate launch, the same two
//                      variants.
//   k_flatfield_fit    ONE workgroup, two passes over the groups, each group re-solved from its
//                      record: W, sum n h, the groups and the rays in use; then the (G, 8) table
//                      {x, used, mu, e_g}, the inside error, {sum, terms, mean} and the plane.
//   k_flatfield_seed   one lane per column (a fixed grid for n, grid-stride): the same
//                      classification, the 64-byte row of the ray's own group, all 2 d gradient
//                      rows of EVERY column (zeros where a ray has no term).
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "focus_records.h"
#include "flatfield_math.h"

namespace tfrt {

constexpr int FLATFIELD_SEED_MAX_GRID = 2048;   // workgroups of the seed launch
constexpr int FLATFIELD_FIT_BLOCK = 1024;
constexpr int FLATFIELD_FIT_WAVES = FLATFIELD_FIT_BLOCK / 64;

struct FlatFieldFitArgs {
  double axis[3];      // the unit normal (2-D: axis[2] = 0)
  double c[3], R;      // the box centre and its largest half-width
  double inv, min_det; // 2^-pbits
  int32_t n_groups;
};

// what the fit's two passes make of group k, from its record
struct FlatFieldGroup {
  double x[3], y[3], n, h;
  long long count;
  bool used;
};

template <int DIM>
__device__ __forceinline__ FlatFieldGroup flatfield_load(const long long* __restrict__ acc, int k,
                                                         const FlatFieldFitArgs& a) {
#pragma clang fp contract(off)
  int64_t rec[FOCUS_SLOTS];
#pragma unroll
  for (int p = 0; p < FOCUS_SLOTS; ++p) rec[p] = acc[FOCUS_SLOTS * (int64_t)k + p];
  FlatFieldGroup q;
  flatfield_solve<DIM>(rec, a.inv, a.min_det, a.axis, q.x, q.y, q.used);
  q.count = rec[0];
  q.n = (double)rec[0];
  q.h = q.used ? focus_dot<DIM>(a.axis, q.x) : 0.0;
  return q;
}

// One workgroup of FLATFIELD_FIT_BLOCK threads.  Thread t owns the groups t, t + 1024, ... (summed
// in that order, unused groups skipped), then the fixed-shape workgroup sum: the same bits on
// every run, and every thread holds the same sums.
template <int DIM>
__global__ __launch_bounds__(FLATFIELD_FIT_BLOCK) void k_flatfield_fit(
    const long long* __restrict__ acc, FlatFieldFitArgs a, double* __restrict__ table,
    double* __restrict__ fit_out, double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FLATFIELD_FIT_WAVES];
  __shared__ long long wcnt[FLATFIELD_FIT_WAVES];
  const int t = threadIdx.x;
  const int G = a.n_groups;

  // first pass: the plane's height
  double W = 0.0, S = 0.0;
  long long used = 0, terms = 0;
  for (int k = t; k < G; k += FLATFIELD_FIT_BLOCK) {
    const FlatFieldGroup q = flatfield_load<DIM>(acc, k, a);
    if (!q.used) continue;
    W += q.n;
    S += q.n * q.h;
    used += 1;
    terms += q.count;
  }
  W = error_block_sum<FLATFIELD_FIT_WAVES>(W, wsum);
  S = error_block_sum<FLATFIELD_FIT_WAVES>(S, wsum);
  used = error_block_sum<FLATFIELD_FIT_WAVES>(used, wcnt);
  terms = error_block_sum<FLATFIELD_FIT_WAVES>(terms, wcnt);
  const double hbar = S / W;
  const bool valid = used >= 2;

  // second pass: the table and the inside error
  const double nan = __builtin_nan("");
  double inside = 0.0;
  for (int k = t; k < G; k += FLATFIELD_FIT_BLOCK) {
    const FlatFieldGroup q = flatfield_load<DIM>(acc, k, a);
    double mu[3] = {0.0, 0.0, 0.0};
    double e = 0.0;
    if (q.used && valid) {
      e = flatfield_group<DIM>(q.h, hbar, a.R, q.y, mu);
      inside += q.n * e;
    }
    double* row = table + FLATFIELD_ROW * (int64_t)k;
    row[0] = q.used ? q.x[0] : nan;
    row[1] = q.used ? q.x[1] : nan;
    row[2] = q.used ? q.x[2] : nan;
    row[3] = q.used ? 1.0 : 0.0;
    row[4] = mu[0];
    row[5] = mu[1];
    row[6] = mu[2];
    row[7] = e;
  }
  inside = error_block_sum<FLATFIELD_FIT_WAVES>(inside, wsum);
  if (t == 0) {
    const double number = (double)terms;
    error_out[0] = inside;
    error_out[1] = number;
    error_out[2] = terms > 0 ? inside / number : nan;
    fit_out[0] = hbar;
    fit_out[1] = focus_dot<DIM>(a.axis, a.c) + a.R * hbar;
    fit_out[2] = W;
    fit_out[3] = (double)used;
    fit_out[4] = valid ? 1.0 : 0.0;
    fit_out[5] = fit_out[6] = fit_out[7] = 0.0;
  }
}

// The gradient rows of every column: flatfield_ray against the row of the ray's own group for a
// counting ray of a used group under a valid plane, zeros for the rest.
template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_flatfield_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, FocusArgs g,
    const double2* __restrict__ table, const double* __restrict__ fit_out,
    double* __restrict__ grad, int64_t grad_stride) {
#pragma clang fp contract(off)
  const bool valid = fit_out[4] != 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    const int label = focus_classify<T, DIM>(rows, stride, mask, group, perm, i, g, link);
    double gs[DIM], ge[DIM];
#pragma unroll
    for (int b = 0; b < DIM; ++b) gs[b] = ge[b] = 0.0;
    if (label >= 0 && valid) {
      // (the row is one 64-byte line: four 16-byte loads issued together)
      const double2* row = table + (FLATFIELD_ROW / 2) * (int64_t)label;
      const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
      if (r1.y != 0.0) {
        const double x[3] = {r0.x, r0.y, r1.x};
        const double mu[3] = {r2.x, r2.y, r3.x};
        double m[DIM];
        focus_normalise<DIM>(link.e, g.box, m);
        flatfield_ray<DIM>(link.d, m, x, mu, g.box.R, link.L, gs, ge);
      }
    }
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      grad[(int64_t)b * grad_stride + i] = gs[b];
      grad[(int64_t)(DIM + b) * grad_stride + i] = ge[b];
    }
  }
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

// (the launches keep no partials: the workspace is one reserved line)
size_t tfrt_flatfield_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > FOCUS_MAX_GROUPS) return 0;
  return align_up(64);
}

int tfrt_flatfield_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                         int32_t dimension, const int32_t* mask, const int32_t* group,
                         int64_t n_source, const int32_t* perm, int32_t n_groups, double x0,
                         double x1, double y0, double y1, double z0, double z1, int32_t pbits,
                         double min_det, double ax, double ay, double az, double* grad,
                         int64_t grad_stride, double* error_out, int64_t* acc, double* table,
                         double* fit_out, int32_t variant, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const double domain[6] = {x0, x1, y0, y1, z0, z1};
  FocusArgs g;
  if (focus_args(rows, stride, n, state_dtype, dimension, group, n_source, n_groups, domain, pbits,
                 min_det, grad, grad_stride, error_out, acc, table, variant, workspace, g) != 0)
    return TFRT_E_BADARG;
  if (!fit_out || (reinterpret_cast<uintptr_t>(table) & 63u) != 0) return TFRT_E_BADARG;
  // the axis: finite, of length 1 within 8 ulp of its square (az is not looked at in 2-D)
  FlatFieldFitArgs fa;
  fa.axis[0] = ax, fa.axis[1] = ay, fa.axis[2] = dimension == 3 ? az : 0.0;
  double sq = 0.0;
  for (int b = 0; b < 3; ++b) {
    if (!isfinite(fa.axis[b])) return TFRT_E_BADARG;
    sq += fa.axis[b] * fa.axis[b];
  }
  if (!(fabs(sq - 1.0) <= 8.0 * 2.220446049250313e-16)) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_flatfield_error_workspace_bytes(n, n_groups))
    return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= FOCUS_LDS_GROUPS);
  for (int b = 0; b < 3; ++b) fa.c[b] = g.box.c[b];
  fa.R = g.box.R, fa.inv = ldexp(1.0, -pbits), fa.min_det = min_det, fa.n_groups = n_groups;

  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  const long long* accs = reinterpret_cast<const long long*>(acc);
  const double2* table2 = reinterpret_cast<const double2*>(table);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int sgrid = error_grid(n, BLOCK, FLATFIELD_SEED_MAX_GRID);

  auto launch = [&](auto tag, auto d) {
    using T = typename decltype(tag)::type;
    constexpr int DIM = decltype(d)::value;
    const T* r = static_cast<const T*>(rows);
    focus_fill_records<T, DIM>(r, stride, n, mask, group, perm, g, lds, accu, st);
    hipLaunchKernelGGL((k_flatfield_fit<DIM>), dim3(1), dim3(FLATFIELD_FIT_BLOCK), 0, st, accs, fa,
                       table, fit_out, error_out);
    if (sgrid > 0)
      hipLaunchKernelGGL((k_flatfield_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride, n,
                         mask, group, perm, g, table2, fit_out, grad, grad_stride);
  };
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    if (dimension == 3)
      launch(tag, dim_tag<3>{});
    else
      launch(tag, dim_tag<2>{});
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
