// SumError: a weighted sum of error terms on one fused step.
//
// Every term of a step reads the same finished rows of one in-place trace and leaves a gradient
// seed on those rows and an error triple; the reverse sweep is linear in its seed, so one trace,
// K evaluations, ONE combination and one sweep make the combined step.  Two pieces live here (the
// definitions, operation by operation, are in include/tfrt_hip.h; combine_math.h is the
// per-element arithmetic, tests/error_combine_reference.py restates both in numpy):
//
//   tfrt_goal_error_columns   GoalError on the fixed-shape columns of an in-place trace
//                             (tfrt_scene3d.in_place == 2): a mask in the place of a ray count, the
//                             goal row looked up through the trace's order inside the kernel.
//                             k_goal_columns (a fixed grid, grid-stride; one partial sum and one
//                             count per workgroup) and k_goal_columns_finish (one workgroup, the
//                             partials in index order).  No atomics: the same bits on every run.
//   tfrt_error_combine        one launch: the coefficients c_k from the weights and -- reduce ==
//                             mean -- the terms' own counts, read on the device; the seed block
//                             acc = c_0 g_0, acc += c_k g_k over the terms that name a row; the
//                             error E = sum c_k e_k.  A pure streaming kernel: (sum_k rows_k +
//                             n_rows) x 8 B per column, 16-byte accesses (two columns per lane)
//                             where pointers and strides allow it, a scalar path otherwise; no LDS.
#include "tfrt_common.h"
#include "combine_math.h"
#include "error_sums.h"
#include "goal_finish.h"

namespace tfrt {

constexpr int GOAL_COLUMNS_MAX_GRID = 512;          // workgroups (two per CU of a 256-CU chip)
constexpr int GOAL_COLUMNS_PER_BLOCK = 4 * BLOCK;
constexpr int COMBINE_MAX_GRID = 2048;              // eight workgroups per CU, grid-stride the rest
constexpr int COMBINE_UNITS_PER_BLOCK = 2 * BLOCK;  // a unit: two columns (16 B) or one (scalar)

struct GoalColumns {
  int64_t stride, n, n_source;
  const int32_t* mask;
  const int32_t* perm;
  const double* goal;
  int64_t goal_stride, goal_ray_stride;
  GoalFields gf;
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_goal_columns(const T* __restrict__ rows, GoalColumns g,
                                                        double* __restrict__ grad,
                                                        int64_t grad_stride,
                                                        double* __restrict__ partial,
                                                        long long* __restrict__ partial_count) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  double sum = 0.0;
  long long count = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < g.n;
       i += (int64_t)gridDim.x * BLOCK) {
    bool counts = g.mask == nullptr || g.mask[i] >= 0;
    int64_t s = i;
    if (counts && g.perm != nullptr) s = g.perm[i];
    counts = counts && goal_source_ok(s, g.n_source);
    for (int c = 0; c < g.gf.n; ++c) {
      const int64_t at = (int64_t)g.gf.row[c];
      double seed = 0.0;
      if (counts) {
        const double d = goal_residual(ldd(rows, at * g.stride + i),
                                       g.goal[(int64_t)c * g.goal_stride + s * g.goal_ray_stride]);
        sum += goal_term(d);
        seed = goal_seed(d);
      }
      grad[at * grad_stride + i] = seed;
    }
    count += counts ? 1 : 0;
  }
  const double s = error_block_sum<WAVES>(sum, wsum);
  const long long c = error_block_sum<WAVES>(count, wcnt);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    partial_count[blockIdx.x] = c;
  }
}

// One workgroup: thread t owns partials t, t + 256, ... (added in that order), then the
// fixed-shape workgroup sum.
__global__ __launch_bounds__(BLOCK) void k_goal_columns_finish(
    const double* __restrict__ partial, const long long* __restrict__ partial_count, int n_partial,
    int n_fields, double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  double sum = 0.0;
  long long count = 0;
  for (int b = threadIdx.x; b < n_partial; b += BLOCK) {
    sum += partial[b];
    count += partial_count[b];
  }
  sum = error_block_sum<WAVES>(sum, wsum);
  count = error_block_sum<WAVES>(count, wcnt);
  if (threadIdx.x == 0) {
    const double terms = (double)n_fields * (double)count;
    error_out[0] = sum;
    error_out[1] = terms;
    error_out[2] = terms > 0.0 ? sum / terms : __builtin_nan("");
  }
}

// The descriptors as the kernel takes them: strides in 32 bits (checked by the host), the error
// triples, which only the first instructions read, apart, the row masks by row.
// row_terms: byte r holds the terms that name row r, bit k for term k -- one word for all masks.
struct CombineTerms {
  const double* grad[COMBINE_MAX_TERMS];
  int32_t stride[COMBINE_MAX_TERMS];
  const double* error[COMBINE_MAX_TERMS];
  uint64_t row_terms;
  int32_t n;
};

// Columns i .. i + W - 1 of every row: W = 2 with one 16-byte access per term and row, W = 1 with
// an 8-byte one.  A loop over the rows, unrolled over the terms: every term's descriptor and
// coefficient stays in scalar registers (unrolling the rows too spilled them), and the branches
// on a term's row mask are uniform over the launch.
template <int W>
__device__ __forceinline__ void combine_columns(const CombineTerms& a,
                                                const double (&c)[COMBINE_MAX_TERMS], int n_rows,
                                                int64_t i, double* __restrict__ out,
                                                int64_t out_stride) {
#pragma clang fp contract(off)
#pragma unroll 1
  for (int r = 0; r < n_rows; ++r) {
    const uint32_t named = (uint32_t)(a.row_terms >> (8 * r)) & 0xffu;
    double acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0;
    bool have = false;
#pragma unroll
    for (int k = 0; k < COMBINE_MAX_TERMS; ++k) {
      if ((named >> k) & 1u) {
        const double* p = a.grad[k] + (int64_t)r * a.stride[k] + i;
        double g[W];
        if constexpr (W == 2) {
          const double2 g2 = *reinterpret_cast<const double2*>(p);
          g[0] = g2.x, g[1] = g2.y;
        } else {
          g[0] = *p;
        }
#pragma unroll
        for (int w = 0; w < W; ++w)
          acc[w] = have ? combine_next(acc[w], c[k], g[w]) : combine_first(c[k], g[w]);
        have = true;
      }
    }
    double* q = out + (int64_t)r * out_stride + i;
    if constexpr (W == 2)
      *reinterpret_cast<double2*>(q) = make_double2(acc[0], acc[1]);
    else
      *q = acc[0];
  }
}

// VEC: a lane takes two neighbouring columns (every pointer 16-byte aligned, every stride even);
// a last odd column is taken alone.  out == NULL: the errors alone.
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_error_combine(
    CombineTerms a, const double* __restrict__ weights, int reduce, int64_t n, int n_rows,
    double* __restrict__ out, int64_t out_stride, double* __restrict__ error_out,
    double* __restrict__ coeff_out) {
#pragma clang fp contract(off)
  // (wave-uniform: the weights and the terms' counts come through the scalar cache)
  double c[COMBINE_MAX_TERMS];
#pragma unroll
  for (int k = 0; k < COMBINE_MAX_TERMS; ++k)
    c[k] = k < a.n ? combine_coefficient(weights[k], a.error[k][1], reduce) : 0.0;

  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < COMBINE_MAX_TERMS; ++k) {
      if (k < a.n) {
        const double v = a.error[k][0];
        e = k == 0 ? combine_first(c[k], v) : combine_next(e, c[k], v);
        coeff_out[k] = c[k];
      }
    }
    error_out[0] = e;
    error_out[1] = 1.0;
    error_out[2] = e;
  }
  if (out == nullptr) return;

  // (the pairs in the loop, a last odd column behind it: one loop with both bodies spilled
  // scalar registers)
  const int64_t units = VEC ? n / 2 : n;
  const int64_t first = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  for (int64_t u = first; u < units; u += (int64_t)gridDim.x * BLOCK)
    combine_columns<VEC ? 2 : 1>(a, c, n_rows, VEC ? 2 * u : u, out, out_stride);
  if (VEC && (n & 1) && first == 0) combine_columns<1>(a, c, n_rows, n - 1, out, out_stride);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_goal_error_columns_workspace_bytes(int64_t n) {
  if (n < 0 || n > INT32_MAX) return 0;
  return align_up(GOAL_COLUMNS_MAX_GRID * sizeof(double)) +
         align_up(GOAL_COLUMNS_MAX_GRID * sizeof(long long));
}

int tfrt_goal_error_columns(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                            int32_t n_rows, const int32_t* mask, const int32_t* perm,
                            int64_t n_source, const int32_t* fields, int32_t n_fields,
                            const double* goal, int64_t goal_stride, int64_t goal_ray_stride,
                            double* grad, int64_t grad_stride, double* error_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (n < 0 || n > INT32_MAX || (n_rows != 4 && n_rows != 6) || n_source < 0 ||
      n_source > INT32_MAX || !fields || n_fields < 1 || n_fields > n_rows || goal_stride < 0 ||
      goal_ray_stride < 0 || !error_out || !workspace || !state_dtype_ok(state_dtype))
    return TFRT_E_BADARG;
  GoalColumns g;
  g.gf.n = n_fields;
  for (int c = 0; c < 6; ++c) {
    g.gf.row[c] = c < n_fields ? fields[c] : 0;
    if (g.gf.row[c] < 0 || g.gf.row[c] >= n_rows) return TFRT_E_BADARG;
    for (int b = 0; b < c && c < n_fields; ++b)
      if (g.gf.row[b] == g.gf.row[c]) return TFRT_E_BADARG;
  }
  if (n > 0 && (!rows || !grad || stride < n || grad_stride < n || (n_source > 0 && !goal)))
    return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_goal_error_columns_workspace_bytes(n)) return TFRT_E_WORKSPACE;

  double* partial = static_cast<double*>(workspace);
  long long* partial_count = reinterpret_cast<long long*>(
      static_cast<char*>(workspace) + align_up(GOAL_COLUMNS_MAX_GRID * sizeof(double)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, GOAL_COLUMNS_PER_BLOCK, GOAL_COLUMNS_MAX_GRID);
  if (grid > 0) {
    g.stride = stride, g.n = n, g.n_source = n_source;
    g.mask = mask, g.perm = perm, g.goal = goal;
    g.goal_stride = goal_stride, g.goal_ray_stride = goal_ray_stride;
    const int rc = dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((k_goal_columns<T>), dim3(grid), dim3(BLOCK), 0, st,
                         static_cast<const T*>(rows), g, grad, grad_stride, partial,
                         partial_count);
      return 0;
    });
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(k_goal_columns_finish, dim3(1), dim3(BLOCK), 0, st, partial, partial_count,
                     grid, n_fields, error_out);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_error_combine(const tfrt_combine_term* terms, int32_t n_terms, const double* weights,
                       int32_t reduce, int64_t n, int32_t n_rows, double* grad_out,
                       int64_t out_stride, double* error_out, double* coeff_out, void* stream) {
  if (!terms || n_terms < 1 || n_terms > COMBINE_MAX_TERMS || !weights || !error_out ||
      !coeff_out || (reduce != 0 && reduce != 1) || n < 0 || n > INT32_MAX ||
      (n_rows != 4 && n_rows != 6))
    return TFRT_E_BADARG;
  CombineTerms a = {};
  a.n = n_terms;
  int with = 0;
  for (int k = 0; k < n_terms; ++k) {
    if (!terms[k].error || (terms[k].row_mask >> n_rows) != 0u || terms[k].stride < 0 ||
        terms[k].stride > INT32_MAX)
      return TFRT_E_BADARG;
    a.grad[k] = terms[k].grad;
    a.stride[k] = (int32_t)terms[k].stride;
    a.error[k] = terms[k].error;
    for (int r = 0; r < n_rows; ++r)
      if ((terms[k].row_mask >> r) & 1u) a.row_terms |= (uint64_t)1 << (8 * r + k);
    with += terms[k].grad != nullptr ? 1 : 0;
  }
  // (the gradients of all terms or of none: none, or n == 0, combines the errors alone)
  if (with != 0 && with != n_terms) return TFRT_E_BADARG;
  const bool with_grad = with != 0 && n > 0;
  bool vec = true;
  if (with_grad) {
    if (!grad_out || out_stride < n) return TFRT_E_BADARG;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(grad_out);
    const uintptr_t o1 = o0 + (uintptr_t)(((int64_t)(n_rows - 1) * out_stride + n) * 8);
    vec = aligned16(grad_out) && out_stride % 2 == 0;
    for (int k = 0; k < n_terms; ++k) {
      if (terms[k].stride < n) return TFRT_E_BADARG;
      const uintptr_t g0 = reinterpret_cast<uintptr_t>(terms[k].grad);
      const uintptr_t g1 = g0 + (uintptr_t)(((int64_t)(n_rows - 1) * terms[k].stride + n) * 8);
      if (g0 < o1 && o0 < g1) return TFRT_E_BADARG;      // the output aliases a term's block
      vec = vec && aligned16(terms[k].grad) && terms[k].stride % 2 == 0;
    }
  }
  const int64_t units = !with_grad ? 0 : (vec ? n / 2 : n);
  int grid = error_grid(units, COMBINE_UNITS_PER_BLOCK, COMBINE_MAX_GRID);
  if (grid < 1) grid = 1;      // (the errors are combined by the launch's first thread)
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((k_error_combine<true>), dim3(grid), dim3(BLOCK), 0, st, a, weights,
                       (int)reduce, n, (int)n_rows, with_grad ? grad_out : nullptr, out_stride,
                       error_out, coeff_out);
  else
    hipLaunchKernelGGL((k_error_combine<false>), dim3(grid), dim3(BLOCK), 0, st, a, weights,
                       (int)reduce, n, (int)n_rows, with_grad ? grad_out : nullptr, out_stride,
                       error_out, coeff_out);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

}  // extern "C"
