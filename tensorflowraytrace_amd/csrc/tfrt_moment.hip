// MomentError: the COVARIANCE of every group of rays -- the size and the shape of its spot -- must
// be a given matrix (`covariance`), or must be round, whatever its size (`shape = round`).
//
// Every source ray carries a group label.  The finished rays of a group have an integer centre k_g
// on a grid of 2^mbits steps per domain width (the grid point nearest to their centroid) and the
// EXACT integer second moment M = sum (m - k)(m - k)^T about it, summed as three int64 limb sums
// per component; C = M / n in scene units is the covariance, D = C - target (or C - s I with the
// free size s = tr C / 2) its residual, and the error is the sum over the used groups of
// n |D|_F^2, plus SpotError's penalty for rays outside the domain.  The definition, operation by
// operation, is in include/tfrt_hip.h at tfrt_moment_error; the per-group arithmetic is in
// moment_math.h; tests/moment_error_reference.py restates it in numpy.
//
// Bit-reproducible by construction: both records are int64 sums (integer addition is associative:
// atomics in any order give the same bits), and the one floating-point sum over the groups has the
// fixed shape and order of k_centroid_table.  No float atomics, nothing waits on another workgroup.
//
// The gradient needs no derivative of the centre: a ray of group g gets 4 D (x - c), because the
// residuals x - c of a group sum to zero (up to the grid), and none of s, which minimises the error.
//
// Six launches:
//
//   k_moment_clear       zeroes both record tables (error_sums.h says why it is a launch).
//   k_spot_accumulate    spot_records.h: tfrt_spot_error's unweighted accumulate launch on this
//                        grid, the same two variants; its penalty and counting partials.
//   k_moment_centres     one lane per group: {kx, ky} of a used group, {-1, -1} of any other, into
//                        a (G, 2) int64 table.  (Forming them in the prologue of pass 2 instead
//                        measured the same step time: DESIGN.md section 6 has the figures.)
//   k_moment_accumulate  pass 2: the limb products of (m - k) of every ray inside a used group ->
//                        the group's second record, through a table in LDS up to MOMENT_LDS_GROUPS.
//   k_moment_table       ONE workgroup, one pass over the groups: the per-group rows {c, 4 D,
//                        used}, {C, D}, the inside error; then the accumulate launch's partials in
//                        index order, {sum, terms, mean} and {groups used, groups with rays}.
//   k_moment_seed        one 64-byte row of the ray's own group per ray inside, the gradient rows
//                        of EVERY column.
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "spot_records.h"
#include "moment_math.h"

namespace tfrt {

constexpr int MOMENT_LDS_GROUPS = 256;     // 9 planes of sums and 2 of centres, int64: 22 KiB
constexpr int MOMENT_LDS_PLANES = MOMENT_SLOTS + 2;
constexpr int MOMENT_MAX_MBITS = 40;
constexpr int MOMENT_SEED_MAX_GRID = 2048;   // workgroups of the seed launch
constexpr int MOMENT_ACC_SLOTS = SpotRecord<false>::SLOTS;

struct MomentTableArgs {
  MomentGrid grid;
  int32_t n_groups, k, mode, fields;
};

// k_error_clear over both record tables in one launch
__global__ __launch_bounds__(BLOCK) void k_moment_clear(unsigned long long* __restrict__ a,
                                                        int entries_a,
                                                        unsigned long long* __restrict__ b,
                                                        int entries_b) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e < entries_a)
    a[e] = 0ull;
  else if (e - entries_a < entries_b)
    b[e - entries_a] = 0ull;
}

// {kx, ky} of group k from its first record: the centre of a used group, {-1, -1} otherwise (a
// fixed-point coordinate is >= 0, so -1 is no centre).
__global__ __launch_bounds__(BLOCK) void k_moment_centres(const long long* __restrict__ acc,
                                                          int n_groups, bool two,
                                                          long long* __restrict__ centres) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n_groups) return;
  const long long* at = acc + MOMENT_ACC_SLOTS * (int64_t)k;
  const long long n = at[0];
  long long kx = -1, ky = -1;
  if (n >= 2) {
    kx = moment_centre(n, at[1]);
    ky = two ? moment_centre(n, at[2]) : 0;
  }
  centres[2 * (int64_t)k] = kx;
  centres[2 * (int64_t)k + 1] = ky;
}

// Pass 2.  LDS: the nine planes of G sums, then the planes of kx and of ky, copied from the table
// of k_moment_centres; else the sums go to `mom` by global atomics and the centres are read from
// that table ray by ray.
template <typename T, bool LDS, int DIM>
__global__ __launch_bounds__(BLOCK) void k_moment_accumulate(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotArgs<false> g, int h,
    const long long* __restrict__ centres, unsigned long long* __restrict__ mom) {
#pragma clang fp contract(off)
  extern __shared__ unsigned long long table[];
  const int G = g.n_groups;
  const bool two = g.row_y >= 0;
  long long* kxs = reinterpret_cast<long long*>(table) + MOMENT_SLOTS * G;
  long long* kys = kxs + G;
  if (LDS) {
    for (int e = threadIdx.x; e < MOMENT_SLOTS * G; e += BLOCK) table[e] = 0ull;
    for (int k = threadIdx.x; k < G; k += BLOCK)
      kxs[k] = centres[2 * (int64_t)k], kys[k] = centres[2 * (int64_t)k + 1];
    __syncthreads();
  }
  auto add = [&](int label, int p, long long v) {
    unsigned long long* to = LDS ? table + (p * G + label) : mom + MOMENT_SLOTS * (int64_t)label + p;
    atomicAdd(to, (unsigned long long)v);
  };
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq = 0.0, wr = 0.0;
    const SpotRay r =
        spot_classify<T, DIM, false>(rows, stride, mask, group, perm, i, g, link, wq, wr);
    if (r.kind != 1) continue;
    const long long kx = LDS ? kxs[r.label] : centres[2 * (int64_t)r.label];
    if (kx < 0) continue;                       // a group of one ray: not used
    const long long dx = (long long)spot_fixed(r.x, g.x0, g.qsx, g.qmax) - kx;
    const long long xl = moment_low(dx, h), xh = moment_high(dx, h);
    add(r.label, 0, xh * xh);
    add(r.label, 1, 2 * (xh * xl));
    add(r.label, 2, xl * xl);
    if (two) {
      const long long ky = LDS ? kys[r.label] : centres[2 * (int64_t)r.label + 1];
      const long long dy = (long long)spot_fixed(r.y, g.y0, g.qsy, g.qmax) - ky;
      const long long yl = moment_low(dy, h), yh = moment_high(dy, h);
      add(r.label, 3, xh * yh);
      add(r.label, 4, xh * yl + xl * yh);
      add(r.label, 5, xl * yl);
      add(r.label, 6, yh * yh);
      add(r.label, 7, 2 * (yh * yl));
      add(r.label, 8, yl * yl);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < MOMENT_SLOTS * G; e += BLOCK) {
      const unsigned long long v = table[e];
      const int plane = e / G, label = e - plane * G;
      if (v != 0ull) atomicAdd(mom + MOMENT_SLOTS * (int64_t)label + plane, v);
    }
  }
}

// One workgroup of FINISH_BLOCK threads.  Thread t owns the groups (and then the partials) t,
// t + 1024, ... (summed in that order), then the fixed-shape workgroup sum: the same bits on every
// run.
__global__ __launch_bounds__(FINISH_BLOCK) void k_moment_table(
    const long long* __restrict__ acc, const long long* __restrict__ mom,
    const double* __restrict__ target, MomentTableArgs a,
    const double* __restrict__ pen_partial, const long long* __restrict__ cnt_partial, int n_acc,
    double* __restrict__ row_out, double* __restrict__ cov_out, double* __restrict__ used_out,
    double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[FINISH_WAVES];
  __shared__ long long wcnt[FINISH_WAVES];
  __shared__ double tsum;
  __shared__ long long tcnt;
  const int t = threadIdx.x;
  const int G = a.n_groups;

  double inside = 0.0;
  long long used = 0, with_rays = 0;
  for (int k = t; k < G; k += FINISH_BLOCK) {
    int64_t rec[3], limbs[MOMENT_SLOTS];
    const long long* at = acc + MOMENT_ACC_SLOTS * (int64_t)k;
    rec[0] = at[0], rec[1] = at[1], rec[2] = at[2];
    const long long* mt = mom + MOMENT_SLOTS * (int64_t)k;
#pragma unroll
    for (int p = 0; p < MOMENT_SLOTS; ++p) limbs[p] = mt[p];
    const double* tg = target != nullptr ? target + (int64_t)a.k * k : nullptr;
    const MomentGroup q = moment_group(rec, limbs, a.grid, a.mode, tg);
    if (q.used) inside += q.e;
    used += q.used ? 1 : 0;
    with_rays += q.rays ? 1 : 0;
    double* ro = row_out + MOMENT_ROW * (int64_t)k;
    ro[0] = q.cx, ro[1] = q.cy;
    ro[2] = q.F[0], ro[3] = q.F[1], ro[4] = q.F[2];
    ro[5] = q.used ? 1.0 : 0.0;
    ro[6] = ro[7] = 0.0;
    double* co = cov_out + MOMENT_COV * (int64_t)k;
#pragma unroll
    for (int c = 0; c < 3; ++c) co[c] = q.C[c], co[3 + c] = q.D[c];
  }
  const double e_in = error_block_total<FINISH_WAVES>(inside, wsum, &tsum);
  used = error_block_total<FINISH_WAVES>(used, wcnt, &tcnt);
  with_rays = error_block_total<FINISH_WAVES>(with_rays, wcnt, &tcnt);

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
    const double e = e_in + pen;
    const double terms = (double)(counting * a.fields);
    error_out[0] = e;
    error_out[1] = terms;
    error_out[2] = counting > 0 ? e / terms : __builtin_nan("");
    used_out[0] = (double)used;
    used_out[1] = (double)with_rays;
  }
}

// The gradient rows of every column: F (x - c) of the ray's own group for a ray inside a used
// group (F = 4 D), the penalty's derivative for one outside (tfrt_spot_error's), zeros for the rest.
template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_moment_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotArgs<false> g,
    const double2* __restrict__ row, double* __restrict__ grad, int64_t grad_stride) {
#pragma clang fp contract(off)
  const bool two = g.row_y >= 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq = 0.0, wr = 0.0;
    const SpotRay r =
        spot_classify<T, DIM, false>(rows, stride, mask, group, perm, i, g, link, wq, wr);
    double gx = 0.0, gy = 0.0;
    if (r.kind == 2) {
      gx = g.oob * (2.0 * r.x) * r.dx;
      gy = g.oob * (2.0 * r.y) * r.dy;
    } else if (r.kind == 1) {
      const double2* at = row + (MOMENT_ROW / 2) * (int64_t)r.label;
      const double2 c = at[0], f0 = at[1], f1 = at[2];     // {cx, cy} {Fxx, Fxy} {Fyy, used}
      if (f1.y != 0.0) {
        const double ux = r.x - c.x;
        if (two) {
          const double uy = r.y - c.y;
          gx = f0.x * ux + f0.y * uy;
          gy = f0.y * ux + f1.x * uy;
        } else {
          gx = f0.x * ux;
        }
      }
    }
    if constexpr (DIM != 0) {
      chain_fields<DIM>(link, r.kind == 1 || r.kind == 2, g.row_x, g.row_y, gx, gy, grad,
                        grad_stride, i);
    } else {
      grad[(int64_t)g.row_x * grad_stride + i] = gx;
      if (two) grad[(int64_t)g.row_y * grad_stride + i] = gy;
    }
  }
}

inline size_t moment_partials_bytes() { return align_up(SPOT_MAX_GRID * sizeof(double)); }

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_moment_error_workspace_bytes(int64_t n, int32_t n_groups) {
  if (n < 0 || n > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS) return 0;
  return 2 * moment_partials_bytes() + align_up((size_t)n_groups * 2 * sizeof(long long));
}

int tfrt_moment_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                      int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                      const int32_t* group, int64_t n_source, const int32_t* perm,
                      int32_t n_groups, int32_t mode, const double* covariance, double x0,
                      double x1, double msx, double y0, double y1, double msy, int32_t mbits,
                      double oob_weight, double* grad, int64_t grad_stride, double* error_out,
                      double* used_out, double* group_rows, double* cov_out, int64_t* acc,
                      int64_t* mom, int32_t variant, void* workspace, size_t workspace_bytes,
                      void* stream) {
  if (dimension < 2 || dimension > 3 || field_x < 0 || field_x >= 3 * dimension || field_y < -1 ||
      field_y >= 3 * dimension)
    return TFRT_E_BADARG;
  const bool two = field_y >= 0;
  // exactly one mode: a target covariance, or "round" (which needs both axes)
  if (mode != MOMENT_TARGET && mode != MOMENT_ROUND) return TFRT_E_BADARG;
  if ((mode == MOMENT_TARGET) != (covariance != nullptr)) return TFRT_E_BADARG;
  if (mode == MOMENT_ROUND && !two) return TFRT_E_BADARG;
  if (n_source < 0 || n_source > INT32_MAX || n_groups < 1 || n_groups > SPOT_MAX_GROUPS ||
      mbits < 2 || mbits > MOMENT_MAX_MBITS || (mbits & 1) != 0 || !group || !used_out ||
      !group_rows || !cov_out || !mom ||
      (reinterpret_cast<uintptr_t>(group_rows) & 15u) != 0 ||
      !error_args_ok(rows, stride, n, state_dtype, field_x, field_y, x0, x1, msx, y0, y1, msy,
                     oob_weight, grad, grad_stride, error_out, acc, variant, workspace))
    return TFRT_E_BADARG;
  if (n >= ((int64_t)1 << (61 - mbits))) return TFRT_E_BADARG;   // n * 2^(mbits + 1) below 2^62
  if (variant == 1 && n_groups > MOMENT_LDS_GROUPS) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_moment_error_workspace_bytes(n, n_groups)) return TFRT_E_WORKSPACE;
  const bool lds = variant == 1 || (variant == 0 && n_groups <= MOMENT_LDS_GROUPS);

  SpotGrid sg;
  sg.x0 = x0, sg.x1 = x1, sg.qsx = msx, sg.oob = oob_weight;
  sg.y0 = two ? y0 : 0.0, sg.y1 = two ? y1 : 0.0, sg.qsy = two ? msy : 0.0;
  sg.qmax = ldexp(1.0, mbits);
  sg.n_source = n_source, sg.n_groups = n_groups, sg.row_x = field_x, sg.row_y = field_y;
  const SpotArgs<false> g{sg};
  MomentTableArgs ta;
  ta.grid.x0 = sg.x0, ta.grid.msx = sg.qsx, ta.grid.y0 = sg.y0, ta.grid.msy = sg.qsy;
  ta.grid.mbits = mbits, ta.grid.h = mbits / 2, ta.grid.two = two;
  ta.n_groups = n_groups, ta.k = two ? 3 : 1, ta.mode = mode, ta.fields = two ? 2 : 1;
  const int h = mbits / 2;

  char* ws = static_cast<char*>(workspace);
  double* pen_partial = reinterpret_cast<double*>(ws);
  long long* cnt_partial = reinterpret_cast<long long*>(ws + moment_partials_bytes());
  long long* centres = reinterpret_cast<long long*>(ws + 2 * moment_partials_bytes());
  unsigned long long* accu = reinterpret_cast<unsigned long long*>(acc);
  const long long* accs = reinterpret_cast<const long long*>(acc);
  unsigned long long* momu = reinterpret_cast<unsigned long long*>(mom);
  const long long* moms = reinterpret_cast<const long long*>(mom);
  const double2* rows2 = reinterpret_cast<const double2*>(group_rows);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int grid = error_grid(n, SPOT_RAYS_PER_BLOCK, SPOT_MAX_GRID);
  const int sgrid = error_grid(n, BLOCK, MOMENT_SEED_MAX_GRID);
  const int64_t entries = (int64_t)n_groups * (MOMENT_ACC_SLOTS + MOMENT_SLOTS);

  hipLaunchKernelGGL(k_moment_clear, dim3(cdiv(entries, BLOCK)), dim3(BLOCK), 0, st, accu,
                     MOMENT_ACC_SLOTS * n_groups, momu, MOMENT_SLOTS * n_groups);
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const T* r = static_cast<const T*>(rows);
    dispatch_fields(dimension, field_x, field_y, [&](auto d) {
      constexpr int DIM = decltype(d)::value;
      if (grid > 0) {
        // (pass 1's table in LDS wherever pass 2's is: MOMENT_LDS_GROUPS <= SPOT_LDS_GROUPS)
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
        hipLaunchKernelGGL(k_moment_centres, dim3(cdiv((int64_t)n_groups, BLOCK)), dim3(BLOCK), 0,
                           st, accs, n_groups, two, centres);
        if (lds)
          hipLaunchKernelGGL((k_moment_accumulate<T, true, DIM>), dim3(grid), dim3(BLOCK),
                             (size_t)n_groups * MOMENT_LDS_PLANES * sizeof(unsigned long long), st,
                             r, stride, n, mask, group, perm, g, h, centres, momu);
        else
          hipLaunchKernelGGL((k_moment_accumulate<T, false, DIM>), dim3(grid), dim3(BLOCK), 0, st,
                             r, stride, n, mask, group, perm, g, h, centres, momu);
      }
      hipLaunchKernelGGL(k_moment_table, dim3(1), dim3(FINISH_BLOCK), 0, st, accs, moms,
                         covariance, ta, pen_partial, cnt_partial, grid,
                         group_rows, cov_out, used_out, error_out);
      if (sgrid > 0)
        hipLaunchKernelGGL((k_moment_seed<T, DIM>), dim3(sgrid), dim3(BLOCK), 0, st, r, stride, n,
                           mask, group, perm, g, rows2, grad, grad_stride);
    });
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
