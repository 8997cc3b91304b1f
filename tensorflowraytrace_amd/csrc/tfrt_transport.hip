// TransportError: sliced optimal transport of the finished rays to a target density.
//
// Along each of K projection directions the landing points are sorted; the ray of mid-rank r among
// n_valid belongs at the goal's quantile r / n_valid, which a table of Q + 1 knots per direction
// (built on the host: ops.transport_tables) gives by linear interpolation.  The error is the sum
// of the squared distances to those targets, its gradient 2 (p - t) along the direction: a global
// pull that needs no transport map and no overlap of pattern and goal.  The definition, operation
// by operation, is in include/tfrt_hip.h at tfrt_transport_error; tests/transport_error_reference.py
// restates it in numpy, transport_math.h is the per-ray arithmetic.
//
// Per direction, eleven launches:
//
//   k_transport_keys    one lane per column: the 26-bit key of its projection (invalid: 2^26 - 1)
//   sort_keys26         the stable radix sort of tfrt_order.hip, two 13-bit digits (8 launches)
//   k_transport_sorted  sk[r] = keys[perm[r]]
//   k_transport_rank    one lane per sorted position r: first = lower bound, last = upper bound of
//                       sk[r] in sk by two binary searches that gallop away from r (never a walk
//                       along a run of ties: every ray in one cell stays n log n, a key without a
//                       tie costs two loads), rank2[perm[r]] = first + last = 2 first + count.  In
//                       the first direction the lane of the last key that counts writes n_valid.
//
// then k_transport_seed over the columns (a fixed grid, grid-stride) -- every direction's target,
// residual and gradient in registers, both gradient rows written once, the squared residuals into
// one partial sum per workgroup -- and k_transport_finish, one workgroup that adds the partials in
// index order.  11 K + 2 launches; nothing is cleared (every buffer is written whole before it is
// read), nothing is read back, no atomics: the same bits on every run.
//
// Ties share the mid-rank, so a ray's rank does not depend on where its column stands: the fused
// step (coherent order) and the generic path (finished order) give every ray the same bits, and
// nothing depends on the sort being stable.
#include "tfrt_common.h"
#include "error_sums.h"
#include "order_sort.h"
#include "transport_math.h"

namespace tfrt {

constexpr int TRANSPORT_MAX_GRID = 512;     // workgroups of the seed (two per CU of a 256-CU chip)
constexpr int TRANSPORT_RAYS_PER_BLOCK = 4 * BLOCK;
constexpr int64_t TRANSPORT_MAX_RAYS = (int64_t)1 << 30;   // rank2 <= 2 n fits an int32

struct TransportColumns {
  int64_t stride, n;
  const int32_t* mask;
  double x0, ix, y0, iy;
  int32_t row_x, row_y;   // row_y < 0: one field
};

// Whether column i counts, and its normalised coordinates (eta = 0 with one field).
template <typename T>
__device__ __forceinline__ bool transport_column(const T* __restrict__ rows,
                                                 const TransportColumns& g, int64_t i, double& xi,
                                                 double& eta) {
  xi = eta = 0.0;
  if (g.mask != nullptr && g.mask[i] < 0) return false;
  const double x = ldd(rows, (int64_t)g.row_x * g.stride + i);
  const double y = g.row_y >= 0 ? ldd(rows, (int64_t)g.row_y * g.stride + i) : 0.0;
  if (!(isfinite(x) && isfinite(y))) return false;
  xi = transport_normalise(x, g.x0, g.ix);
  if (g.row_y >= 0) eta = transport_normalise(y, g.y0, g.iy);
  return true;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_transport_keys(const T* __restrict__ rows,
                                                          TransportColumns g,
                                                          const double* __restrict__ cs,
                                                          unsigned* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= g.n) return;
  double xi, eta;
  unsigned key = TRANSPORT_KEY_INVALID;
  if (transport_column(rows, g, i, xi, eta)) {
    const bool two = g.row_y >= 0;
    const TransportDirection d = two ? transport_direction(cs[0], cs[1])
                                     : transport_direction(1.0, 0.0);
    key = transport_key(d, two ? transport_project(d.c, d.s, xi, eta) : xi);
  }
  keys[i] = key;
}

__global__ __launch_bounds__(BLOCK) void k_transport_sorted(const unsigned* __restrict__ keys,
                                                            const int32_t* __restrict__ perm, int n,
                                                            unsigned* __restrict__ sk) {
  const int r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= n) return;
  const int32_t p = perm[r];
  // (perm is a permutation of [0, n): the sort wrote it; an index outside reads nothing)
  sk[r] = (p >= 0 && p < n) ? keys[p] : TRANSPORT_KEY_INVALID;
}

// The run of keys equal to q = sk[r] around position r of the sorted keys: its first index, and
// the index behind its last (the number of keys <= q).  Galloping away from r -- 1, 2, 4, ...
// positions -- and then bisecting: about 2 log2(run length) loads, one or two when the key has no
// tie, and never more than 2 log2(n) (every ray in one cell).  Neighbouring lanes hold
// neighbouring positions, so their loads fall into the same cache lines.
__device__ __forceinline__ int transport_first(const unsigned* __restrict__ sk, int r, unsigned q) {
  int hi = r, lo, step = 1;      // sk[hi] == q
  for (;;) {
    lo = hi - step;
    if (lo < 0) {
      lo = -1;
      break;
    }
    if (sk[lo] < q) break;
    hi = lo;
    step <<= 1;
  }
  while (hi - lo > 1) {          // sk[lo] < q (lo == -1: nothing below), sk[hi] == q
    const int mid = lo + ((hi - lo) >> 1);
    if (sk[mid] < q)
      lo = mid;
    else
      hi = mid;
  }
  return hi;
}
__device__ __forceinline__ int transport_last(const unsigned* __restrict__ sk, int r, int n,
                                              unsigned q) {
  int lo = r, hi, step = 1;      // sk[lo] == q
  for (;;) {
    hi = lo + step;              // (n <= 2^30: no overflow)
    if (hi >= n) {
      hi = n;
      break;
    }
    if (sk[hi] > q) break;
    lo = hi;
    step <<= 1;
  }
  while (hi - lo > 1) {          // sk[lo] == q, sk[hi] > q (hi == n: nothing above)
    const int mid = lo + ((hi - lo) >> 1);
    if (sk[mid] > q)
      hi = mid;
    else
      lo = mid;
  }
  return hi;
}

// One lane per SORTED position r: the column perm[r] gets rank2 = first + last = 2 first + count.
// n_valid given (the first direction): the lane of the last key that counts writes it -- the
// index behind that key's run --, lane 0 writes 0 when no key counts: exactly one store.
__global__ __launch_bounds__(BLOCK) void k_transport_rank(const unsigned* __restrict__ sk,
                                                          const int32_t* __restrict__ perm, int n,
                                                          int32_t* __restrict__ rank2,
                                                          int32_t* __restrict__ n_valid) {
  const int r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= n) return;
  const unsigned q = sk[r];
  const int32_t p = perm[r];
  // (perm is a permutation of [0, n): the sort wrote it; an index outside writes nothing)
  const bool ok = p >= 0 && p < n;
  if (q == TRANSPORT_KEY_INVALID) {
    if (r == 0 && n_valid != nullptr) *n_valid = 0;
    if (ok) rank2[p] = -1;
    return;
  }
  const int first = transport_first(sk, r, q);
  const int last = transport_last(sk, r, n, q);
  if (n_valid != nullptr && r == last - 1 && (last == n || sk[last] == TRANSPORT_KEY_INVALID))
    *n_valid = last;
  if (ok) rank2[p] = first + last;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_transport_seed(
    const T* __restrict__ rows, TransportColumns g, const double* __restrict__ cs,
    const double* __restrict__ tables, int n_knots, int n_directions,
    const int32_t* __restrict__ rank2, const int32_t* __restrict__ n_valid,
    double* __restrict__ grad, int64_t grad_stride, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  const bool two = g.row_y >= 0;
  const int32_t nv = *n_valid;
  double sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < g.n;
       i += (int64_t)gridDim.x * BLOCK) {
    double xi, eta, gx = 0.0, gy = 0.0, e = 0.0;
    if (transport_column(rows, g, i, xi, eta) && nv > 0) {
      for (int k = 0; k < n_directions; ++k) {
        const double c = two ? cs[2 * k] : 1.0, s = two ? cs[2 * k + 1] : 0.0;
        const int32_t r2 = rank2[(int64_t)k * g.n + i];
        // (a valid column has 0 < rank2 <= 2 n_valid; anything else would read outside the table)
        if (r2 < 0 || (int64_t)r2 > 2 * (int64_t)nv) continue;
        const double p = two ? transport_project(c, s, xi, eta) : xi;
        const double t =
            transport_target(tables + (int64_t)k * (n_knots + 1), n_knots, r2, nv);
        const double d = p - t;
        e += d * d;
        gx += ((2.0 * d) * c) * g.ix;
        gy += ((2.0 * d) * s) * g.iy;
      }
    }
    sum += e;
    grad[(int64_t)g.row_x * grad_stride + i] = gx;
    if (two) grad[(int64_t)g.row_y * grad_stride + i] = gy;
  }
  const double s = error_block_sum<WAVES>(sum, wsum);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One workgroup: thread t owns partials t, t + 256, ... (added in that order), then the
// fixed-shape workgroup sum.  n_valid null: no column at all.
__global__ __launch_bounds__(BLOCK) void k_transport_finish(const double* __restrict__ partial,
                                                            int n_partial,
                                                            const int32_t* __restrict__ n_valid,
                                                            int n_directions,
                                                            double* __restrict__ error_out) {
#pragma clang fp contract(off)
  __shared__ double wsum[WAVES];
  double sum = 0.0;
  for (int b = threadIdx.x; b < n_partial; b += BLOCK) sum += partial[b];
  sum = error_block_sum<WAVES>(sum, wsum);
  if (threadIdx.x == 0) {
    const double terms = (double)n_directions * (double)(n_valid != nullptr ? *n_valid : 0);
    error_out[0] = sum;
    error_out[1] = terms;
    error_out[2] = terms > 0.0 ? sum / terms : __builtin_nan("");
  }
}

struct TransportLayout {
  size_t keys, sk, perm, n_valid, partial, sort, total;
};

static TransportLayout transport_layout(int64_t n) {
  TransportLayout L;
  const size_t m = n > 0 ? (size_t)n : 1;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o = align_up(o + bytes);
    return at;
  };
  L.keys = take(m * sizeof(unsigned));
  L.sk = take(m * sizeof(unsigned));
  L.perm = take(m * sizeof(int32_t));
  L.n_valid = take(sizeof(int32_t));
  L.partial = take(TRANSPORT_MAX_GRID * sizeof(double));
  L.sort = take(sort_keys26_workspace_bytes(n));
  L.total = o;
  return L;
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

size_t tfrt_transport_error_workspace_bytes(int64_t n, int32_t n_directions) {
  if (n < 0 || n > TRANSPORT_MAX_RAYS || n_directions < 1 ||
      n_directions > TRANSPORT_MAX_DIRECTIONS)
    return 0;
  return transport_layout(n).total;
}

int tfrt_transport_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                         int32_t dimension, const int32_t* mask, int32_t row_x, int32_t row_y,
                         double x0, double ix, double y0, double iy, const double* angles_cs,
                         const double* tables, int32_t n_knots, int32_t n_directions,
                         double* grad, int64_t grad_stride, double* err, int32_t* rank2,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (n < 0 || n > TRANSPORT_MAX_RAYS || dimension < 2 || dimension > 3 || row_x < 0 ||
      row_x >= 2 * dimension || row_y < -1 || row_y >= 2 * dimension || row_x == row_y)
    return TFRT_E_BADARG;
  if (n_directions < 1 || n_directions > TRANSPORT_MAX_DIRECTIONS || n_knots < 2 ||
      n_knots > TRANSPORT_MAX_KNOTS || (row_y < 0 && n_directions != 1))
    return TFRT_E_BADARG;
  if (!isfinite(x0) || !isfinite(ix) || !(ix > 0.0) ||
      (row_y >= 0 && (!isfinite(y0) || !isfinite(iy) || !(iy > 0.0))))
    return TFRT_E_BADARG;
  if (!angles_cs || !tables || !err || !workspace || !state_dtype_ok(state_dtype))
    return TFRT_E_BADARG;
  if (n > 0 && (!rows || !grad || !rank2 || stride < n || grad_stride < n)) return TFRT_E_BADARG;
  if (workspace_bytes < tfrt_transport_error_workspace_bytes(n, n_directions))
    return TFRT_E_WORKSPACE;

  const TransportLayout L = transport_layout(n);
  char* ws = static_cast<char*>(workspace);
  unsigned* keys = reinterpret_cast<unsigned*>(ws + L.keys);
  unsigned* sk = reinterpret_cast<unsigned*>(ws + L.sk);
  int32_t* perm = reinterpret_cast<int32_t*>(ws + L.perm);
  int32_t* n_valid = reinterpret_cast<int32_t*>(ws + L.n_valid);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    hipLaunchKernelGGL(k_transport_finish, dim3(1), dim3(BLOCK), 0, st, partial, 0,
                       static_cast<const int32_t*>(nullptr), n_directions, err);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  }

  TransportColumns g;
  g.stride = stride, g.n = n, g.mask = mask;
  g.x0 = x0, g.ix = ix, g.y0 = row_y >= 0 ? y0 : 0.0, g.iy = row_y >= 0 ? iy : 0.0;
  g.row_x = row_x, g.row_y = row_y;
  const int nblk = cdiv(n, BLOCK);
  const int grid = error_grid(n, TRANSPORT_RAYS_PER_BLOCK, TRANSPORT_MAX_GRID);
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    const T* r = static_cast<const T*>(rows);
    for (int k = 0; k < n_directions; ++k) {
      hipLaunchKernelGGL((k_transport_keys<T>), dim3(nblk), dim3(BLOCK), 0, st, r, g,
                         angles_cs + 2 * k, keys);
      const int rc = sort_keys26(ws + L.sort, (int)n, keys, perm, st);
      if (rc != 0) return rc;
      hipLaunchKernelGGL(k_transport_sorted, dim3(nblk), dim3(BLOCK), 0, st, keys, perm, (int)n,
                         sk);
      hipLaunchKernelGGL(k_transport_rank, dim3(nblk), dim3(BLOCK), 0, st, sk, perm, (int)n,
                         rank2 + (int64_t)k * n, k == 0 ? n_valid : nullptr);
    }
    hipLaunchKernelGGL((k_transport_seed<T>), dim3(grid), dim3(BLOCK), 0, st, r, g, angles_cs,
                       tables, n_knots, n_directions, rank2, n_valid, grad, grad_stride, partial);
    hipLaunchKernelGGL(k_transport_finish, dim3(1), dim3(BLOCK), 0, st, partial, grid, n_valid,
                       n_directions, err);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

}  // extern "C"
