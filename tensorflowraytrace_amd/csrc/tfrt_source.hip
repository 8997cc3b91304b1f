// Source rays made on the device, in place.
//
// The reference's optimisation scripts re-draw their rays every step: dev/hexalens.py:36-48 builds
// its AperatureSource from two RandomUniformCircle distributions (tfrt/distributions.py:1586-1598:
// tf.random.uniform in _update), lifted and moved by BasePointTransformation (:2014-2120), and
// SGD_Optimizer.single_step calls optical_system.update() first (tfrt/optimizer.py:217).  With
// stock tensor ops that is ~20 small kernels and a new set of tensors per step -- which also ends
// every per-source cache and the launch graph of the step.  Here a source is a small PROGRAM:
//
//   points program   how sample i of a distribution is made: a table row (static distributions),
//                    or two uniform numbers of a counter-based generator (Philox4x32-10, counter =
//                    (sample, epoch), key = (seed, stream)) pushed through the distribution's
//                    formula (circle / square / spherical cap, uniform or Lambertian:
//                    distributions.py:1375-1393, 1586-1598, 1751-1775, 1814-1850; or the quantile
//                    curves of a 2-D density, density_map.h: ArbitraryBasePoints, :2635-2798) and the
//                    transformation (lift to 3-D, scale, quaternion, translation)
//   source program   AperatureSource / PointSource / AngularSource assembly of two of those
//                    (tfrt/sources.py:464-1095, undense: sample i of each input makes ray i)
//   pool program     PrecompiledSource (tfrt/sources.py:1099-1358): a stored set of rays as 48-byte
//                    records, ray i = a row drawn with replacement (one Philox number) plus a
//                    normal jitter of the end points (Box-Muller on three more draws); the row is
//                    also handed out (tfrt_source3d_pool_rows) for the fields that are not geometry
//   samples program  a 1-D distribution of a 2-D source (a random angle in a fan, uniform or
//                    Lambertian; a random point on a beam or between two points; a table): ONE
//                    uniform number per sample (distributions.py:350-377, 458-501)
//   2-D source       the 2-D branches of the same three sources over two samples programs, a
//                    centre and a scalar central angle (tfrt_source2d_program)
//   2-D pool         the pool program with two axes: 32-byte records, one row draw and two more
//                    for the normals, the rows handed out by tfrt_source2d_pool_rows
//
// Rays and points are functions of (program, epoch, i): they are written into the caller's
// persistent buffers by one launch, any subset of them can be made again later (the sorted copy of
// an ordered source, a field somebody asks for after the step), and nothing but the device-side
// epoch counters changes from step to step, so the step stays one launch graph.
#include "tfrt_common.h"
#include "source_programs.h"

namespace tfrt {

// DENSITY: a TFRT_PTS_DENSITY program (see eval_points)
template <bool DENSITY>
__global__ __launch_bounds__(BLOCK) void k_points(tfrt_points_program pg, const int32_t* index,
                                                  int64_t first, int64_t n,
                                                  double* __restrict__ points,
                                                  int32_t cols, double* __restrict__ aux0,
                                                  double* __restrict__ aux1) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t i = first + (index != nullptr ? index[j] : j);
  double p[3], aux[2];
  eval_points<double, DENSITY>(pg, i, p, aux);
  if (points != nullptr) {
    if (cols == 3) {
      points[3 * j] = p[0];
      points[3 * j + 1] = p[1];
      points[3 * j + 2] = p[2];
    } else {                 // the untransformed distribution's own plane
      points[2 * j] = p[1];
      points[2 * j + 1] = p[2];
    }
  }
  if (aux0 != nullptr) aux0[j] = aux[0];
  if (aux1 != nullptr) aux1[j] = aux[1];
}

template <typename T, bool POOL, bool DENSITY>
__global__ __launch_bounds__(BLOCK) void k_source3d(tfrt_source3d_program sp,
                                                    const int32_t* __restrict__ index,
                                                    int64_t first, int64_t n,
                                                    T* __restrict__ rays, int64_t stride,
                                                    double* __restrict__ fields,
                                                    int64_t fstride) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t i = first + (index != nullptr ? index[j] : j);
  double s[3], e[3];
  eval_ray<POOL, DENSITY>(sp, i, s, e);
  if (rays != nullptr) store_ray3(rays, stride, j, s, e);
  if (fields != nullptr) store_ray3(fields, fstride, j, s, e);
}

// TFRT_SRC_POOL: the row every ray is made from (eval_pool's own pool_row); SP: the 3-D or the 2-D
// program
template <typename SP>
__global__ __launch_bounds__(BLOCK) void k_pool_rows(SP sp, const int32_t* __restrict__ index,
                                                     int64_t first, int64_t n,
                                                     int32_t* __restrict__ rows) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t i = first + (index != nullptr ? index[j] : j);
  const uint64_t epoch = sp.pool_downsample ? (uint64_t)*sp.pool_epoch : 0;
  rows[j] = (int32_t)pool_row(sp, i, epoch);
}

// One lane per ray / sample, nothing shared: store-bound (4 state columns and / or 4 float64 columns
// per ray, every column written by consecutive lanes).  POOL: see eval_ray2.
template <typename T, bool POOL>
__global__ __launch_bounds__(BLOCK) void k_source2d(tfrt_source2d_program sp,
                                                    const int32_t* __restrict__ index,
                                                    int64_t first, int64_t n,
                                                    T* __restrict__ rays, int64_t stride,
                                                    double* __restrict__ fields,
                                                    int64_t fstride) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t i = first + (index != nullptr ? index[j] : j);
  double s[2], e[2];
  eval_ray2<POOL>(sp, i, s, e);
  if (rays != nullptr) {           // the float64 result rounded once
    rays[j] = static_cast<T>(s[0]);
    rays[stride + j] = static_cast<T>(s[1]);
    rays[2 * stride + j] = static_cast<T>(e[0]);
    rays[3 * stride + j] = static_cast<T>(e[1]);
  }
  if (fields != nullptr) {
    fields[j] = s[0];
    fields[fstride + j] = s[1];
    fields[2 * fstride + j] = e[0];
    fields[3 * fstride + j] = e[1];
  }
}

__global__ __launch_bounds__(BLOCK) void k_samples(tfrt_samples_program pg,
                                                   const int32_t* __restrict__ index,
                                                   int64_t first, int64_t n,
                                                   double* __restrict__ values, int32_t cols,
                                                   double* __restrict__ ranks) {
  const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (j >= n) return;
  const int64_t i = first + (index != nullptr ? index[j] : j);
  double v[2], rank;
  eval_sample(pg, i, v, &rank);
  if (values != nullptr) {
    if (cols == 2) {               // (n, 2) rows, as the distributions' `points`
      values[2 * j] = v[0];
      values[2 * j + 1] = v[1];
    } else {
      values[j] = v[0];
    }
  }
  if (ranks != nullptr) ranks[j] = rank;
}

__global__ void k_epoch_advance(int64_t* p0, int64_t* p1, int64_t* p2, int64_t* p3, int64_t* p4,
                                int64_t* p5, int64_t* p6, int64_t* p7, int n) {
  int64_t* p[8] = {p0, p1, p2, p3, p4, p5, p6, p7};
  const int t = threadIdx.x;
  if (t < n && p[t] != nullptr) p[t][0] += 1;
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

int tfrt_epoch_advance(int64_t* const* epochs, int32_t n, void* stream) {
  if (n < 0 || n > 8 || (n > 0 && !epochs)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  int64_t* p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < n; ++i) p[i] = epochs[i];
  for (int i = 0; i < n; ++i)           // (the same counter twice would race)
    for (int j = 0; j < i; ++j)
      if (p[i] != nullptr && p[i] == p[j]) return TFRT_E_BADARG;
  hipLaunchKernelGGL(k_epoch_advance, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), p[0],
                     p[1], p[2], p[3], p[4], p[5], p[6], p[7], n);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_points_generate(const tfrt_points_program* program, const int32_t* index,
                         int64_t first, int64_t n, double* points, int32_t point_columns, double* aux0, double* aux1,
                         void* stream) {
  if (!points_program_ok(program) || n < 0 || (point_columns != 2 && point_columns != 3))
    return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->count)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  if (program->kind == TFRT_PTS_DENSITY)
    hipLaunchKernelGGL(k_points<true>, dim3(cdiv(n, BLOCK)), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(stream), *program, index, first, n, points,
                       point_columns, aux0, aux1);
  else
    hipLaunchKernelGGL(k_points<false>, dim3(cdiv(n, BLOCK)), dim3(BLOCK), 0,
                       static_cast<hipStream_t>(stream), *program, index, first, n, points,
                       point_columns, aux0, aux1);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_source3d_generate(const tfrt_source3d_program* program, const int32_t* index,
                           int64_t first, int64_t n, int32_t state_dtype, void* rays, int64_t stride, double* fields,
                           int64_t field_stride, void* stream) {
  if (n < 0 || !source_program_ok(program)) return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->n_rays)) return TFRT_E_BADARG;
  if ((rays != nullptr && stride < n) || (fields != nullptr && field_stride < n))
    return TFRT_E_BADARG;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(n, BLOCK));
  const bool pool = program->kind == TFRT_SRC_POOL, density = source_program_density(program);
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, st, *program, index, first, n,
                         static_cast<T*>(rays), stride, fields, field_stride);
    };
    if (pool) launch(k_source3d<T, true, false>);
    else if (density) launch(k_source3d<T, false, true>);
    else launch(k_source3d<T, false, false>);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

int tfrt_source3d_pool_rows(const tfrt_source3d_program* program, const int32_t* index,
                            int64_t first, int64_t n, int32_t* rows, void* stream) {
  if (n < 0 || !source_program_ok(program) || program->kind != TFRT_SRC_POOL) return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->n_rays)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  if (rows == nullptr) return TFRT_E_BADARG;
  hipLaunchKernelGGL(k_pool_rows<tfrt_source3d_program>, dim3(cdiv(n, BLOCK)), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), *program, index, first, n, rows);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_samples_generate(const tfrt_samples_program* program, const int32_t* index,
                          int64_t first, int64_t n, double* values, int32_t value_columns,
                          double* ranks, void* stream) {
  const int cols = samples_program_columns(program);
  if (cols == 0 || n < 0 || value_columns != cols) return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->count)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  if (program->count == 0) return TFRT_E_BADARG;
  hipLaunchKernelGGL(k_samples, dim3(cdiv(n, BLOCK)), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), *program, index, first, n, values, cols,
                     ranks);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_source2d_generate(const tfrt_source2d_program* program, const int32_t* index,
                           int64_t first, int64_t n, int32_t state_dtype, void* rays, int64_t stride,
                           double* fields, int64_t field_stride, void* stream) {
  if (n < 0 || !source2d_program_ok(program)) return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->n_rays)) return TFRT_E_BADARG;
  if ((rays != nullptr && stride < n) || (fields != nullptr && field_stride < n))
    return TFRT_E_BADARG;
  if (!state_dtype_ok(state_dtype)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  if (program->n_rays == 0) return TFRT_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(n, BLOCK));
  const bool pool = program->kind == TFRT_SRC_POOL;
  return dispatch_state(state_dtype, TFRT_E_BADARG, [&](auto tag) {
    using T = typename decltype(tag)::type;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, st, *program, index, first, n,
                         static_cast<T*>(rays), stride, fields, field_stride);
    };
    if (pool) launch(k_source2d<T, true>);
    else launch(k_source2d<T, false>);
    return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
  });
}

int tfrt_source2d_pool_rows(const tfrt_source2d_program* program, const int32_t* index,
                            int64_t first, int64_t n, int32_t* rows, void* stream) {
  if (n < 0 || !source2d_program_ok(program) || program->kind != TFRT_SRC_POOL) return TFRT_E_BADARG;
  if (first < 0 || (index == nullptr && first + n > program->n_rays)) return TFRT_E_BADARG;
  if (n == 0) return 0;
  if (rows == nullptr) return TFRT_E_BADARG;
  hipLaunchKernelGGL(k_pool_rows<tfrt_source2d_program>, dim3(cdiv(n, BLOCK)), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), *program, index, first, n, rows);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

}  // extern "C"
