// Parameter-update kernels of the optimiser step (tfrt/optimizer.py:223-282, 316).
//
// k_sgd_process : non-finite -> 0, scale, clip of one gradient tensor and, optionally, the
//                 Keras-SGD apply `param -= sgd_lr * processed` in the same launch: the host
//                 path of the reference is six eager ops per parameter per step.
// k_sgd_momentum_multi : the same with the Keras momentum / Nesterov rule and a velocity buffer.
// k_adam_multi  : the same with the Keras Adam rule, its m / v buffers and a device step state.
// k_csr_matvec  : y = A x for a CSR matrix: the accumulator / smoother products
//                 (optimizer.py:250-255, 277-282).  The matrices the mesh tools build
//                 (mesh_tools.py:221-421) have a handful of non-zeros per row, a dense (P,P)
//                 product reads P^2 doubles (213 MB for the 5167-vertex lens) to use ~P*k of them.
//
// All of it is HBM/latency bound (tens of KB per launch); one thread per element / one wave per
// row, coalesced loads, nothing else to tune.
#include "tfrt_common.h"
#include "goal_finish.h"

namespace tfrt {

// the reference runs these as separate multiply / subtract ops: keep them unfused
#pragma clang fp contract(off)

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_sgd_process(const T* __restrict__ grad,
                                                       T* __restrict__ processed,
                                                       T* __restrict__ param, int64_t n, T scale,
                                                       T clip, T sgd_lr,
                                                       const double* __restrict__ hyper) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (hyper != nullptr) {  // step-dependent values live on the device (replayed launch graphs)
    scale = static_cast<T>(hyper[0]);
    clip = static_cast<T>(hyper[1]);
    sgd_lr = static_cast<T>(hyper[2]);
  }
  T g = grad[i];
  // optimizer.py:226-229 (tf.where(is_finite(g), g, 0)), :233 scale, :236-247 clip_by_value
  g = isfinite(g) ? g : T(0);
  g = g * scale;
  g = g < -clip ? -clip : (g > clip ? clip : g);
  if (processed != nullptr) processed[i] = g;
  if (param != nullptr) param[i] = param[i] - sgd_lr * g;
}

// The same for up to SGD_BATCH tensors in one launch (an optimiser with several parameter
// tensors -- the two surfaces of a lens -- otherwise pays one ~4 us launch each per step).
constexpr int SGD_BATCH = 8;
struct SgdBatch {
  const double* grad[SGD_BATCH];
  double* processed[SGD_BATCH];
  double* param[SGD_BATCH];
  int64_t n[SGD_BATCH];
  int32_t first_block[SGD_BATCH + 1];
  int32_t count;
};

__global__ __launch_bounds__(BLOCK) void k_sgd_process_multi(SgdBatch b,
                                                             const double* __restrict__ hyper,
                                                             tfrt_goal_pending goal) {
  // (one workgroup more than the tensors need, when the step's error sum is still to be finished)
  if ((int)blockIdx.x == b.first_block[SGD_BATCH]) {
    goal_finish_block(goal);
    return;
  }
  int k = 0;
  while (k + 1 < b.count && (int)blockIdx.x >= b.first_block[k + 1]) ++k;  // block-uniform
  const int64_t i = (int64_t)((int)blockIdx.x - b.first_block[k]) * BLOCK + threadIdx.x;
  if (i >= b.n[k]) return;
  const double scale = hyper[3 * k], clip = hyper[3 * k + 1], sgd_lr = hyper[3 * k + 2];
  double g = b.grad[k][i];
  g = isfinite(g) ? g : 0.0;
  g = g * scale;
  g = g < -clip ? -clip : (g > clip ? clip : g);
  if (b.processed[k] != nullptr) b.processed[k][i] = g;
  if (b.param[k] != nullptr) b.param[k][i] = b.param[k][i] - sgd_lr * g;
}

// The same with the Keras SGD momentum rule (optimizer.py:128-132 with momentum assigned, the
// generic path's SGD_Optimizer.apply_gradients): a persistent velocity per parameter element and
// two more scalars per tensor, {scale, clip, sgd_lr, momentum, nesterov} (5 float64).
//   v  = m*v - lr*g;   p += nesterov ? m*v - lr*g : v
// and, while m == 0, plain `p -= lr*g` with v left unwritten.  m is read on the device, so a
// captured launch graph replays across momentum phases.
struct SgdMomentumBatch {
  const double* grad[SGD_BATCH];
  double* processed[SGD_BATCH];
  double* param[SGD_BATCH];
  double* velocity[SGD_BATCH];
  int64_t n[SGD_BATCH];
  int32_t first_block[SGD_BATCH + 1];
  int32_t count;
};

__global__ __launch_bounds__(BLOCK) void k_sgd_momentum_multi(SgdMomentumBatch b,
                                                              const double* __restrict__ hyper,
                                                              tfrt_goal_pending goal) {
  if ((int)blockIdx.x == b.first_block[SGD_BATCH]) {
    goal_finish_block(goal);
    return;
  }
  int k = 0;
  while (k + 1 < b.count && (int)blockIdx.x >= b.first_block[k + 1]) ++k;  // block-uniform
  const int64_t i = (int64_t)((int)blockIdx.x - b.first_block[k]) * BLOCK + threadIdx.x;
  if (i >= b.n[k]) return;
  const double* h = hyper + 5 * k;
  const double scale = h[0], clip = h[1], sgd_lr = h[2], m = h[3];
  const bool nesterov = h[4] != 0.0;
  double g = b.grad[k][i];
  g = isfinite(g) ? g : 0.0;
  g = g * scale;
  g = g < -clip ? -clip : (g > clip ? clip : g);
  if (b.processed[k] != nullptr) b.processed[k][i] = g;
  double* p = b.param[k];
  if (m == 0.0) {  // optimizer.py: momentum off for this phase -- v keeps its value
    p[i] = p[i] - sgd_lr * g;
    return;
  }
  const double v = m * b.velocity[k][i] - sgd_lr * g;
  b.velocity[k][i] = v;
  p[i] = nesterov ? p[i] + (m * v - sgd_lr * g) : p[i] + v;
}

// The Keras Adam rule (non-amsgrad) after the same processing: persistent m and v per parameter
// element, {scale, clip, adam_learning_rate, beta1, beta2, epsilon} per tensor (6 float64) and the
// running state {t, p1, p2} per tensor (p1 = beta1^t, p2 = beta2^t as running products: IEEE
// exact, unlike the device pow).  With the state of THIS step, t+1, p1*beta1, p2*beta2:
//   lr_t = lr * sqrt(1 - p2) / (1 - p1)
//   m = beta1*m + (1 - beta1)*g;   v = beta2*v + (1 - beta2)*(g*g);   p -= lr_t*m / (sqrt(v) + eps)
// every operation rounded on its own.
//
// The state lives on the device (a replayed graph must count its steps) and this launch both
// reads and advances it.  In a workgroup only thread 0 reads its tensor's state, before any
// element is touched, and hands lr_t to the others through LDS; when the workgroup's work is
// issued the same thread takes a ticket (an acquire-release add, device scope).  Whoever draws the
// last ticket knows that every other workgroup's read is complete, writes {t+1, p1*beta1,
// p2*beta2} of every tensor and puts the ticket back to 0 for the next launch.  Nothing depends on
// the order in which workgroups run, and no workgroup ever sees the advanced value.
struct AdamBatch {
  const double* grad[SGD_BATCH];
  double* processed[SGD_BATCH];
  double* param[SGD_BATCH];
  double* m[SGD_BATCH];
  double* v[SGD_BATCH];
  int64_t n[SGD_BATCH];
  int32_t first_block[SGD_BATCH + 1];
  int32_t count;
  int32_t finish;  // the workgroup after the tensors' finishes `goal` (else it only takes a ticket)
};

__global__ __launch_bounds__(BLOCK) void k_adam_multi(AdamBatch b,
                                                      const double* __restrict__ hyper,
                                                      double* state, unsigned int* ticket,
                                                      tfrt_goal_pending goal) {
#pragma clang fp contract(off)
  __shared__ double lr_shared;
  if ((int)blockIdx.x >= b.first_block[SGD_BATCH]) {
    if (b.finish) goal_finish_block(goal);
  } else {
    int k = 0;
    while (k + 1 < b.count && (int)blockIdx.x >= b.first_block[k + 1]) ++k;  // block-uniform
    const double* h = hyper + 6 * k;
    if (threadIdx.x == 0) {
      const double p1 = state[3 * k + 1] * h[3], p2 = state[3 * k + 2] * h[4];
      lr_shared = h[2] * sqrt(1.0 - p2) / (1.0 - p1);
    }
    __syncthreads();
    const int64_t i = (int64_t)((int)blockIdx.x - b.first_block[k]) * BLOCK + threadIdx.x;
    if (i < b.n[k]) {
      const double scale = h[0], clip = h[1], beta1 = h[3], beta2 = h[4], eps = h[5];
      const double lr_t = lr_shared;
      double g = b.grad[k][i];
      g = isfinite(g) ? g : 0.0;
      g = g * scale;
      g = g < -clip ? -clip : (g > clip ? clip : g);
      if (b.processed[k] != nullptr) b.processed[k][i] = g;
      const double m = beta1 * b.m[k][i] + (1.0 - beta1) * g;
      const double v = beta2 * b.v[k][i] + (1.0 - beta2) * (g * g);
      b.m[k][i] = m;
      b.v[k][i] = v;
      double* p = b.param[k];
      p[i] = p[i] - lr_t * m / (sqrt(v) + eps);
    }
  }
  if (threadIdx.x != 0) return;
  // (release: this thread's read of the state is complete before the add is visible; acquire:
  // the writer's stores come after every other workgroup's add)
  const unsigned int t =
      __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (t != gridDim.x - 1) return;
  for (int k = 0; k < b.count; ++k) {
    double* s = state + 3 * k;
    const double t1 = s[0] + 1.0, p1 = s[1] * hyper[6 * k + 3], p2 = s[2] * hyper[6 * k + 4];
    s[0] = t1;
    s[1] = p1;
    s[2] = p2;
  }
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one wave per row; lanes stride over the row's non-zeros, butterfly-sum at the end
__global__ __launch_bounds__(BLOCK) void k_csr_matvec(const int64_t* __restrict__ crow,
                                                      const int64_t* __restrict__ col,
                                                      const double* __restrict__ val,
                                                      const double* __restrict__ x,
                                                      double* __restrict__ y, int64_t n_rows) {
  const int64_t row = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= n_rows) return;  // whole wave leaves together: row is wave-uniform
  const int64_t lo = crow[row], hi = crow[row + 1];
  double acc = 0.0;
  for (int64_t k = lo + lane_id(); k < hi; k += 64) acc += val[k] * x[col[k]];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane_id() == 0) y[row] = acc;
}

}  // namespace tfrt

using namespace tfrt;

extern "C" {

static int sgd_process_launch(const void* grad, void* processed, void* param, int64_t n,
                              int32_t dtype, double scale, double clip, double sgd_learning_rate,
                              const double* hyper, void* stream) {
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(cdiv(n, BLOCK));
  if (dtype == TFRT_F64)
    hipLaunchKernelGGL((k_sgd_process<double>), grid, dim3(BLOCK), 0, st,
                       static_cast<const double*>(grad), static_cast<double*>(processed),
                       static_cast<double*>(param), n, scale, clip, sgd_learning_rate, hyper);
  else
    hipLaunchKernelGGL((k_sgd_process<float>), grid, dim3(BLOCK), 0, st,
                       static_cast<const float*>(grad), static_cast<float*>(processed),
                       static_cast<float*>(param), n, (float)scale, (float)clip,
                       (float)sgd_learning_rate, hyper);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_sgd_process(const void* grad, void* processed, void* param, int64_t n, int32_t dtype,
                     double scale, double clip, double sgd_learning_rate, void* stream) {
  if (n < 0 || (n > 0 && !grad) || clip < 0.0 || (dtype != TFRT_F32 && dtype != TFRT_F64))
    return TFRT_E_BADARG;
  return sgd_process_launch(grad, processed, param, n, dtype, scale, clip, sgd_learning_rate,
                            nullptr, stream);
}

int tfrt_sgd_process_dev(const void* grad, void* processed, void* param, int64_t n, int32_t dtype,
                         const double* hyper, void* stream) {
  if (n < 0 || (n > 0 && !grad) || !hyper || (dtype != TFRT_F32 && dtype != TFRT_F64))
    return TFRT_E_BADARG;
  return sgd_process_launch(grad, processed, param, n, dtype, 0.0, 0.0, 0.0, hyper, stream);
}

static int sgd_multi_launch(int32_t n_tensors, const void* const* grad, void* const* processed,
                            void* const* param, const int64_t* n, const double* hyper,
                            const tfrt_goal_pending* pending, void* stream) {
  if (n_tensors < 0 || n_tensors > SGD_BATCH || (n_tensors > 0 && (!grad || !n || !hyper)))
    return TFRT_E_BADARG;
  if (pending != nullptr && (!pending->partial || (!pending->n_finished && !pending->partial_counts) ||
      !pending->error_out ||
                             pending->n_partial < 0))
    return TFRT_E_BADARG;
  SgdBatch b;
  int blocks = 0;
  for (int k = 0; k < SGD_BATCH; ++k) {
    const bool on = k < n_tensors;
    if (on && (n[k] < 0 || (n[k] > 0 && !grad[k]))) return TFRT_E_BADARG;
    b.grad[k] = on ? static_cast<const double*>(grad[k]) : nullptr;
    b.processed[k] = (on && processed) ? static_cast<double*>(processed[k]) : nullptr;
    b.param[k] = (on && param) ? static_cast<double*>(param[k]) : nullptr;
    b.n[k] = on ? n[k] : 0;
    b.first_block[k] = blocks;
    if (on) blocks += cdiv(n[k], BLOCK);
  }
  b.first_block[SGD_BATCH] = blocks;
  b.count = n_tensors;
  const int grid = blocks + (pending != nullptr ? 1 : 0);
  if (grid == 0) return 0;
  hipLaunchKernelGGL(k_sgd_process_multi, dim3(grid), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), b, hyper,
                     pending != nullptr ? *pending : tfrt_goal_pending{});
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_sgd_process_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, const int64_t* n, const double* hyper,
                           void* stream) {
  return sgd_multi_launch(n_tensors, grad, processed, param, n, hyper, nullptr, stream);
}

int tfrt_sgd_process_multi_finish(int32_t n_tensors, const void* const* grad,
                                  void* const* processed, void* const* param, const int64_t* n,
                                  const double* hyper, const tfrt_goal_pending* pending,
                                  void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return sgd_multi_launch(n_tensors, grad, processed, param, n, hyper, pending, stream);
}

static int sgd_momentum_launch(int32_t n_tensors, const void* const* grad,
                               void* const* processed, void* const* param, void* const* velocity,
                               const int64_t* n, const double* hyper,
                               const tfrt_goal_pending* pending, void* stream) {
  if (n_tensors < 0 || n_tensors > SGD_BATCH ||
      (n_tensors > 0 && (!grad || !param || !velocity || !n || !hyper)))
    return TFRT_E_BADARG;
  if (pending != nullptr &&
      (!pending->partial || (!pending->n_finished && !pending->partial_counts) ||
       !pending->error_out || pending->n_partial < 0))
    return TFRT_E_BADARG;
  SgdMomentumBatch b;
  int blocks = 0;
  for (int k = 0; k < SGD_BATCH; ++k) {
    const bool on = k < n_tensors;
    if (on && (n[k] < 0 || (n[k] > 0 && (!grad[k] || !param[k] || !velocity[k]))))
      return TFRT_E_BADARG;
    b.grad[k] = on ? static_cast<const double*>(grad[k]) : nullptr;
    b.processed[k] = (on && processed) ? static_cast<double*>(processed[k]) : nullptr;
    b.param[k] = on ? static_cast<double*>(param[k]) : nullptr;
    b.velocity[k] = on ? static_cast<double*>(velocity[k]) : nullptr;
    b.n[k] = on ? n[k] : 0;
    b.first_block[k] = blocks;
    if (on) blocks += cdiv(n[k], BLOCK);
  }
  b.first_block[SGD_BATCH] = blocks;
  b.count = n_tensors;
  const int grid = blocks + (pending != nullptr ? 1 : 0);
  if (grid == 0) return 0;
  hipLaunchKernelGGL(k_sgd_momentum_multi, dim3(grid), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), b, hyper,
                     pending != nullptr ? *pending : tfrt_goal_pending{});
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_sgd_momentum_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                            void* const* param, void* const* velocity, const int64_t* n,
                            const double* hyper, void* stream) {
  return sgd_momentum_launch(n_tensors, grad, processed, param, velocity, n, hyper, nullptr,
                             stream);
}

int tfrt_sgd_momentum_multi_finish(int32_t n_tensors, const void* const* grad,
                                   void* const* processed, void* const* param,
                                   void* const* velocity, const int64_t* n, const double* hyper,
                                   const tfrt_goal_pending* pending, void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return sgd_momentum_launch(n_tensors, grad, processed, param, velocity, n, hyper, pending,
                             stream);
}

static int adam_launch(int32_t n_tensors, const void* const* grad, void* const* processed,
                       void* const* param, void* const* m, void* const* v, const int64_t* n,
                       const double* hyper, double* state, uint32_t* ticket,
                       const tfrt_goal_pending* pending, void* stream) {
  if (n_tensors < 0 || n_tensors > SGD_BATCH ||
      (n_tensors > 0 && (!grad || !param || !m || !v || !n || !hyper || !state || !ticket)))
    return TFRT_E_BADARG;
  if (pending != nullptr &&
      (!pending->partial || (!pending->n_finished && !pending->partial_counts) ||
       !pending->error_out || pending->n_partial < 0))
    return TFRT_E_BADARG;
  AdamBatch b;
  int blocks = 0;
  for (int k = 0; k < SGD_BATCH; ++k) {
    const bool on = k < n_tensors;
    if (on && (n[k] < 0 || (n[k] > 0 && (!grad[k] || !param[k] || !m[k] || !v[k]))))
      return TFRT_E_BADARG;
    b.grad[k] = on ? static_cast<const double*>(grad[k]) : nullptr;
    b.processed[k] = (on && processed) ? static_cast<double*>(processed[k]) : nullptr;
    b.param[k] = on ? static_cast<double*>(param[k]) : nullptr;
    b.m[k] = on ? static_cast<double*>(m[k]) : nullptr;
    b.v[k] = on ? static_cast<double*>(v[k]) : nullptr;
    b.n[k] = on ? n[k] : 0;
    b.first_block[k] = blocks;
    if (on) blocks += cdiv(n[k], BLOCK);
  }
  b.first_block[SGD_BATCH] = blocks;
  b.count = n_tensors;
  b.finish = pending != nullptr ? 1 : 0;
  // (tensors without elements still count the step: one workgroup that only takes the ticket)
  const int grid = blocks + ((pending != nullptr || (blocks == 0 && n_tensors > 0)) ? 1 : 0);
  if (grid == 0) return 0;
  hipLaunchKernelGGL(k_adam_multi, dim3(grid), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), b,
                     hyper, state, ticket, pending != nullptr ? *pending : tfrt_goal_pending{});
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

int tfrt_adam_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                    void* const* param, void* const* m, void* const* v, const int64_t* n,
                    const double* hyper, double* state, uint32_t* ticket, void* stream) {
  return adam_launch(n_tensors, grad, processed, param, m, v, n, hyper, state, ticket, nullptr,
                     stream);
}

int tfrt_adam_multi_finish(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, void* const* m, void* const* v, const int64_t* n,
                           const double* hyper, double* state, uint32_t* ticket,
                           const tfrt_goal_pending* pending, void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return adam_launch(n_tensors, grad, processed, param, m, v, n, hyper, state, ticket, pending,
                     stream);
}

int tfrt_csr_matvec(const int64_t* crow_indices, const int64_t* col_indices, const double* values,
                    const double* x, double* y, int64_t n_rows, void* stream) {
  if (n_rows < 0 || (n_rows > 0 && (!crow_indices || !x || !y))) return TFRT_E_BADARG;
  if (n_rows == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_csr_matvec, dim3(cdiv(n_rows, WAVES)), dim3(BLOCK), 0, st, crow_indices,
                     col_indices, values, x, y, n_rows);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

}  // extern "C"
