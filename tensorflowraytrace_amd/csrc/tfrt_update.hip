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
#include <array>

#include "tfrt_common.h"
#include "goal_finish.h"

namespace tfrt {

// the reference runs these as separate multiply / subtract ops: keep them unfused.  (Everything
// below that does arithmetic, the shared processing included, is compiled under this pragma.)
#pragma clang fp contract(off)

// optimizer.py:226-229 (tf.where(is_finite(g), g, 0)), :233 scale, :236-247 clip_by_value; the
// processed value is also written to processed[i] where the caller wants it
template <typename T>
__device__ __forceinline__ T process_gradient(T g, T scale, T clip, T* processed, int64_t i) {
  g = isfinite(g) ? g : T(0);
  g = g * scale;
  g = g < -clip ? -clip : (g > clip ? clip : g);
  if (processed != nullptr) processed[i] = g;
  return g;
}

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
  const T g = process_gradient(grad[i], scale, clip, processed, i);
  if (param != nullptr) param[i] = param[i] - sgd_lr * g;
}

// The same for up to SGD_BATCH tensors in one launch (an optimiser with several parameter
// tensors -- the two surfaces of a lens -- otherwise pays one ~4 us launch each per step), under
// one of three update rules.  The rules share the batch, the way a thread finds its tensor and
// element, the processing and the host launcher; a rule is a __global__ function of its own (the
// plain one pays for no other's LDS, barrier or ticket) with its per-element apply, STATES arrays
// of persistent per-element state and its row of `hyper`, {scale, clip, ...}, per tensor.
constexpr int SGD_BATCH = 8;
template <int STATES>
struct UpdateBatch {
  const double* grad[SGD_BATCH];
  double* processed[SGD_BATCH];
  double* param[SGD_BATCH];
  double* state[STATES][SGD_BATCH];  // none | velocity | m, v
  int64_t n[SGD_BATCH];
  int32_t first_block[SGD_BATCH + 1];
  int32_t count;
};
// (the plain rule's kernel-argument block carries no other rule's arrays)
static_assert(sizeof(UpdateBatch<0>) == 4 * 8 * SGD_BATCH + 4 * (SGD_BATCH + 2));

// The tensor this workgroup works on (block-uniform) and, in `i`, the thread's element of it,
// which may lie past the tensor's end; -1 in the workgroup behind the tensors' (one more than
// they need), which finishes the step's error sum here when one is pending.
template <int STATES>
__device__ __forceinline__ int locate(const UpdateBatch<STATES>& b, const tfrt_goal_pending& goal,
                                      int64_t& i) {
  if ((int)blockIdx.x >= b.first_block[SGD_BATCH]) {
    if (goal.partial != nullptr) goal_finish_block(goal);
    return -1;
  }
  int k = 0;
  while (k + 1 < b.count && (int)blockIdx.x >= b.first_block[k + 1]) ++k;  // block-uniform
  i = (int64_t)((int)blockIdx.x - b.first_block[k]) * BLOCK + threadIdx.x;
  return k;
}

// Plain SGD, {scale, clip, sgd_lr} per tensor: p -= lr*g (a null param: processing only).
__global__ __launch_bounds__(BLOCK) void k_sgd_process_multi(UpdateBatch<0> b,
                                                             const double* __restrict__ hyper,
                                                             tfrt_goal_pending goal) {
  int64_t i;
  const int k = locate(b, goal, i);
  if (k < 0 || i >= b.n[k]) return;
  const double* h = hyper + 3 * k;
  const double g = process_gradient(b.grad[k][i], h[0], h[1], b.processed[k], i);
  if (b.param[k] != nullptr) b.param[k][i] = b.param[k][i] - h[2] * g;
}

// The Keras SGD momentum rule (optimizer.py:128-132 with momentum assigned, the generic path's
// SGD_Optimizer.apply_gradients): a persistent velocity per parameter element and two more
// scalars per tensor, {scale, clip, sgd_lr, momentum, nesterov} (5 float64).
//   v  = m*v - lr*g;   p += nesterov ? m*v - lr*g : v
// and, while m == 0, plain `p -= lr*g` with v left unwritten.  m is read on the device, so a
// captured launch graph replays across momentum phases.
__global__ __launch_bounds__(BLOCK) void k_sgd_momentum_multi(UpdateBatch<1> b,
                                                              const double* __restrict__ hyper,
                                                              tfrt_goal_pending goal) {
  int64_t i;
  const int k = locate(b, goal, i);
  if (k < 0 || i >= b.n[k]) return;
  const double* h = hyper + 5 * k;
  const double sgd_lr = h[2], m = h[3];
  const bool nesterov = h[4] != 0.0;
  const double g = process_gradient(b.grad[k][i], h[0], h[1], b.processed[k], i);
  double* p = b.param[k];
  if (m == 0.0) {  // optimizer.py: momentum off for this phase -- v keeps its value
    p[i] = p[i] - sgd_lr * g;
    return;
  }
  double* velocity = b.state[0][k];
  const double v = m * velocity[i] - sgd_lr * g;
  velocity[i] = v;
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
// the order in which workgroups run, and no workgroup ever sees the advanced value.  (The
// workgroup behind the tensors' takes a ticket too, also when it has no error sum to finish: it
// is then the only one of a batch whose tensors have no elements, which still counts the step.)
__global__ __launch_bounds__(BLOCK) void k_adam_multi(UpdateBatch<2> b,
                                                      const double* __restrict__ hyper,
                                                      tfrt_goal_pending goal, double* state,
                                                      unsigned int* ticket) {
  __shared__ double lr_shared;
  int64_t i;
  const int k = locate(b, goal, i);
  if (k >= 0) {
    const double* h = hyper + 6 * k;
    if (threadIdx.x == 0) {
      const double p1 = state[3 * k + 1] * h[3], p2 = state[3 * k + 2] * h[4];
      lr_shared = h[2] * sqrt(1.0 - p2) / (1.0 - p1);
    }
    __syncthreads();
    if (i < b.n[k]) {
      const double beta1 = h[3], beta2 = h[4], eps = h[5];
      const double lr_t = lr_shared;
      const double g = process_gradient(b.grad[k][i], h[0], h[1], b.processed[k], i);
      const double m = beta1 * b.state[0][k][i] + (1.0 - beta1) * g;
      const double v = beta2 * b.state[1][k][i] + (1.0 - beta2) * (g * g);
      b.state[0][k][i] = m;
      b.state[1][k][i] = v;
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
  for (int j = 0; j < b.count; ++j) {
    double* s = state + 3 * j;
    const double t1 = s[0] + 1.0, p1 = s[1] * hyper[6 * j + 3], p2 = s[2] * hyper[6 * j + 4];
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

static bool pending_ok(const tfrt_goal_pending* p) {
  return p == nullptr || (p->partial && (p->n_finished || p->partial_counts) && p->error_out &&
                          p->n_partial >= 0);
}

// Validates, fills the batch and launches a rule's kernel over it, with one more workgroup when
// `pending` is to be finished.  A rule with state arrays needs its parameters (the plain one may
// only process); `extra` are a rule's further device arguments, Adam's step state and ticket.
template <int STATES, typename... Extra>
static int update_launch(void (*kernel)(UpdateBatch<STATES>, const double*, tfrt_goal_pending,
                                        Extra...),
                         int32_t n_tensors, const void* const* grad, void* const* processed,
                         void* const* param, std::array<void* const*, STATES> state,
                         const int64_t* n, const double* hyper, const tfrt_goal_pending* pending,
                         void* stream, Extra... extra) {
  bool have = grad && n && hyper && (STATES == 0 || param) && (... && (extra != nullptr));
  for (void* const* s : state) have = have && s;
  if (n_tensors < 0 || n_tensors > SGD_BATCH || (n_tensors > 0 && !have) || !pending_ok(pending))
    return TFRT_E_BADARG;
  UpdateBatch<STATES> b;
  int blocks = 0;
  for (int k = 0; k < SGD_BATCH; ++k) {
    const bool on = k < n_tensors;
    bool ok = !on || n[k] == 0 || (n[k] > 0 && grad[k] && (STATES == 0 || param[k]));
    b.grad[k] = on ? static_cast<const double*>(grad[k]) : nullptr;
    b.processed[k] = (on && processed) ? static_cast<double*>(processed[k]) : nullptr;
    b.param[k] = (on && param) ? static_cast<double*>(param[k]) : nullptr;
    for (int s = 0; s < STATES; ++s) {
      b.state[s][k] = on ? static_cast<double*>(state[s][k]) : nullptr;
      ok = ok && (!on || n[k] == 0 || b.state[s][k]);
    }
    if (!ok) return TFRT_E_BADARG;
    b.n[k] = on ? n[k] : 0;
    b.first_block[k] = blocks;
    if (on) blocks += cdiv(n[k], BLOCK);
  }
  b.first_block[SGD_BATCH] = blocks;
  b.count = n_tensors;
  // (Adam: tensors without elements still count the step, in one workgroup that only takes the
  // ticket)
  const bool ticket_only = sizeof...(Extra) > 0 && blocks == 0 && n_tensors > 0;
  const int grid = blocks + ((pending != nullptr || ticket_only) ? 1 : 0);
  if (grid == 0) return 0;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), b,
                     hyper, pending != nullptr ? *pending : tfrt_goal_pending{}, extra...);
  return hipGetLastError() == hipSuccess ? 0 : TFRT_E_LAUNCH;
}

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

int tfrt_sgd_process_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, const int64_t* n, const double* hyper,
                           void* stream) {
  return update_launch<0>(k_sgd_process_multi, n_tensors, grad, processed, param, {}, n, hyper,
                          nullptr, stream);
}

int tfrt_sgd_process_multi_finish(int32_t n_tensors, const void* const* grad,
                                  void* const* processed, void* const* param, const int64_t* n,
                                  const double* hyper, const tfrt_goal_pending* pending,
                                  void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return update_launch<0>(k_sgd_process_multi, n_tensors, grad, processed, param, {}, n, hyper,
                          pending, stream);
}

int tfrt_sgd_momentum_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                            void* const* param, void* const* velocity, const int64_t* n,
                            const double* hyper, void* stream) {
  return update_launch<1>(k_sgd_momentum_multi, n_tensors, grad, processed, param, {velocity}, n,
                          hyper, nullptr, stream);
}

int tfrt_sgd_momentum_multi_finish(int32_t n_tensors, const void* const* grad,
                                   void* const* processed, void* const* param,
                                   void* const* velocity, const int64_t* n, const double* hyper,
                                   const tfrt_goal_pending* pending, void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return update_launch<1>(k_sgd_momentum_multi, n_tensors, grad, processed, param, {velocity}, n,
                          hyper, pending, stream);
}

int tfrt_adam_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                    void* const* param, void* const* m, void* const* v, const int64_t* n,
                    const double* hyper, double* state, uint32_t* ticket, void* stream) {
  return update_launch<2>(k_adam_multi, n_tensors, grad, processed, param, {m, v}, n, hyper,
                          nullptr, stream, state, ticket);
}

int tfrt_adam_multi_finish(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, void* const* m, void* const* v, const int64_t* n,
                           const double* hyper, double* state, uint32_t* ticket,
                           const tfrt_goal_pending* pending, void* stream) {
  if (!pending) return TFRT_E_BADARG;
  return update_launch<2>(k_adam_multi, n_tensors, grad, processed, param, {m, v}, n, hyper,
                          pending, stream, state, ticket);
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
