/*
 * tfrt_hip.h -- C ABI of libtfrt_hip.so, the MI355X (gfx950) implementation of the tfrt
 * hot path: batched ray x boundary intersection, nearest-hit reduction, classification /
 * stable compaction, Snell refraction / reflection, iterated over passes, plus the
 * hand-derived reverse sweep.
 *
 * The upstream reference (ecpoppenheimer/TensorFlowRayTrace) is pure Python on TensorFlow
 * eager ops: it has NO native/FFI boundary on this path.  Each entry point below therefore
 * cites the Python seam it replaces (file:line in the reference); INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add at that seam.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensors); nothing is
 *    allocated, freed or retained; no global state; re-entrant
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing
 *    synchronises, so a caller may capture a call into a hipGraph
 *  - ray sets are SoA: a "ray block" is 6 rows (3-D: xs,ys,zs,xe,ye,ze) or 4 rows
 *    (2-D: xs,ys,xe,ye) of `stride` elements each; `state_dtype` selects the element type
 *    of ray blocks (TFRT_F32 / TFRT_F64 / TFRT_F16).  Geometry, indices of refraction and gradients
 *    are always float64.
 *  - return value: 0 on success, negative TFRT_E_* otherwise (see tfrt_strerror)
 */
#ifndef TFRT_HIP_H
#define TFRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFRT_VERSION 107 /* 0.1.0 */

#define TFRT_F32 0
#define TFRT_F64 1
#define TFRT_F16 2 /* storage-only experiment (BASELINE config 5): half ray state, math stays f32/f64 */

/* boundary catagory, tfrt/engine.py:14-16 */
#define TFRT_OPTICAL 0
#define TFRT_STOP 1
#define TFRT_TARGET 2

/* ray classes produced by a pass (tfrt/engine.py:2027-2111) */
#define TFRT_CLS_ACTIVE 0
#define TFRT_CLS_FINISHED 1
#define TFRT_CLS_STOPPED 2
#define TFRT_CLS_DEAD 3

/* flags (OpticalEngine constructor kwargs, tfrt/engine.py:1216-1230) */
#define TFRT_COMPILE_ACTIVE 1u
#define TFRT_COMPILE_FINISHED 2u
#define TFRT_COMPILE_STOPPED 4u
#define TFRT_COMPILE_DEAD 8u

#define TFRT_E_BADARG (-1)
#define TFRT_E_WORKSPACE (-2)
#define TFRT_E_LAUNCH (-3)
#define TFRT_E_UNSUPPORTED (-4)

int tfrt_version(void);
const char* tfrt_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Triangle boundaries: vertices -> per-face data.
 * Replaces TriangleBoundaryBase.update_fields_from_vertices, tfrt/boundaries.py:890-923
 * (gather faces, cross, normalize) and, in reverse, the tape's scatter through that gather
 * with the per-corner stop_gradient mask (`vertex_update_map`, boundaries.py:900-913).
 *
 *   vertices    (V,3) f64 row-major
 *   faces       (F,3) i32 vertex indices
 *   face_verts  (F,9) f64 : xp,yp,zp,x1,y1,z1,x2,y2,z2 per face
 *   norm        (F,3) f64 : normalize((P1-P0) x (P2-P1))
 */
int tfrt_build_faces_forward(const double* vertices, int64_t n_vertices, const int32_t* faces,
                             int64_t n_faces, double* face_verts, double* norm, void* stream);

/* grad_norm and update_mask may be NULL.  update_mask (F,3) u8: 0 = stop_gradient for that
 * corner.  corner_start (V+1) / corner_list (3F) i32, both or neither: the face corners f*3+c
 * sorted by the vertex they reference (corner_list[corner_start[v] .. corner_start[v+1]) are
 * vertex v's).  With them the reverse is a gather -- one lane per vertex sums its corners in
 * list order: no atomics, grad_vertices (V,3) is OVERWRITTEN and the result is bit-identical
 * from run to run.  Without them (NULL) it scatters with float64 atomics and ACCUMULATES into
 * grad_vertices (caller zeroes). */
int tfrt_build_faces_backward(const double* grad_face_verts, const double* grad_norm,
                              const double* face_verts, const int32_t* faces,
                              const uint8_t* update_mask, int64_t n_faces, int64_t n_vertices,
                              const int32_t* corner_start, const int32_t* corner_list,
                              double* grad_vertices, void* stream);

/* Parametric surface: parameters -> per-face data in one launch.
 * Replaces ParametricTriangleBoundary._update, tfrt/boundaries.py:1065-1078
 * (`zero_points + parameters[:,None] * vectors`, boundaries.py:1080-1092) followed by
 * update_fields_from_vertices (boundaries.py:890-923); bit-identical with the two-step path
 * (product and sum stay separate roundings).
 *
 *   zero_points, vectors  (V,3) f64 row-major;  parameters (V,) f64
 * The reverse sums, per face corner that update_mask lets through, dot(grad of that corner,
 * vectors[vertex]) into grad_parameters (V,): as a gather when corner_start / corner_list are
 * given (see tfrt_build_faces_backward: overwritten, deterministic), else with atomics
 * (ACCUMULATED, caller zeroes). */
int tfrt_param_faces_forward(const double* zero_points, const double* vectors,
                             const double* parameters, int64_t n_vertices, const int32_t* faces,
                             int64_t n_faces, double* face_verts, double* norm, void* stream);
int tfrt_param_faces_backward(const double* grad_face_verts, const double* grad_norm,
                              const double* face_verts, const int32_t* faces,
                              const uint8_t* update_mask, const double* vectors, int64_t n_faces,
                              int64_t n_vertices, const int32_t* corner_start,
                              const int32_t* corner_list, double* grad_parameters, void* stream);

/* The same for several surfaces of one optical system with ONE launch each way -- all the
 * parametric boundaries of OpticalSystem3D.update (engine.py:971-1018 merges their fields with
 * tf.concat afterwards): every surface writes its rows of the system's merged (M, 9) block
 * directly, and a surface with `copy_from` (a fixed boundary: target, stop) has its rows copied
 * into its place, so the merged block needs no concatenation.  At most TFRT_MAX_SURFACES
 * descriptors (a host array; they travel by value in the kernel arguments).  The reverse is the
 * gather form of tfrt_param_faces_backward per surface (corner lists required). */
#define TFRT_MAX_SURFACES 8
typedef struct tfrt_face_surface {
  const double* zero_points;   /* (V,3)  unused with copy_from */
  const double* vectors;       /* (V,3) */
  const double* parameters;    /* (V,) */
  const int32_t* faces;        /* (F,3) vertex indices */
  int64_t n_vertices, n_faces;
  double* face_verts;          /* (F,9) out: this surface's rows of the merged block */
  double* norm;                /* (F,3) out, or NULL */
  const double* copy_from;     /* (F,9) fixed faces to copy instead, or NULL */
} tfrt_face_surface;
typedef struct tfrt_face_surface_grad {
  const double* grad_face_verts;  /* (F,9) or NULL */
  const double* grad_norm;        /* (F,3) or NULL */
  const double* face_verts;       /* (F,9) forward result (needed with grad_norm) */
  const uint8_t* update_mask;     /* (F,3) or NULL */
  const double* vectors;          /* (V,3) */
  const int32_t* corner_start;    /* (V+1) */
  const int32_t* corner_list;     /* face * 3 + corner, grouped by vertex */
  int64_t n_vertices;
  double* grad_parameters;        /* (V,) out (overwritten) */
  /* (F,9) rows or NULL: the faces' four sums (tfrt_scene3d.face_sums: the first four doubles of
   * every row; the other five are not read) in place of grad_face_verts -- expanded per face
   * through face_verts (required then), the normal's half added as before.
   * Both given: TFRT_E_BADARG, like all three upstreams NULL. */
  const double* grad_face_sums;
} tfrt_face_surface_grad;
int tfrt_param_faces_forward_multi(const tfrt_face_surface* surfaces, int32_t n_surfaces,
                                   void* stream);
int tfrt_param_faces_backward_multi(const tfrt_face_surface_grad* surfaces, int32_t n_surfaces,
                                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser step, parameter side (SGD_Optimizer.process_gradient / single_step,
 * tfrt/optimizer.py:223-257 and :316).
 *
 * tfrt_sgd_process: per element, in the tensors' own dtype (TFRT_F32 / TFRT_F64)
 *     g = isfinite(grad) ? grad : 0            (optimizer.py:226-229)
 *     g = g * scale                            (:233, scale = lr_scale*individual_lr*learning_rate)
 *     g = min(max(g, -clip), clip)             (:236-247, clip >= 0)
 *     processed[i] = g                         (skipped when processed == NULL)
 *     param[i]    -= sgd_learning_rate * g     (skipped when param == NULL; the Keras SGD
 *                                               apply of optimizer.py:316, no momentum)
 * `processed` may alias `grad`.
 */
int tfrt_sgd_process(const void* grad, void* processed, void* param, int64_t n, int32_t dtype,
                     double scale, double clip, double sgd_learning_rate, void* stream);

/* Same, with {scale, clip, sgd_learning_rate} read from three float64 on the DEVICE: the values
 * change from step to step (learning-rate schedules, optimizer.py:384-389) while a captured
 * launch graph of the step replays unchanged. */
int tfrt_sgd_process_dev(const void* grad, void* processed, void* param, int64_t n, int32_t dtype,
                         const double* hyper, void* stream);

/* tfrt_sgd_process_dev for up to 8 float64 tensors in ONE launch (the per-parameter loop of
 * optimizer.py:223-247, 316): host arrays of n_tensors device pointers (`processed` / `param`
 * and their entries may be NULL as above) and element counts; `hyper` holds {scale, clip,
 * sgd_learning_rate} per tensor, 3 * n_tensors float64 on the device. */
/* The second stage of tfrt_goal_error3d's error sum, left to the caller
 * (tfrt_goal_error3d_deferred): a dependent launch costs ~4.5 us whatever it does, and nothing on
 * the device waits for the sum. */
typedef struct tfrt_goal_pending {
  const double* partial;       /* per-workgroup partial sums (in the goal workspace) */
  int32_t n_partial;
  const int32_t* n_finished;   /* device count of finished rays */
  int32_t n_fields;
  double* error_out;           /* {sum, n_terms, mean} */
  const int32_t* tests_lo_hi;  /* the trace's test count (two int32) or NULL */
  int64_t* tests_total;        /* running total it is added to, or NULL */
  /* A reverse sweep over an in-place tape (tfrt_scene3d.in_place) whose trace was not asked for
   * ray sets counts for itself: per partial sum two int32 {finished rays, passes the wavefront's
   * rays entered}.  When given, the number of error terms and the trace's test count (passes x
   * n_faces) are summed from them instead of being read through n_finished / tests_lo_hi, and
   * left in counts_tail ([1] finished total, [4] / [5] test count) if that is given too. */
  const int32_t* partial_counts;
  int64_t n_faces;
  int32_t* counts_tail;
} tfrt_goal_pending;

int tfrt_sgd_process_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, const int64_t* n, const double* hyper,
                           void* stream);

/* ... and finishes a pending error sum in one more workgroup of the same launch. */
int tfrt_sgd_process_multi_finish(int32_t n_tensors, const void* const* grad,
                                  void* const* processed, void* const* param, const int64_t* n,
                                  const double* hyper, const tfrt_goal_pending* pending,
                                  void* stream);

/* tfrt_sgd_process_multi with the Keras SGD momentum rule (optimizer.py:128-132 with momentum
 * assigned): `hyper` holds {scale, clip, sgd_learning_rate, momentum, nesterov} per tensor,
 * 5 * n_tensors float64 on the device, and velocity[k] is a persistent float64 buffer of n[k]
 * elements per tensor (zero before the first step).  Per element, after the processing above,
 *     if momentum == 0:  param[i] -= sgd_learning_rate * g        (velocity[i] NOT written)
 *     else:              v = momentum * velocity[i] - sgd_learning_rate * g;  velocity[i] = v
 *                        param[i] += momentum * v - sgd_learning_rate * g     (nesterov != 0)
 *                        param[i] += v                                        (nesterov == 0)
 * every product and difference rounded on its own (no fused multiply-add).  `processed` and its
 * entries may be NULL; `param`, `velocity` and their entries (for n[k] > 0) may not.  `processed`
 * may alias `grad`; `velocity` aliases neither `grad` nor `param`. */
int tfrt_sgd_momentum_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                            void* const* param, void* const* velocity, const int64_t* n,
                            const double* hyper, void* stream);

/* ... and finishes a pending error sum in one more workgroup of the same launch. */
int tfrt_sgd_momentum_multi_finish(int32_t n_tensors, const void* const* grad,
                                   void* const* processed, void* const* param,
                                   void* const* velocity, const int64_t* n, const double* hyper,
                                   const tfrt_goal_pending* pending, void* stream);

/* tfrt_sgd_process_multi with the Keras Adam rule (non-amsgrad; the reference hands its processed
 * gradients to a Keras optimiser object, and Adam is the one its users reach for next).  `hyper`
 * holds {scale, clip, adam_learning_rate, beta1, beta2, epsilon} per tensor, 6 * n_tensors float64
 * on the device; m[k] and v[k] are persistent float64 buffers of n[k] elements per tensor (zero
 * before the first step); `state` holds {t, p1, p2} per tensor, 3 * n_tensors float64 on the
 * device, {0, 1, 1} before the first step.  One launch is one step of every tensor in it:
 *     t  = t + 1;   p1 = p1 * beta1;   p2 = p2 * beta2      (running products, not pow(): exact
 *                                                            IEEE products, reproducible anywhere)
 *     lr_t = adam_learning_rate * sqrt(1 - p2) / (1 - p1)
 * and per element, with g the gradient after the processing above (non-finite -> 0, scale, clip),
 *     m[i] = beta1 * m[i] + (1 - beta1) * g
 *     v[i] = beta2 * v[i] + (1 - beta2) * (g * g)
 *     param[i] -= lr_t * m[i] / (sqrt(v[i]) + epsilon)
 * every product, sum, difference, quotient and square root rounded on its own (no fused
 * multiply-add; float64 sqrt and / are correctly rounded), (1 - beta) computed on the device, the
 * expressions evaluated left to right as written.
 *
 * The step state: the launch reads {p1, p2} and advances {t, p1, p2} itself, so a captured graph
 * counts its replays and every hyper value may change between them.  In each workgroup one thread
 * reads its tensor's state before the workgroup touches an element and, once the workgroup's work is
 * issued, adds 1 to `*ticket` (acquire-release, device scope).  The workgroup that draws the last
 * ticket -- every other one has read the state by then -- writes the advanced state of all
 * n_tensors tensors (tensors with n[k] == 0 included) and stores 0 to the ticket.  No workgroup can
 * see the advanced value and nothing depends on the order workgroups run in.  `ticket` is one
 * uint32 on the device, 0 before the first launch and left 0 by every launch; launches that may
 * run concurrently (different streams) need a ticket each.
 *
 * `processed` and its entries may be NULL; `param`, `m`, `v` and their entries (for n[k] > 0),
 * `state` and `ticket` may not.  `processed` may alias `grad`; m and v alias nothing else. */
int tfrt_adam_multi(int32_t n_tensors, const void* const* grad, void* const* processed,
                    void* const* param, void* const* m, void* const* v, const int64_t* n,
                    const double* hyper, double* state, uint32_t* ticket, void* stream);

/* ... and finishes a pending error sum in one more workgroup of the same launch. */
int tfrt_adam_multi_finish(int32_t n_tensors, const void* const* grad, void* const* processed,
                           void* const* param, void* const* m, void* const* v, const int64_t* n,
                           const double* hyper, double* state, uint32_t* ticket,
                           const tfrt_goal_pending* pending, void* stream);

/* y = A x, A in CSR form (int64 indices, f64 values): the accumulator (optimizer.py:250-255)
 * and smoother (optimizer.py:277-282) products for the sparse matrices the mesh tools
 * produce (mesh_tools.py:221-421).  x and y must not alias. */
int tfrt_csr_matvec(const int64_t* crow_indices, const int64_t* col_indices, const double* values,
                    const double* x, double* y, int64_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scene description shared by the 3-D entry points (the merged boundary set of
 * OpticalSystem3D._merge_boundaries, tfrt/engine.py:971-1018: optical, stop, target order).
 */
typedef struct tfrt_scene3d {
  const double* face_verts; /* (M,9) f64 */
  const int32_t* catagory;  /* (M) TFRT_OPTICAL / _STOP / _TARGET */
  const int32_t* mat_in;    /* (M) material index opposite the norm, or NULL ("value" mode) */
  const int32_t* mat_out;   /* (M) material index on the norm side, or NULL */
  const double* n_in;       /* (M) per-face refractive index ("value" mode) or NULL */
  const double* n_out;      /* (M) or NULL */
  int64_t n_faces;          /* M */
  /* n_table[m * n_table_stride + source_ray] = n_m(wavelength of that source ray); the
   * host evaluates the material callables once per source ray (wavelength is inherited
   * unchanged, tfrt/operation.py:238-239).  NULL in "value" mode. */
  const double* n_table;
  int64_t n_table_stride;
  int32_t n_materials;
  double intersect_epsilion; /* OpticalSystemBase kwargs, tfrt/engine.py:174-190 */
  double size_epsilion;
  double ray_start_epsilion;
  /* (M) u8, backward only: 0 = this face's vertices are constants (e.g. a target plane),
   * skip its gradient accumulation; NULL = accumulate for every face. */
  const uint8_t* face_grad_mask;
  /* (M) i32, optional: a permutation of the face indices that puts spatially close faces next
   * to each other (e.g. Morton order of the centroids).  When given (and M >= 64) the trace
   * visits faces in clusters of 16 consecutive entries behind a bounding-sphere test (a
   * two-level conservative filter); results are identical to the all-pairs path (NULL). */
  const int32_t* cluster_order;
  /* 1: every source ray has the same wavelength -- n_table has ONE column, n_table[m *
   * n_table_stride] = n_m(that wavelength), read by every ray (a source made from one wavelength,
   * e.g. dev/hexalens.py:48 `[drawing.YELLOW]`).  0: one column per source ray. */
  int32_t n_table_uniform;
  /* Reverse sweep only.  0 (default): the 9 face-gradient terms of every ray are summed with
   * float64 atomics (LDS windows, then global): fastest, but float64 addition is not
   * associative, so the last bits of a face's sum depend on the arrival order and differ from
   * run to run.  1: ordered mode -- per pass the terms are scaled by a power of two taken from
   * their largest magnitude, rounded to 64-bit integers and summed with integer atomics (exact,
   * hence order-independent), then converted back: bit-identical results on every run, at a
   * resolution of 2^-40 of the pass's largest term. */
  int32_t deterministic;
  /* With cluster_order.  1: the caller hands the source rays over in a COHERENT order --
   * neighbouring rays have neighbouring lines, e.g. sorted along a Hilbert curve through their
   * aperture points (tensorflowraytrace_amd.ops.ray_order).  A wavefront of 64 consecutive rays is
   * then tried as ONE narrow bundle that walks the face hierarchy once for all of them
   * (k_intersect_beam; wavefronts that are no narrow bundles are cut, or left to the grouped
   * per-ray walk), and the reverse sweep sums the face gradients of a wavefront's rays before
   * touching memory.  The outputs are what they always are -- every class compacted stably in the
   * order of the rays handed in -- so a caller that sorted its rays maps the ray ids back and
   * restores its own order per pass (the Python engine does).  Results never depend on the flag;
   * with rays that are not coherent it only costs time. */
  int32_t coherent_rays;
  /* With coherent_rays.  0: behind k_intersect_beam the grouped kernel is launched for the
   * wavefronts that are no (few) narrow bundles; their number, summed over the passes, comes back
   * in counts[TFRT_COUNTS_LEN - 1].  1: no such launch -- k_intersect_beam finishes every
   * wavefront itself, cutting it down to single rays if need be: always correct, but slow for
   * rays that are not coherent; meant for a source whose earlier traces left no wavefront over
   * (saves one kernel launch per pass). */
  int32_t coherent_only;
  /* Reverse sweep only, "value" mode (n_in / n_out given): (M) f64 each, ACCUMULATED into, or
   * NULL -- d error / d n_in[face], d error / d n_out[face] (tfrt/operation.py:268-272 reads the
   * two fields as ordinary tensors, which a tape can differentiate).  Both or neither. */
  double* grad_n_in;
  double* grad_n_out;
  /* Forward only, optional: clear_count f64 at clear_buffer are set to zero by the trace's set-up
   * launch -- the (M,9) block a reverse sweep will ACCUMULATE into (tfrt_trace3d_backward,
   * tfrt_trace3d_backward_goal), cleared without a launch of its own.  NULL / 0: nothing. */
  double* clear_buffer;
  int64_t clear_count;
  /* With coherent_rays and cluster_order, max_passes >= 1.  1: ALL passes of the trace run in ONE
   * launch with every ray kept in its slot (k_trace_inplace): a lane intersects, classifies and
   * refracts its ray pass after pass, the tape holds one record per pass at slot = ray index, and
   * nothing is compacted between passes -- StandardReaction emits exactly one child per active ray
   * (tfrt/operation.py:255-307), so the reference's per-pass boolean_mask (tfrt/engine.py:2069-2111)
   * is not needed to go on tracing.  The reference's output order is made afterwards: a scan of
   * per-wavefront class counts always (it fills `counts`), and a gather of the class rows only when
   * tfrt_trace3d_forward is given somewhere to put them (any tfrt_ray_out with rays, or
   * `unfinished`) -- or later by tfrt_trace3d_compact.  Outputs, counts and gradients are those of
   * the per-pass path bit for bit (reverse-sweep sums: to the last bits of a differently ordered
   * sum).  Every wavefront is finished by the one kernel, however wide its bundle (like
   * coherent_only, which it implies): meant for sources whose earlier traces left no wavefront
   * over.  The SAME value must be passed to the reverse sweep.  Ignored (per-pass path) when the
   * conditions above do not hold.
   * `counts`: a forward call that is given no room for ray sets does not run the scan either -- a
   * folded reverse sweep (tfrt_trace3d_backward_goal) needs neither and counts the finished rays
   * and the tests itself; tfrt_trace3d_compact then fills `counts` together with the sets.
   * 2: as 1, and the FINISHED rays are handed out where they are -- `finished` (capacity >= n_rays,
   * the only class given) receives ray r's finished row (start, hit point on the target) at
   * column r, finished->face[r] = the target face hit or -1 when ray r did not finish (its column
   * then holds the source ray: finite stand-in values that carry no gradient), finished->ray_id[r]
   * = the number of passes ray r entered; nothing is compacted, `counts` is not written.  For
   * error functions that work row by row on fixed-shape tensors (no ray count to read back:
   * tfrt/optimizer.py:216-220 with a mask instead of a boolean_mask); tfrt_trace3d_backward then
   * takes grad_finished in the same layout (capacity >= n_rays, no other class gradient). */
  int32_t in_place;
  /* With in_place, optional: (n_rays) i32, ray_slot[r] = the column of src_rays that holds the
   * CALLER's ray r -- the rays were handed over in another order than the caller's own, e.g. the
   * coherent order of tfrt_ray_order (ray_slot is that permutation's inverse).  The ray sets are
   * then compacted in the caller's numbering: every class lists, pass after pass, its rays by
   * ascending r with ray_id = r, exactly what a trace of the rays in the caller's order returns
   * (tfrt/engine.py:2069-2111, 1379-1403), and class gradients are read in that order by the
   * reverse sweep -- no tfrt_restore_order afterwards.  NULL: the order of src_rays. */
  const int32_t* ray_slot;
  /* With in_place, optional: (ceil(n_rays / 64)) i32, a permutation of the GROUPS of 64 consecutive
   * columns of src_rays -- the order in which k_trace_inplace and the folded goal sweep of an
   * in-place trace (tfrt_trace3d_backward_goal's steady-state kernel) take them: workgroup b works
   * on group wave_schedule[b], the expensive groups first (tfrt_trace3d_wave_schedule makes one).
   * A hint about time only: every group is traced and swept exactly as without it, and whatever is
   * stored per wavefront is stored at the wavefront's own index, so outputs, counts and the error
   * sum are the same bit for bit (the face gradient's atomics were unordered before).  It MUST be
   * a permutation: a group that is missing is not traced.  Read by the device when the launch
   * runs, so a captured launch sees later contents.  NULL: index order.  No reference counterpart
   * (the reference has no wavefronts). */
  const int32_t* wave_schedule;
  /* Reverse sweep only.  0 (default): grad_face_verts is the (M,9) block of face-vertex gradients.
   * 1: the four-sum form -- the first FOUR doubles of a face's row of that (M,9) block receive
   * the sums, over the rays that hit the face, of the gradient w.r.t. C = (P1 - P0) x (P2 - P0)
   * (three) and w.r.t. the hit parameter's numerator (one); the row's other five doubles are not
   * written.  A face's nine vertex gradients are linear in these four with coefficients of the
   * face alone, so the sweep neither forms nor sums the nine per ray; whoever reads the block
   * expands once per face (tfrt_face_surface_grad.grad_face_sums does; csrc/trace_math.h
   * face_sums_expand).  The rows stay where they are, so a face's row is its own in either form
   * (frozen faces' rows stay zero) and clear_buffer / clear_count are what they were.  Honoured
   * by the one-launch sweeps of coherent rays (k_backward_chain, k_backward_chain_goal_inplace);
   * a call that would take any other route (deterministic, rays that are not coherent, more
   * passes than the chain holds without in_place) returns TFRT_E_UNSUPPORTED before it launches
   * anything and never writes the other form.  Pass the same value to the forward. */
  int32_t face_sums;
} tfrt_scene3d;

/* One class of output rays (finished / active history / stopped / dead), compacted stably in
 * source order pass after pass, exactly like the reference's per-pass boolean_mask + concat
 * (tfrt/engine.py:2069-2111, 1379-1399). */
typedef struct tfrt_ray_out {
  void* rays;       /* 6 x capacity ray block (state dtype) or NULL if not compiled */
  int32_t* ray_id;  /* (capacity) index of the source ray each output row descends from */
  int32_t* face;    /* (capacity) merged face index hit (-1 for dead rays) */
  int64_t capacity; /* row stride of `rays` */
} tfrt_ray_out;

/* Bytes of scratch+tape the trace needs.  The SAME buffer must be passed to forward and,
 * untouched, to backward. */
size_t tfrt_trace3d_workspace_bytes(int64_t n_rays, int64_t n_faces, int32_t max_passes,
                                    int32_t state_dtype);

/* Number of int32 in `counts`: per pass 8 ints {n_active,n_finished,n_stopped,n_dead,
 * base_active,base_finished,base_stopped,base_dead}, then 8 trailing ints:
 * {total_active,total_finished,total_stopped,total_dead,n_tests_lo,n_tests_hi,error,
 *  wavefronts left to the grouped kernel (coherent-ray traces)}. */
#define TFRT_COUNTS_PER_PASS 8
#define TFRT_COUNTS_LEN(max_passes) (8 * ((max_passes) + 1))

/* Whole trace, forward.  Replaces OpticalEngine.ray_trace -> single_pass ->
 * process_projection_3D -> OpticalSystem3D.intersect/_intersection ->
 * geometry.line_triangle_intersect, then StandardReaction.main -> geometry.snells_law_3D
 * (tfrt/engine.py:2311-2330, 2193-2302, 1988-2191, 1020-1166; tfrt/geometry.py:191-320,
 * 671-753; tfrt/operation.py:255-307).
 *
 *   src_rays   6 x src_stride ray block, n_rays valid columns
 *   unfinished ray block (6 x n_rays) receiving the rays still active after the last pass
 *              (what single_pass returns, engine.py:2302), + their source ids; may be NULL
 *   counts     TFRT_COUNTS_LEN(max_passes) int32, written by the device
 */
int tfrt_trace3d_forward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                         const tfrt_scene3d* scene, double new_ray_length,
                         double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                         uint32_t flags, tfrt_ray_out* finished, tfrt_ray_out* active,
                         tfrt_ray_out* stopped, tfrt_ray_out* dead, void* unfinished,
                         int32_t* unfinished_id, int32_t* counts, void* workspace,
                         size_t workspace_bytes, void* stream);

/* The class outputs of an in-place trace (tfrt_scene3d.in_place) that tfrt_trace3d_forward was
 * given no room for: every class compacted stably into `finished` / `active` / `stopped` / `dead`
 * (+ `unfinished`), rows recomputed from the tape in `workspace`, exactly as a forward call with
 * these outputs would have left them, and `counts` filled like that call would have filled it (its
 * error flag is set when a capacity is exceeded).  Also records every tape entry's output row,
 * which tfrt_trace3d_backward / _backward_goal need to read class gradients (grad_finished, ...):
 * call it (or give forward its outputs) before a reverse sweep that is handed any.  Same
 * src_rays / n_rays / max_passes / state_dtype / flags / dead_ray_length as the forward call;
 * ray_slot as tfrt_scene3d.ray_slot (NULL: the sets in the order of src_rays).
 * Replaces the ray-set properties of tfrt/engine.py:1379-1403 for a trace whose sets are cut
 * lazily. */
int tfrt_trace3d_compact(const void* src_rays, int64_t src_stride, int64_t n_rays,
                         double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                         uint32_t flags, tfrt_ray_out* finished, tfrt_ray_out* active,
                         tfrt_ray_out* stopped, tfrt_ray_out* dead, void* unfinished,
                         int32_t* unfinished_id, int32_t* counts, int64_t n_faces,
                         const int32_t* ray_slot, void* workspace, size_t workspace_bytes,
                         void* stream);

/* 1 when tfrt_trace3d_forward takes the in-place route for this scene, ray count and pass count
 * (tfrt_scene3d.in_place is honoured), 0 when it runs the per-pass launch sequence, < 0 on bad
 * arguments.  A caller that hands over ray_slot needs to know which of the two orders its ray
 * sets come back in. */
int tfrt_trace3d_in_place(const tfrt_scene3d* scene, int64_t n_rays, int32_t max_passes);

/* Work an in-place trace actually executed (measurement; no reference counterpart -- the reference
 * executes every pair, tfrt/engine.py:1103-1166): executed[0] = (ray, face) pairs that reached the
 * exact float64 test of tfrt/geometry.py:286-311, executed[1] = candidate faces tested as triangles
 * against a wavefront's bundle; both summed over the passes of the trace whose tape is in
 * `workspace`.  `counts` tells how many pairs the trace DECIDED (n_tests). */
int tfrt_trace3d_executed(int64_t n_rays, int64_t n_faces, int32_t max_passes, int32_t state_dtype,
                          const void* workspace, size_t workspace_bytes, int64_t* executed,
                          void* stream);

/* The wavefront schedule for the NEXT in-place traces of these rays in this order
 * (tfrt_scene3d.wave_schedule), from the work the trace whose tape is in `workspace` recorded per
 * wavefront: schedule_out receives ceil(n_rays / 64) i32, the groups of 64 rays listed by cost
 * class (passes entered, candidate faces tested), the heaviest class first, ascending inside a
 * class; equal costs give 0, 1, 2, ...  One small launch on `stream`; meant to run when a step's
 * launch sequence is set up, not inside it.  Same n_rays / n_faces / max_passes / state_dtype as
 * the forward call.  No reference counterpart. */
int tfrt_trace3d_wave_schedule(int64_t n_rays, int64_t n_faces, int32_t max_passes,
                               int32_t state_dtype, const void* workspace, size_t workspace_bytes,
                               int32_t* schedule_out, void* stream);

/* What tfrt_trace3d_wave_schedule reads (measurement and tests; no reference counterpart): the
 * count rows the in-place trace whose tape is in `workspace` left per wavefront, copied densely
 * into rows_out, (max_passes + 2) x W u32 -- rows 0 .. max_passes-1 the four class counts of each
 * pass, one byte each (non-zero: the wavefront entered the pass), then the (ray, face) pairs that
 * reached the exact test and the candidate faces tested against the bundle.  Returns W > 0, the
 * trace's wavefronts (of 64 rays, or of 32: then two to a group of the schedule), or < 0 on bad
 * arguments; rows_out NULL: only W. */
int tfrt_trace3d_wave_rows(int64_t n_rays, int64_t n_faces, int32_t max_passes, int32_t state_dtype,
                           const void* workspace, size_t workspace_bytes, uint32_t* rows_out,
                           void* stream);

/* Reverse sweep over the tape left in `workspace` by tfrt_trace3d_forward with the same
 * arguments.  Replaces the ray-dependent part of tape.gradient in
 * SGD_Optimizer.process_gradient, tfrt/optimizer.py:216-220.
 *
 *   grad_finished/active/stopped/dead : 6 x capacity f64 blocks (row stride = the matching
 *              tfrt_ray_out.capacity of the forward call) or NULL
 *   grad_face_verts (M,9) f64, ACCUMULATED into (caller zeroes); with tfrt_scene3d.face_sums only
 *                   the first four doubles of every row (the faces' four sums)
 *   grad_src_rays   6 x n_rays f64 or NULL
 */
int tfrt_trace3d_backward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                          const tfrt_scene3d* scene, double new_ray_length,
                          double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                          const double* grad_finished, int64_t cap_finished,
                          const double* grad_active, int64_t cap_active,
                          const double* grad_stopped, int64_t cap_stopped,
                          const double* grad_dead, int64_t cap_dead, double* grad_face_verts,
                          double* grad_src_rays, const int32_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Built-in image-forming error of the reference's optimisation scripts
 * (dev/hexalens.py:144-168: output = stack(finished[field_c]), goal = f(inherited source
 * fields), error = tf.math.squared_difference(output, goal)) evaluated on the device, with its
 * gradient seed, so that an optimiser step reads no ray count back and is a fixed launch
 * sequence.  Replaces the user error function + the first node of tape.gradient
 * (tfrt/optimizer.py:216-220) for error functions of that form.
 *
 *   finished_rays  6 x capacity ray block written by tfrt_trace3d_forward (state dtype)
 *   finished_id    (capacity) source-ray index per finished row (tfrt_ray_out.ray_id)
 *   counts         the device-side counters of that trace (TFRT_COUNTS_LEN(max_passes) int32):
 *                  the number of finished rows and the trace's test count are read from its tail
 *   fields[c]      row of the ray block (0..5 = x_start..z_end) compared with goal column c
 *   goal           f64 goal table, entry (c, source ray r) at goal[c * goal_stride +
 *                  r * goal_ray_stride]: one contiguous column per field (goal_ray_stride 1) or
 *                  one row per ray (goal_stride 1, goal_ray_stride n_fields)
 *   grad_finished  6 x capacity f64: rows fields[c] receive 2 * (output - goal) for the
 *                  finished rows; other rows and rows beyond n_finished are left untouched
 *                  (zero them once: tfrt_trace3d_backward reads finished rows only)
 *   error_out      3 f64: {sum of the error terms, number of terms, sum / max(terms, 1)}; the
 *                  sum is formed in a fixed order (bit-identical from run to run)
 *   zero_buffer    optional: zero_count f64 cleared by the same launch (the (M,9) face-gradient
 *                  block the reverse sweep accumulates into), or NULL / 0
 *   tests_total    optional device int64: incremented by the trace's ray-face test count
 *   workspace      tfrt_goal_error3d_workspace_bytes(capacity) bytes of scratch
 */
size_t tfrt_goal_error3d_workspace_bytes(int64_t capacity);
int tfrt_goal_error3d(const void* finished_rays, int64_t capacity, const int32_t* finished_id,
                      int32_t state_dtype, const int32_t* counts, int32_t max_passes,
                      const int32_t* fields, int32_t n_fields, const double* goal,
                      int64_t goal_stride, int64_t goal_ray_stride, double* grad_finished,
                      double* error_out, double* zero_buffer, int64_t zero_count,
                      int64_t* tests_total, void* workspace, size_t workspace_bytes,
                      void* stream);

/* The same without the second stage of the sum: `pending` (host struct) is filled in and whoever
 * runs next finishes it -- tfrt_sgd_process_multi_finish in a spare workgroup of the parameter
 * update's launch, or tfrt_goal_finish (the launch tfrt_goal_error3d would have made). */
int tfrt_goal_error3d_deferred(const void* finished_rays, int64_t capacity,
                               const int32_t* finished_id, int32_t state_dtype,
                               const int32_t* counts, int32_t max_passes, const int32_t* fields,
                               int32_t n_fields, const double* goal, int64_t goal_stride,
                               int64_t goal_ray_stride, double* grad_finished, double* error_out,
                               double* zero_buffer, int64_t zero_count, int64_t* tests_total,
                               void* workspace, size_t workspace_bytes,
                               tfrt_goal_pending* pending, void* stream);
int tfrt_goal_finish(const tfrt_goal_pending* pending, void* stream);

/* DensityError: the columns that count, taken together, must land with the density `goal` on an
 * (ny x nx) grid of bins over the domain [x0, x1] x [y0, y1] -- the soft-histogram form of
 * tfrt/analyze.py:134-290 (DistributionDifferential), which bins hard and has no gradient.  Four
 * launches (clear `hq`, splat, bins, seed), no host read, no allocation: captured with the rest of
 * a step.
 *
 * A column i counts if mask is NULL or mask[i] >= 0 (tfrt_ray_out.face of an in-place trace with
 * the finished rows at the rays' own columns) and its coordinates x = rows[row_x], y = rows[row_y]
 * (converted to f64) are finite.  Every operation below is rounded on its own (no contraction).
 *   outside the closed domain on any axis: nothing goes to the histogram; the error gains
 *     oob_weight * (ex^2 + ey^2), ex = max(x0 - x, 0) + max(x - x1, 0), and the gradient is the
 *     derivative of that expression;
 *   inside: u = (x - x0) * sx - 0.5, i0 = floor(u), t = u - i0; weight 1 - t goes to column
 *     clamp(i0, 0, nx - 1), weight t to column clamp(i0 + 1, 0, nx - 1) (the outer half bin piles
 *     onto the edge bin); y alike, the four weights are the products (two weights without y).
 *   Each weight w is added to its bin as the integer rint(w * 2^32), half to even, in the int64
 *   histogram hq: the sum does not depend on the order of the atomics.  H = hq / 2^32, s = ||H||;
 *   s == 0: E_hist = sum g^2 and every pull is 0; else h = H / s, r = h - g, E_hist = sum r^2 and
 *   the pull on bin b is D_b = (2 / s) (r_b - h_b sum_c h_c r_c).  A counting ray inside gets
 *     d/dx = sx [(1 - ty)(D[j0,i1] - D[j0,i0]) + ty (D[j1,i1] - D[j1,i0])], d/dy symmetric
 *   (clamped indices; quantisation treated as the identity).  error = E_hist + penalties; all of
 *   its sums have a fixed shape and order: two runs give the same bits.
 *
 *   rows, stride    ray block in the state dtype, entry (row, i) at rows[row * stride + i], n columns
 *   row_x, row_y    rows (0..5) of x and y; row_y = -1: one field (then ny must be 1)
 *   goal            (ny, nx) f64, non-negative, L2-normalised by the caller
 *   sx, sy          nx / (x1 - x0), ny / (y1 - y0), computed by the caller in f64
 *   grad            f64 block, entry (row, i) at grad[row * grad_stride + i]: rows row_x and row_y
 *                   are written for EVERY column (0 where a ray does not count); no other row is
 *   error_out       3 f64 {error, 1, error}: one error term, the mean is the sum
 *   hq              nx * ny int64, cleared and filled by this call
 *   splat_variant   0: the per-workgroup LDS histogram up to 4,096 bins, global 64-bit atomics
 *                   above; 1 / 2 force one of them (1 with more than 4,096 bins: TFRT_E_BADARG)
 *   workspace       tfrt_density_error_workspace_bytes(n, nx, ny) bytes (0: bad arguments)
 * nx, ny >= 1, nx * ny <= 65,536, 0 <= n < 2^31 (n == 0 is legal: error = sum g^2).
 */
size_t tfrt_density_error_workspace_bytes(int64_t n, int32_t nx, int32_t ny);
int tfrt_density_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                       const int32_t* mask, int32_t row_x, int32_t row_y, const double* goal,
                       int32_t nx, int32_t ny, double x0, double x1, double sx, double y0,
                       double y1, double sy, double oob_weight, double* grad, int64_t grad_stride,
                       double* error_out, int64_t* hq, int32_t splat_variant, void* workspace,
                       size_t workspace_bytes, void* stream);

/* tfrt_density_error with FIELD CODES in the place of rows: a field is a row of the ray block or a
 * direction cosine of the finished ray's last link (far-field intensity: a density over the
 * outgoing direction).  The same launches and the same workspace as tfrt_density_error; no
 * direction block in memory -- the splat and the seed each recompute the direction from the rows
 * they stream.
 *
 * `rows` is the geometry block of a `dimension`-D trace (d = dimension, 2 or 3): 2d rows, 0..d-1
 * the start of the last link (x, y[, z]), d..2d-1 its end.  Field codes:
 *   c < 2d           block row c
 *   2d <= c < 3d     d_(c - 2d), the direction cosine on axis c - 2d
 * (3-D: x_dir, y_dir, z_dir = 6, 7, 8; 2-D: x_dir, y_dir = 4, 5).  A position and a direction may
 * be mixed (phase space); the two codes must differ.  For a column, every operation an IEEE f64
 * operation rounded on its own, no contraction:
 *   e_a = (double) end_a - (double) start_a                a = x, y[, z]
 *   q   = e_x*e_x + e_y*e_y [+ e_z*e_z]                    summed left to right
 *   L   = sqrt(q),  d_a = e_a / L
 * With at least one direction field, a column with any non-finite geometry row, or with L not
 * finite or not > 0, is a column whose coordinates are not finite: it does not count.  The value
 * v_k of field k then goes through exactly the expressions of tfrt_density_error (domain test,
 * penalty, bilinear weights, histogram, pulls), which also give gv_k = d error / d v_k, there
 * written to the gradient rows.  Here, with a direction field:
 *   t   = the sum over the direction fields k, in field order, of gv_k * d_(a_k)
 *   G_b = ((gv_k of the direction field of axis b, else 0.0) - t * d_b) / L         every axis b
 *   grad[end_b]   =  G_b   (+ gv_k of a position field that names that row, added last)
 *   grad[start_b] = -G_b   (+ likewise)
 * and ALL 2d rows of `grad` are written for every column, 0.0 where a column does not count.
 * With position fields only (both codes < 2d) the rows written and every bit are
 * tfrt_density_error's.
 *
 * With rows in float32 the subtraction end - start cancels: a direction is good to about
 * eps32 * max|coordinate| / L, not to eps32.
 *
 *   dimension          2 or 3; rows has 2 * dimension rows of `stride`
 *   field_x, field_y   codes in [0, 3 * dimension); field_y = -1: one field (then ny must be 1);
 *                      field_x != field_y
 *   grad               f64 block of 2 * dimension rows of `grad_stride`
 * Everything else as for tfrt_density_error.
 */
int tfrt_density_error_fields(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                              int32_t dimension, const int32_t* mask, int32_t field_x,
                              int32_t field_y, const double* goal, int32_t nx, int32_t ny,
                              double x0, double x1, double sx, double y0, double y1, double sy,
                              double oob_weight, double* grad, int64_t grad_stride,
                              double* error_out, int64_t* hq, int32_t splat_variant,
                              void* workspace, size_t workspace_bytes, void* stream);

/* SpotError: the columns that carry the same group label must meet in one point -- the sum over
 * the rays of the squared distance to the CENTROID of their own group (the squared RMS spot size
 * times the ray count), wherever the centroids lie.  Four launches (clear `acc`, accumulate, seed,
 * finish), no host read, no allocation: captured with the rest of a step.
 *
 * With k the number of fields (1 or 2), a column i COUNTS if mask is NULL or mask[i] >= 0
 * (tfrt_ray_out.face of an in-place trace with the finished rows at the rays' own columns), and
 * terms = k * (number of counting columns).  Coordinates x = rows[row_x], y = rows[row_y] are
 * converted to f64; every operation below is an IEEE f64 operation rounded on its own (no
 * contraction).  A counting column goes to exactly one of four cases, tried in this order:
 *   a coordinate is non-finite: no error, gradient 0;
 *   no spot: s = perm ? perm[i] : i, label = group[s]; s outside [0, n_source) or label outside
 *     [0, n_groups): no error, gradient 0 (the label -1 excludes a ray; nothing is read out of
 *     bounds, whatever perm and group hold);
 *   outside the closed domain on any axis: nothing goes to `acc`; the error gains
 *     oob_weight * (ex^2 + ey^2), ex = max(x0 - x, 0) + max(x - x1, 0), and the gradient is the
 *     derivative of that expression (as tfrt_density_error);
 *   inside: qx = (int64) min(max(rint((x - x0) * qsx), 0), 2^qbits), half to even, qy alike;
 *     {1, qx, qy} is added to record `label` of `acc` with 64-bit integer atomics: the sums do not
 *     depend on the order of the atomics.
 * Once every column is in, a group with count > 0 has cx = x0 + ((double) Sx / (double) count) / qsx
 * and cy alike.  An inside ray has dx = x - cx, the terms dx * dx and dy * dy and the gradient rows
 * 2 * dx and 2 * dy: exact without a derivative of the centroid, because the residuals of a group
 * sum to zero (up to the quantisation, half a step of 1 / qsx).  error = the sum of the inside
 * terms + the sum of the penalties; all sums have a fixed shape and order: two runs give the same
 * bits.
 *
 *   rows, stride    ray block in the state dtype, entry (row, i) at rows[row * stride + i], n columns
 *   row_x, row_y    rows (0..5) of x and y; row_y = -1: one field (qy = 0, Sy stays 0)
 *   group           n_source int32 labels, one per SOURCE ray
 *   perm            n int32, the source ray of column i; or NULL: column i is source ray i
 *   n_groups        G, 1 <= G <= 2^20
 *   qbits           1..52; the caller uses min(52, 62 - bit_length(n_source)).  n >= 2^(62 - qbits)
 *                   is refused: n * 2^qbits < 2^62, no sum overflows
 *   qsx, qsy        ldexp(1, qbits) / (x1 - x0) and / (y1 - y0), computed by the caller in f64
 *   grad            f64 block, entry (row, i) at grad[row * grad_stride + i]: rows row_x and row_y
 *                   are written for EVERY column (0 where a ray does not count); no other row is
 *   error_out       3 f64 {error, terms, terms > 0 ? error / terms : NaN}
 *   acc             n_groups records of four int64 {count, Sx, Sy, 0} (32 B: the adds of one ray
 *                   fall into one sector), cleared and filled by this call
 *   variant         0: a per-workgroup table in LDS up to 1,024 groups, global 64-bit atomics
 *                   above; 1 / 2 force one of them (1 with more than 1,024 groups: TFRT_E_BADARG)
 *   workspace       tfrt_spot_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * 0 <= n < 2^31 (n == 0 is legal: {0, 0, NaN}), 0 <= n_source < 2^31.
 */
size_t tfrt_spot_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_spot_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                    const int32_t* mask, int32_t row_x, int32_t row_y, const int32_t* group,
                    int64_t n_source, const int32_t* perm, int32_t n_groups, double x0, double x1,
                    double qsx, double y0, double y1, double qsy, int32_t qbits,
                    double oob_weight, double* grad, int64_t grad_stride, double* error_out,
                    int64_t* acc, int32_t variant, void* workspace, size_t workspace_bytes,
                    void* stream);

/* tfrt_spot_error with FIELD CODES in the place of rows (collimation: the rays of one group must
 * leave parallel -- a spot in direction space; the centroids are then mean direction cosines).
 * The fields, their codes, the column's direction (e, q, L, d), the chain rule from
 * gv_k = d error / d v_k to the 2 * dimension rows of `grad` and the float32 caveat are those of
 * tfrt_density_error_fields, with tfrt_spot_error's expressions for v_k -> {acc, error, gv_k}.
 * With at least one direction field a column with a non-finite geometry row, or with L not finite
 * or not > 0, takes the first of tfrt_spot_error's four cases ("a coordinate is non-finite": no
 * error, gradient 0, counted in `terms`).  The same launches and the same workspace as
 * tfrt_spot_error; with position fields only the rows written and every bit are its.
 *
 *   dimension          2 or 3; rows has 2 * dimension rows of `stride`
 *   field_x, field_y   codes in [0, 3 * dimension); field_y = -1: one field; field_x != field_y
 *   grad               f64 block of 2 * dimension rows of `grad_stride`
 * Everything else as for tfrt_spot_error.
 */
int tfrt_spot_error_fields(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                           int32_t dimension, const int32_t* mask, int32_t field_x,
                           int32_t field_y, const int32_t* group, int64_t n_source,
                           const int32_t* perm, int32_t n_groups, double x0, double x1, double qsx,
                           double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                           double* grad, int64_t grad_stride, double* error_out, int64_t* acc,
                           int32_t variant, void* workspace, size_t workspace_bytes, void* stream);

/* tfrt_density_error_fields with a radiant power per SOURCE ray (a Lambertian emitter sampled
 * uniformly in angle, a spectrum, an apodised pupil, a measured ray file): `weight` holds n_source
 * f64 in [0, 1] -- only ratios matter, the caller divides by the maximum.  The same four launches
 * and the same workspace (tfrt_density_error_workspace_bytes), no host read, no allocation.
 *
 * For a counting column i -- after the case "a coordinate is non-finite", before the domain test --
 *   s = perm ? perm[i] : i;  s outside [0, n_source), or w = weight[s] not finite or not in [0, 1]:
 *     the column does not count: no error, gradient 0 (nothing is read out of bounds, whatever
 *     perm holds).
 * Otherwise everything is tfrt_density_error_fields' with, every operation an IEEE f64 operation
 * rounded on its own:
 *   inside: a bilinear weight b (bx * by; bx with one field) enters its bin as the integer
 *     rint((b * w) * 2^32), half to even (w <= 1: the int64 bins overflow no sooner); the gradient
 *     gv_k is the unweighted expression multiplied by w last;
 *   outside: the penalty oob_weight * (ex^2 + ey^2) and its gradient, each multiplied by w last.
 * s, E_hist and the pulls come from the weighted histogram exactly as in tfrt_density_error.  With
 * a direction field gv_k carries w when it enters the chain rule.  On return the first nx * ny f64
 * of `workspace` hold the pulls D_b (row-major, as `goal`): what a ray made of them can be checked
 * bit for bit, although their own sums over the bins are only reproducible, not portable.
 *
 *   weight      n_source f64, one per SOURCE ray; NULL: TFRT_E_BADARG
 *   n_source    0 <= n_source < 2^31
 *   perm        n int32, the source ray of column i; or NULL: column i is source ray i
 * Everything else as for tfrt_density_error_fields.
 */
int tfrt_density_error_weighted(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                                int32_t dimension, const int32_t* mask, int32_t field_x,
                                int32_t field_y, const double* goal, const double* weight,
                                int64_t n_source, const int32_t* perm, int32_t nx, int32_t ny,
                                double x0, double x1, double sx, double y0, double y1, double sy,
                                double oob_weight, double* grad, int64_t grad_stride,
                                double* error_out, int64_t* hq, int32_t splat_variant,
                                void* workspace, size_t workspace_bytes, void* stream);

/* tfrt_spot_error_fields with a radiant power per SOURCE ray: the centroid of a group is the
 * WEIGHTED mean of its rays and the error the weighted sum of squared distances to it.  `weight`
 * holds n_source f64 in [0, 1] (only ratios matter, the caller divides by the maximum).  The same
 * four launches, no host read, no allocation.
 *
 * The four cases of tfrt_spot_error, with the second one wider.  For a counting column with finite
 * coordinates, s = perm ? perm[i] : i:
 *   no spot: s outside [0, n_source); or w = weight[s] not finite or not in [0, 1]; or
 *     wq = rint(w * 2^wbits) (half to even) == 0; or the label group[s] outside [0, n_groups): no
 *     error, gradient 0.  The weight is read once, behind the index check the label needs.
 * wr = (double) wq * 2^-wbits is exact, and it is the weight used everywhere below: the weighted
 * residuals of a group sum to zero in the quantised quantities.  Every operation an IEEE f64
 * operation rounded on its own:
 *   outside the closed domain: the penalty oob_weight * (ex^2 + ey^2) and its gradient, each
 *     multiplied by wr last;
 *   inside: qx as in tfrt_spot_error; with h = qbits / 2 (rounded down) the product wq * qx goes
 *     into two limbs, so that a position keeps its full qbits: Xhi += wq * (qx >> h),
 *     Xlo += wq * (qx & (2^h - 1)); Yhi, Ylo alike; W += wq; count += 1 (64-bit integer atomics).
 * Every sum stays below n * 2^wbits * 2^ceil(qbits / 2): n >= 2^(62 - wbits - ceil(qbits / 2)) is
 * refused (the bound n < 2^(62 - qbits) of tfrt_spot_error is not asked for here).  A group with
 * W > 0 has
 *   X = ldexp((double) Xhi, h) + (double) Xlo,   cx = x0 + (X / (double) W) / qsx,   cy alike.
 * An inside ray has dx = x - cx, the terms wr * (dx * dx) and wr * (dy * dy) (added in that order)
 * and the gradient rows (2 * dx) * wr and (2 * dy) * wr.  error_out stays
 * {error, k * counting columns, error / terms}.
 *
 *   weight      n_source f64, one per SOURCE ray; NULL: TFRT_E_BADARG
 *   wbits       1..20; the caller uses min(20, 62 - bit_length(n_source) - ceil(qbits / 2))
 *   acc         n_groups records of eight int64 {W, Xhi, Xlo, Yhi, Ylo, count, 0, 0} (64 B: the
 *               adds of one ray fall into one line), cleared and filled by this call
 *   variant     0: a per-workgroup table in LDS (six planes of G int64) up to 512 groups -- the
 *               24 KiB of tfrt_spot_error's table at 1,024 --, global 64-bit atomics above; 1 / 2
 *               force one of them (1 with more than 512 groups: TFRT_E_BADARG)
 *   workspace   tfrt_spot_error_weighted_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * Everything else as for tfrt_spot_error_fields.
 */
size_t tfrt_spot_error_weighted_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_spot_error_weighted(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                             int32_t dimension, const int32_t* mask, int32_t field_x,
                             int32_t field_y, const int32_t* group, const double* weight,
                             int32_t wbits, int64_t n_source, const int32_t* perm,
                             int32_t n_groups, double x0, double x1, double qsx, double y0,
                             double y1, double qsy, int32_t qbits, double oob_weight, double* grad,
                             int64_t grad_stride, double* error_out, int64_t* acc, int32_t variant,
                             void* workspace, size_t workspace_bytes, void* stream);

/* TransportError: sliced optimal transport (Wasserstein-2) of the columns to a target density.
 * Along each of K directions the columns' projections are sorted, the column of mid-rank r among
 * the n_valid that count belongs at the goal's quantile r / n_valid, and the error is the sum of
 * the squared distances to those targets.  The goal enters as one quantile table per direction,
 * built on the host.  No transport map, no overlap of pattern and goal needed; columns that do
 * not count simply take no part.
 *
 * For column i and direction k (c_k, s_k = cos, sin of its angle), coordinates converted to f64,
 * every operation rounded on its own:
 *   - the column counts if mask[i] >= 0 (mask given) and both coordinates are finite;
 *   - xi = (x - x0) * ix, eta = (y - y0) * iy;  p = c * xi + s * eta (two products, one sum; one
 *     field: p = xi);
 *   - key: a = min(0, c) + min(0, s), b = max(0, c) + max(0, s), lo = a - (b - a),
 *     scale = 2^26 / (3 * (b - a)), q = clamp(floor((p - lo) * scale), 0, 2^26 - 2) (a NaN: 0);
 *     a column that does not count has q = 2^26 - 1;
 *   - rank among the n_valid columns that count: first = keys smaller than q, count = keys equal
 *     to q, rank2 = 2 * first + count (-1 for a column that does not count),
 *     u = (first + count * 0.5) / n_valid: ties share the mid-rank, so nothing depends on the
 *     order of the columns;
 *   - target: z = u * Q, m = min(floor(z), Q - 1), f = z - m, t = T_k[m] + f * (T_k[m+1] - T_k[m]);
 *     d = p - t, the term is d * d;
 *   - gradient, summed over k = 0 .. K-1 in that order from 0: gx += ((2 * d) * c) * ix,
 *     gy += ((2 * d) * s) * iy (the targets are constants); zeros for a column that does not count;
 *   - err = {sum of all terms, K * n_valid, sum / terms (NaN without terms)}: per column the terms
 *     are added over k, per lane over its columns, then a fixed-shape workgroup sum and the
 *     workgroups' partial sums in index order -- two runs give the same bits.
 *
 *   rows, stride, n   the columns: element (r, i) at rows[r * stride + i]; 0 <= n <= 2^30
 *   state_dtype       TFRT_F32 / TFRT_F64 / TFRT_F16
 *   dimension         2 or 3: rows is a (2 * dimension)-row geometry block
 *   mask              n int32 or NULL
 *   row_x, row_y      rows of the block, distinct; row_y = -1: one field, and n_directions must be 1
 *                     (its direction is (1, 0) whatever angles_cs holds)
 *   x0, ix, y0, iy    the domain's lower ends and 1 / width, finite, ix, iy > 0
 *   angles_cs         (K, 2) f64 on the device: c_k, s_k
 *   tables            (K, Q + 1) f64 on the device, each row non-decreasing
 *   n_knots           Q, 2 .. 65,536;  n_directions: K, 1 .. 64
 *   grad, grad_stride rows row_x (and row_y) are written for EVERY column, f64
 *   err               3 f64
 *   rank2             (K, n) int32, contiguous
 *   workspace         tfrt_transport_error_workspace_bytes(n, n_directions) bytes (0: bad arguments)
 * 11 K + 2 launches (per direction: keys, the eight of the radix sort, sorted keys, ranks; then
 * the seed and the error), nothing cleared, no atomics, no host read, no allocation: capturable.
 * Bad arguments are refused with TFRT_E_BADARG / TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_transport_error_workspace_bytes(int64_t n, int32_t n_directions);
int tfrt_transport_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                         int32_t dimension, const int32_t* mask, int32_t row_x, int32_t row_y,
                         double x0, double ix, double y0, double iy, const double* angles_cs,
                         const double* tables, int32_t n_knots, int32_t n_directions,
                         double* grad, int64_t grad_stride, double* err, int32_t* rank2,
                         void* workspace, size_t workspace_bytes, void* stream);

/* FocusError: the columns that carry the same group label, taken as LINES, must pass through one
 * common point of space -- wherever along the beam that is.  The error is the sum over the rays of
 * the squared distance of their group's FOCUS (the point nearest to all the group's lines in the
 * least-squares sense) from the ray's own line, in the scene's units.  Five launches (clear `acc`,
 * accumulate, solve, seed, finish), no host read, no allocation: captured with the rest of a step.
 *
 * `rows` is the 2d-row geometry block of a d-D trace, d = `dimension` = 2 or 3: rows 0..d-1 the
 * start s of the finished ray's last link, rows d..2d-1 its end e, converted to f64.  Every
 * operation below is an IEEE f64 operation rounded on its own (no contraction); a sum of products
 * is summed left to right, x first.
 *
 * The line of column i (the direction of tfrt_density_error_fields):
 *   v = e - s,  L = sqrt(v.v),  u = v / L;  the link is `ok` if every geometry row is finite and L
 *   is finite and > 0.
 * A column COUNTS if all of these hold (anything else has no term and gets zeros in all 2d rows of
 * `grad`; nothing is read out of bounds, whatever perm and group hold):
 *   mask is NULL or mask[i] >= 0;  the link is ok;  src = perm ? perm[i] : i lies in [0, n_source);
 *   label = group[src] lies in [0, n_groups);  lo_a <= e_a <= hi_a on every axis a of the closed
 *   box `domain`.
 * Normalisation, the constants computed once by the entry on the host:
 *   c_a = 0.5 * (lo_a + hi_a),  R = the largest of 0.5 * (hi_a - lo_a),  iR = 1.0 / R;
 *   m_a = (e_a - c_a) * iR, so |m_a| <= 1.
 * The record of a group, ten int64 {count, Pxx, Pxy, Pxz, Pyy, Pyz, Pzz, tx, ty, tz} (2-D: the z
 * slots stay 0).  With P = I - u u^T and t = P m a counting column adds, by 64-bit integer atomics
 * (the sums do not depend on the order of the atomics):
 *   1;  rint(P_ab * 2^pbits) with P_aa = 1.0 - u_a * u_a and P_ab = -(u_a * u_b), a < b;
 *   rint(t_a * 2^pbits) with w = u.m and t_a = m_a - w * u_a;  rint is half to even.
 * The focus of a group, once every column is in: n = (double) count, a_ab = ((double) Aq_ab *
 * 2^-pbits) / n, b_a = ((double) bq_a * 2^-pbits) / n, and
 *   3-D:  c00 = a11*a22 - a12*a12,  c01 = a02*a12 - a01*a22,  c02 = a01*a12 - a02*a11,
 *         c11 = a00*a22 - a02*a02,  c12 = a01*a02 - a00*a12,  c22 = a00*a11 - a01*a01,
 *         det = a00*c00 + a01*c01 + a02*c02,
 *         x_0 = (c00*b0 + c01*b1 + c02*b2) / det,  x_1 = (c01*b0 + c11*b1 + c12*b2) / det,
 *         x_2 = (c02*b0 + c12*b1 + c22*b2) / det;
 *   2-D:  det = a00*a11 - a01*a01,  x_0 = (a11*b0 - a01*b1) / det,  x_1 = (a00*b1 - a01*b0) / det.
 * The group HAS A FOCUS if count >= 2 and det >= min_det (a definition: a collimated group has
 * none); the real focus is c + R x.  A group without a focus leaves its rays without term and
 * gradient.
 * The term of a counting column whose group has a focus:
 *   q = m - x,  a = u.q,  r_b = q_b - a * u_b,  rho_b = R * r_b,  alpha = R * a;  term = rho.rho;
 *   lever = alpha / L,  grad[end_b] = (2.0 * rho_b) * (1.0 - lever),
 *   grad[start_b] = (2.0 * rho_b) * lever
 * -- the lever rule of the foot point e - alpha u along the link; exact without a derivative of x,
 * because x minimises the group's sum (up to the quantisation, relative 2^-pbits).
 * error_out = {sum of the terms, number of terms, sum / number (NaN without terms)}; the sums have
 * a fixed shape and order: two runs give the same bits.
 *
 *   rows, stride    ray block in the state dtype, 2 * dimension rows, entry (row, i) at
 *                   rows[row * stride + i], n columns
 *   group           n_source int32 labels, one per SOURCE ray
 *   perm            n int32, the source ray of column i; or NULL: column i is source ray i
 *   n_groups        G, 1 <= G <= 2^20
 *   x0 .. z1        the box, lo < hi and finite on every axis in use (z0, z1 are ignored in 2-D)
 *   pbits           1..40; the caller uses min(40, 60 - bit_length(n_source)).  n >= 2^(61 - pbits)
 *                   is refused: |t_a| < 2, so n * 2 * 2^pbits < 2^62 and no sum overflows
 *   min_det         finite and > 0
 *   grad            f64 block of 2 * dimension rows of `grad_stride`, every row written for EVERY
 *                   column
 *   acc             n_groups records of ten int64, cleared and filled by this call
 *   foci            n_groups rows of four f64 {x_0, x_1, x_2, 1.0} in NORMALISED coordinates (2-D:
 *                   x_2 = 0.0), {NaN, NaN, NaN, 0.0} for a group without a focus
 *   variant         0: a per-workgroup table in LDS up to 256 groups (ten planes of G int64,
 *                   20 KiB), global 64-bit atomics above; 1 / 2 force one of them (1 with more than
 *                   256 groups: TFRT_E_BADARG)
 *   workspace       tfrt_focus_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * 0 <= n < 2^31 (n == 0 is legal: {0, 0, NaN}), 0 <= n_source < 2^31.  Bad arguments are refused
 * with TFRT_E_BADARG / TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_focus_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_focus_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                     int32_t dimension, const int32_t* mask, const int32_t* group,
                     int64_t n_source, const int32_t* perm, int32_t n_groups, double x0, double x1,
                     double y0, double y1, double z0, double z1, int32_t pbits, double min_det,
                     double* grad, int64_t grad_stride, double* error_out, int64_t* acc,
                     double* foci, int32_t variant, void* workspace, size_t workspace_bytes,
                     void* stream);

/* DistortionError: the centroids of the groups must be a scaled (or affine) copy of the object,
 * at whatever magnification and offset the lens gives -- the distortion term of a lens merit
 * function.  Every group g has an object point p_g (`points`); a weighted least-squares fit
 * c ~ A p + t over the groups' centroids gives every group a target, and the error is the sum over
 * the rays inside of the squared distance of their GROUP'S CENTROID from its target, plus
 * tfrt_spot_error's penalty for rays outside the domain.  Four launches (clear `acc`,
 * tfrt_spot_error's unweighted accumulate launch, fit, seed), no host read, no allocation, no float
 * atomics: captured with the rest of a step.
 *
 * The columns, the fields and their codes, the four cases of a counting column in their order, the
 * out-of-domain penalty and its gradient, the records {count, Sx, Sy, 0} with `qbits` and qsx, qsy,
 * terms = k * (number of counting columns) and the chain rule of a direction field are exactly
 * tfrt_spot_error_fields'.  Every operation below is an IEEE f64 operation rounded on its own (no
 * contraction).  With one field the y component of every point and centroid is 0.0 and the same
 * expressions run.
 *
 * A group with count > 0 is USED: w = (double) count, cx = x0 + ((double) Sx / w) / qsx, cy alike,
 * (px, py) = its row of `points`.  Sums over the used groups:
 *   first pass    W = sum w,  pm = (sum w * p) / W,  cm = (sum w * c) / W          (per component)
 *   second pass   dp = p - pm, dc = c - cm;
 *                 Sxx = sum w * (dpx * dpx), Sxy = sum w * (dpx * dpy), Syy = sum w * (dpy * dpy),
 *                 Cxx = sum w * (dcx * dpx), Cxy = sum w * (dcx * dpy),
 *                 Cyx = sum w * (dcy * dpx), Cyy = sum w * (dcy * dpy)
 * The fit, with trp = Sxx + Syy:
 *   fit_kind 0, "scale" (and fit_kind 1 with one field): M = (Cxx + Cyy) / trp, A = M I (A01 = A10
 *     = 0.0); VALID iff at least two groups are used and trp > 0;
 *   fit_kind 1, "affine" (two fields): det = Sxx * Syy - Sxy * Sxy, h = trp / 2.0; VALID iff
 *     det > min_cond * (h * h) (scale-free);  A = Scp Spp^-1 by cofactors:
 *       A00 = (Cxx * Syy - Cxy * Sxy) / det,  A01 = (Cxy * Sxx - Cxx * Sxy) / det,
 *       A10 = (Cyx * Syy - Cyy * Sxy) / det,  A11 = (Cyy * Sxx - Cyx * Sxy) / det;
 *   t0 = cmx - (A00 * pmx + A01 * pmy),  t1 = cmy - (A10 * pmx + A11 * pmy)      (for reporting).
 * Third pass, for a used group with a valid fit:
 *   rx = cx - (cmx + (A00 * dpx + A01 * dpy)),  ry = cy - (cmy + (A10 * dpx + A11 * dpy));
 * without a valid fit rx = ry = 0.0; an unused group has rx = ry = NaN.
 *   error = (sum w * (rx * rx) + sum w * (ry * ry)) + the sum of the penalties.
 * A ray inside gets the gradient 2.0 * rx and 2.0 * ry of its own group (chained onto the start
 * and end rows with a direction field, as the spot seed): exact without a derivative of the fit,
 * because (A, t) minimises the error, and d c / d x_i = 1 / count (up to the quantisation of the
 * records).  Without a valid fit the rays inside add no error and get a zero gradient; the
 * penalties remain.
 * Every sum over the groups has a fixed shape and order: thread j of the one workgroup of
 * B = 1,024 threads takes the groups j, j + B, j + 2B, ... in ascending order, starting from 0.0
 * and skipping unused groups; the threads are combined within each 64-lane wave by
 * v += v[lane ^ d] for d = 32, 16, 8, 4, 2, 1, then the 16 waves in index order starting from 0.0.
 * The penalty and count partials of the accumulate launch are summed the same way, in index order.
 * Two runs give the same bits.
 *
 *   points       n_groups rows of k f64 (k = the number of fields), on the device; read by the
 *                fit launch, so overwriting it between replays of a captured step is seen
 *   fit_kind     0: scale, 1: affine
 *   min_cond     finite and >= 0
 *   fit_out      8 f64 {A00, A01, A10, A11, t0, t1, valid (1.0 / 0.0), groups used}; A and t are
 *                NaN without a valid fit
 *   residual     n_groups rows of two f64 {rx, ry}, 16-byte aligned
 *   acc          n_groups records of four int64 {count, Sx, Sy, 0}, cleared and filled by this call
 *   variant      tfrt_spot_error's
 *   workspace    tfrt_distortion_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * Everything else as for tfrt_spot_error_fields.  Bad arguments are refused with TFRT_E_BADARG /
 * TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_distortion_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_distortion_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                          int32_t dimension, const int32_t* mask, int32_t field_x,
                          int32_t field_y, const int32_t* group, int64_t n_source,
                          const int32_t* perm, int32_t n_groups, const double* points,
                          int32_t fit_kind, double min_cond, double x0, double x1, double qsx,
                          double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                          double* grad, int64_t grad_stride, double* error_out, double* fit_out,
                          double* residual, int64_t* acc, int32_t variant, void* workspace,
                          size_t workspace_bytes, void* stream);

/* CentroidError: the CENTROID of every group of rays must lie at a given target, or the centroids
 * of the groups of one parent must coincide, wherever they do -- telecentricity and prescribed
 * chief-ray angles, a prescribed image height per object point, registration (lateral colour, the
 * overlap of several beams).  It does not charge the spread of a group.  The error is the sum over
 * the rays inside of the squared distance of their GROUP'S CENTROID from its target, plus
 * tfrt_spot_error's penalty for rays outside the domain.  Four launches with `targets` (clear
 * `acc`, tfrt_spot_error's unweighted accumulate launch, table, seed), five with `parents` (clear
 * `acc` and `parent_acc` in one launch, accumulate, the parents' records, table, seed); no host
 * read, no allocation, no float atomics: captured with the rest of a step.
 *
 * The columns, the fields and their codes, the four cases of a counting column in their order, the
 * out-of-domain penalty and its gradient, the records {count, Sx, Sy, 0} with `qbits` and qsx, qsy,
 * terms = k * (number of counting columns) and the chain rule of a direction field are exactly
 * tfrt_spot_error_fields'.  Every operation below is an IEEE f64 operation rounded on its own (no
 * contraction).  With one field the y component of every centroid and target is 0.0 and the same
 * expressions run.
 *
 * A group g HAS RAYS iff count_g > 0: w_g = (double) count_g,
 *   cx_g = x0 + ((double) Sx_g / w_g) / qsx,  cy_g = y0 + ((double) Sy_g / w_g) / qsy.
 * Exactly one of `targets` and `parents` is given (TFRT_E_BADARG otherwise).
 *   targets   t_g = row g of `targets`; the group HAS A TARGET iff every entry of the row is finite
 *             (a NaN says "not pinned").
 *   parents   p = parents[g]; the group HAS A TARGET iff 0 <= p < n_parents.  The record of parent
 *             p is the INTEGER sum {count, Sx, Sy} of the records of its groups that have rays and
 *             a target (int64 atomics: integer addition is associative, any order gives the same
 *             bits; the sums are bounded by those over all n rays, which the records are sized
 *             for).  C_p is formed from the parent's record by the expression of a centroid, and
 *             t_g = C_parents[g].
 * A group is USED iff it has rays and has a target:
 *   rx = cx_g - tx_g,  ry = cy_g - ty_g,  and it adds  w_g * (rx * rx)  and  w_g * (ry * ry).
 * The residual table: {rx, ry} of a used group; {0.0, 0.0} for a group with rays that is not used;
 * {NaN, NaN} for a group without rays (no ray reads it).
 *   error = (sum w * (rx * rx) + sum w * (ry * ry)) + the sum of the penalties,
 *   error_out = {error, terms, error / terms (NaN with no counting column)}.
 * A ray inside gets the gradient 2.0 * rx and 2.0 * ry of its own group (chained onto the start
 * and end rows with a direction field, as the spot seed; all 2 d rows of every column are then
 * written); a ray outside the penalty's derivative; every other ray zeros.  That is the exact
 * gradient up to the quantisation of the records, without a derivative of a centroid: with
 * d c_g / d x_i = 1 / count_g, d/dx_i of count_g |c_g - t_g|^2 is 2 r_g; and C_p is the weighted
 * mean of its groups' centroids, which minimises sum_g count_g |c_g - C|^2, so the derivative
 * through C_p drops out.
 * Every float sum over the groups has tfrt_distortion_error's fixed shape and order: thread j of
 * the one workgroup of B = 1,024 threads takes the groups j, j + B, j + 2B, ... in ascending order,
 * starting from 0.0 and skipping groups that are not used; the threads are combined within each
 * 64-lane wave by v += v[lane ^ d] for d = 32, 16, 8, 4, 2, 1, then the 16 waves in index order
 * starting from 0.0.  The penalty and count partials of the accumulate launch are summed the same
 * way, in index order.  Two runs give the same bits.
 *
 *   targets      n_groups rows of k f64 (k = the number of fields), on the device, or NULL; read
 *                by the table launch, so overwriting it between replays of a captured step is seen
 *   parents      n_groups int32 on the device, or NULL; read by the launches, overwritable alike
 *   n_parents    1 .. 2^20 with `parents` (ignored with `targets`)
 *   parent_acc   n_parents records of four int64 {count, Sx, Sy, 0}, cleared and filled by this
 *                call; required with `parents` (ignored with `targets`)
 *   used_out     2 f64 {groups used, parents with rays (0.0 with `targets`)}
 *   residual     n_groups rows of two f64 {rx, ry}, 16-byte aligned
 *   acc          n_groups records of four int64 {count, Sx, Sy, 0}, cleared and filled by this call
 *   variant      tfrt_spot_error's
 *   workspace    tfrt_centroid_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * Everything else as for tfrt_spot_error_fields.  Bad arguments are refused with TFRT_E_BADARG /
 * TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_centroid_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_centroid_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                        int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                        const int32_t* group, int64_t n_source, const int32_t* perm,
                        int32_t n_groups, const double* targets, const int32_t* parents,
                        int32_t n_parents, int64_t* parent_acc, double x0, double x1, double qsx,
                        double y0, double y1, double qsy, int32_t qbits, double oob_weight,
                        double* grad, int64_t grad_stride, double* error_out, double* used_out,
                        double* residual, int64_t* acc, int32_t variant, void* workspace,
                        size_t workspace_bytes, void* stream);

/* MomentError: the COVARIANCE of every group of rays -- the size and the shape of its spot -- must
 * be a given matrix (mode 0, `covariance`), or must be round at whatever size (mode 1): a spot of
 * a prescribed width, an anamorphic spot, the astigmatism term of an imaging merit function, a
 * beam matrix in phase space.  The error is the sum over the used groups of n |D|_F^2 with D the
 * residual of the group's covariance, plus tfrt_spot_error's penalty for rays outside the domain.
 * Six launches (clear `acc` and `mom`, tfrt_spot_error's unweighted accumulate launch, the centres,
 * pass 2, table, seed); no host read, no allocation, no float atomics: captured with the rest of a
 * step.
 *
 * The columns, the fields and their codes, the four cases of a counting column in their order, the
 * out-of-domain penalty and its gradient, terms = k * (number of counting columns) and the chain
 * rule of a direction field are exactly tfrt_spot_error_fields'.  Every operation below is an IEEE
 * f64 operation rounded on its own (no contraction); integers are exact.  With one field every xy
 * and yy component and cy are 0.0.
 *
 * Grid.  `mbits` is even, 2 .. 40 (ops.moment_mbits(N) = min(40, 2 * ((61 - bit_length(N)) / 2))
 * for a source of N rays), h = mbits / 2, msx = 2^mbits / (x1 - x0) and msy alike, computed once
 * by the caller; n < 2^(61 - mbits).  A ray inside has
 *   mx = min(max(rint((x - x0) * msx), 0), 2^mbits)   (tfrt_spot_error's fixed point on this grid).
 * Pass 1.  {1, mx, my} is added to the record {n, Sx, Sy, 0} of the ray's group in `acc`.
 * Centre.  A group is USED iff n >= 2.  kx = (2 Sx + n) / (2 n) (integer division), ky alike;
 *   cx = x0 + (double) kx / msx,  cy = y0 + (double) ky / msy   (also formed for n = 1).
 * Pass 2.  A ray inside a used group: dx = mx - kx, dxl = dx & (2^h - 1), dxh = dx >> h (arithmetic),
 * dy alike; for (a, b) = (x, x), (x, y), (y, y) the group's record in `mom` -- nine int64
 * {xxHH, xxHL, xxLL, xyHH, xyHL, xyLL, yyHH, yyHL, yyLL} -- receives
 *   HH += ah * bh,  HL += ah * bl + al * bh,  LL += al * bl.
 * |dx| <= 2^mbits, so a term is at most 2^(mbits + 1) in magnitude and a sum stays below 2^62.
 * HH 2^mbits + HL 2^h + LL is the exact integer sum(da * db).
 * Covariance.  Mf = (ldexp((double) HH, mbits) + ldexp((double) HL, h)) + (double) LL,
 *   C_ab = (Mf_ab / (double) n) / (ms_a * ms_b):
 * the second moment about the centre in scene units squared (the centre lies within half a grid
 * step of the centroid; the (c - k)^2 correction is dropped by definition).
 * Residual.  mode 0: t = row g of `covariance`, {txx, txy, tyy} (one field: {txx});
 *   D_ab = C_ab - t_ab, or 0.0 where t_ab is NaN (a free component).
 * mode 1 (two fields):  s = (Cxx + Cyy) / 2.0,  Dxx = Cxx - s,  Dxy = Cxy,  Dyy = Cyy - s.
 * Error.  e_g = n * ((Dxx * Dxx + 2.0 * (Dxy * Dxy)) + Dyy * Dyy),
 *   error = (sum of e_g over the used groups) + the sum of the penalties,
 *   error_out = {error, terms, error / terms (NaN with no counting column)}.
 * The sum over the groups has tfrt_centroid_error's fixed shape and order, the partials of the
 * accumulate launch likewise.  Two runs give the same bits.
 * Gradient.  With F = 4.0 * D (exact), a ray inside a used group gets
 *   gx = Fxx * (x - cx) + Fxy * (y - cy),  gy = Fxy * (x - cx) + Fyy * (y - cy)
 * (one field: gx = Fxx * (x - cx)) from its own f64 coordinates, chained onto the start and end
 * rows with a direction field; a ray outside the penalty's derivative; every other ray zeros.
 * That is the gradient of the error without a derivative of the centre (the residuals of a group
 * sum to zero) or of s (which minimises the error), up to the grid.
 *
 *   mode         0: target covariance; 1: round
 *   covariance   mode 0: n_groups rows of 3 f64 (one field: of 1) on the device, read by the table
 *                launch, so overwriting it between replays of a captured step is seen; mode 1: NULL
 *   used_out     2 f64 {groups used, groups with rays}
 *   group_rows   n_groups rows of eight f64 {cx, cy, Fxx, Fxy, Fyy, used (1.0 / 0.0), 0, 0},
 *                16-byte aligned; c is NaN for a group without rays, F is 0.0 for one not used
 *   cov_out      n_groups rows of six f64 {Cxx, Cxy, Cyy, Dxx, Dxy, Dyy}, NaN for a group not used
 *   acc          n_groups records of four int64, mom: n_groups records of nine int64; both cleared
 *                and filled by this call
 *   variant      0: by n_groups; 1: the tables of both passes in LDS (up to 256 groups); 2: global
 *                atomics
 *   workspace    tfrt_moment_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * Everything else as for tfrt_spot_error_fields.  Bad arguments are refused with TFRT_E_BADARG /
 * TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_moment_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_moment_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                      int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                      const int32_t* group, int64_t n_source, const int32_t* perm,
                      int32_t n_groups, int32_t mode, const double* covariance, double x0,
                      double x1, double msx, double y0, double y1, double msy, int32_t mbits,
                      double oob_weight, double* grad, int64_t grad_stride, double* error_out,
                      double* used_out, double* group_rows, double* cov_out, int64_t* acc,
                      int64_t* mom, int32_t variant, void* workspace, size_t workspace_bytes,
                      void* stream);

/* MixingError: every group of rays must land with the SAME density on the target, whatever that
 * density is (the dies of an LED behind a mixing rod, the input zones of a homogeniser, the beams
 * of a combiner).  The error is the mass-weighted mean over the groups of the mean squared
 * difference of the group's density from the pooled one, in units of the uniform density, plus
 * tfrt_density_error's penalty for rays outside the domain.  Six launches (clear `hq`, splat,
 * margins, pulls, finish, seed); no host read, no allocation, no float atomics: captured with the
 * rest of a step.
 *
 * The columns, the fields and their codes, the domain constants sx = nx / (x1 - x0) and sy, the
 * bilinear splat with its clamped indices, the out-of-domain penalty and its gradient and the
 * chain rule of a direction field are exactly tfrt_density_error_fields'; with `weight` the
 * weight w of a column's source ray and every place it enters are tfrt_density_error_weighted's.
 * Column i is source ray s = perm[i] (perm NULL: i).  Every operation below is an IEEE f64
 * operation rounded on its own (no contraction); integers are exact.
 *
 * Classification.  tfrt_density_error's (weighted: tfrt_density_error_weighted's), then: a column
 * that counts without a source ray (s outside [0, n_source)) or whose label group[s] lies outside
 * [0, G) does not count -- no error, zero gradient, no penalty.  A column outside the closed domain
 * adds oob_weight * (ex^2 + ey^2) (times w last) and gets the derivative of that.
 * Histogram.  A column inside adds rint(b * 2^32) (weighted: rint((b * w) * 2^32), half to even)
 * for each of its two or four bilinear weights b to the cell of its bin in plane group[s] of the
 * int64 table Hq[G][ny][nx].
 * Margins (integer sums, free of order; no overflow for n < 2^31).  With B = nx * ny:
 *   nq_g = sum_b Hq_gb,  Pq_b = sum_g Hq_gb,  Nq = sum_g nq_g.
 * Error.  A group is USED iff nq_g > 0.  For a cell of a used group
 *   p = (double) Hq_gb / (double) nq_g,  m = (double) Pq_b / (double) Nq,  d = p - m,
 *   e_g = (double) B * sum_b (d * d),   E_mix = sum over the used groups of
 *   ((double) nq_g / (double) Nq) * e_g,   error = E_mix + the sum of the penalties,
 *   error_out = {error, 1, error}  (ONE error term, as tfrt_density_error).
 * Nq == 0: E_mix = 0.0 and every pull is 0.0.
 * Pull.  N = (double) Nq * 2^-32,  D_gb = ((2.0 * (double) B) / N) * d; 0.0 in a group not used.
 * Gradient.  A column inside gets tfrt_density_error's expressions on plane group[s] of D,
 *   gx = sx * ((1 - ty) * (D[j0][i1] - D[j0][i0]) + ty * (D[j1][i1] - D[j1][i0])),
 *   gy = sy * ((1 - tx) * (D[j1][i0] - D[j0][i0]) + tx * (D[j1][i1] - D[j0][i1]))
 * (one field: gx = sx * (D[i1] - D[i0])), times w last, chained onto the start and end rows with a
 * direction field.  That is the gradient of the error without a derivative of m, nq_g or Nq: m is
 * the mass-weighted mean of the p_g and so minimises the error, and a column inside carries total
 * weight 1 (w) wherever it stands.
 * Orders.  Thread t of 1,024 adds the d * d of the bins t, t + 1024, ... of its group in ascending
 * order onto 0.0; within each wave of 64 threads v[lane] += v[lane ^ s] for s = 32 .. 1; then the
 * 16 waves in index order onto 0.0.  The sum over the groups has the same shape with the groups in
 * the bins' place (tfrt_centroid_error's), the penalties that of tfrt_centroid_error's: two runs
 * give the same bits.
 *
 *   group        n_source int32 labels of the SOURCE rays; n_groups = G, 1 .. 1,024;
 *                G * nx * ny <= 2^20, nx * ny <= 65,536
 *   weight       NULL, or n_source f64 in [0, 1] (a column whose weight is not in [0, 1] does not
 *                count)
 *   used_out     2 f64 {groups used, N}
 *   group_errors G f64: e_g, NaN for a group not used
 *   pull         G * ny * nx f64: D
 *   hq           G * ny * nx int64, cleared and filled by this call
 *   variant      0: by the number of cells; 1: the table in LDS (G * nx * ny <= 4,096); 2: global
 *                atomics
 *   workspace    tfrt_mixing_error_workspace_bytes(n, n_groups, nx, ny) bytes (0: bad arguments)
 * Rows of `grad` other than those named are not written.  Bad arguments are refused with
 * TFRT_E_BADARG / TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_mixing_error_workspace_bytes(int64_t n, int32_t n_groups, int32_t nx, int32_t ny);
int tfrt_mixing_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                      int32_t dimension, const int32_t* mask, int32_t field_x, int32_t field_y,
                      const int32_t* group, int64_t n_source, const int32_t* perm,
                      int32_t n_groups, const double* weight, int32_t nx, int32_t ny, double x0,
                      double x1, double sx, double y0, double y1, double sy, double oob_weight,
                      double* grad, int64_t grad_stride, double* error_out, double* used_out,
                      double* group_errors, double* pull, int64_t* hq, int32_t variant,
                      void* workspace, size_t workspace_bytes, void* stream);

/* FlatFieldError: the foci of all groups must lie in ONE plane with the unit normal a = `axis` --
 * wherever along the normal that plane has to stand.  The error is the sum, over the counting rays
 * of the groups with a focus, of the squared distance of their group's focus from that plane, in
 * the scene's units.  Four launches (clear `acc`, tfrt_focus_error's accumulate launch, fit, seed),
 * no host read, no allocation, no float atomics, no finishing launch: captured with the rest of a
 * step.
 *
 * Everything up to a group's focus is exactly tfrt_focus_error's: the columns and which of them
 * COUNT, the box constants c, R, iR, m = (e - c) * iR, `pbits`, the ten-slot int64 records, a and
 * b, the cofactors c00 .. c22 and det, "has a focus iff count >= 2 and det >= min_det", and
 * x = A^-1 b.  Every operation below is an IEEE f64 operation rounded on its own (no contraction);
 * a sum of products is summed left to right, x first; in 2-D the third component of every vector
 * is 0.0 and is left out of the sums.
 *
 * A group is USED iff it has a focus.  With the same cofactors, y = A^-1 a:
 *   3-D:  y_0 = (c00*a_0 + c01*a_1 + c02*a_2) / det,  y_1 = (c01*a_0 + c11*a_1 + c12*a_2) / det,
 *         y_2 = (c02*a_0 + c12*a_1 + c22*a_2) / det;
 *   2-D:  y_0 = (a11*a_0 - a01*a_1) / det,  y_1 = (a00*a_1 - a01*a_0) / det
 * (a_0, a_1, a_2 the axis; a00 .. a22 the group's matrix), and
 *   n = (double) count,  h = a.x.
 * First pass, over the used groups:
 *   W = sum n,  S = sum n * h,  the number of used groups,  terms = sum count (an integer);
 *   hbar = S / W;  the plane is VALID iff at least two groups are used.
 * Second pass, for a used group under a valid plane:
 *   r = h - hbar,  s = R * r,  e_g = s * s,  mu_b = (2.0 * s) * y_b   (2-D: mu_2 = 0.0);
 *   inside = sum n * e_g.
 * Without a valid plane e_g = 0.0, mu = 0.0 and inside = 0.0.
 *   error_out = {inside, (double) terms, inside / terms (NaN with terms == 0)}.
 * The plane is a.p = a.c + R * hbar in the scene's coordinates; hbar is not differentiated, because
 * it minimises the sum (sum n * r = 0).  The focus IS differentiated: d error / d x_g = 2 R^2 n r a
 * and d x_g = A_g^-1 (1 / n) sum_i d[P_i (m_i - x_g)], so mu = 2 R r A^-1 a is the group's adjoint
 * in the scene's units (n cancels).
 * A counting column of a used group under a valid plane, against x and mu of its group:
 *   q = m - x,  alpha = u.q,  lever = (R * alpha) / L,  rest = 1.0 - lever,
 *   beta = mu.u,  k = beta / L,  and per component b:
 *   rho_b = R * (q_b - alpha * u_b),  muP_b = mu_b - beta * u_b,  turn_b = k * rho_b,
 *   grad[end_b] = muP_b * rest - turn_b,  grad[start_b] = muP_b * lever + turn_b
 * -- the lever rule applied to the part of the adjoint across the ray, plus a term from turning the
 * ray.  Every other column gets 0.0 in all 2d rows.
 * Every sum over the groups has a fixed shape and order: thread j of the one workgroup of
 * B = 1,024 threads takes the groups j, j + B, j + 2B, ... in ascending order, starting from 0.0
 * and skipping unused groups; the threads are combined within each 64-lane wave by
 * v += v[lane ^ d] for d = 32, 16, 8, 4, 2, 1, then the 16 waves in index order starting from 0.0
 * (tfrt_distortion_error's convention).  Two runs give the same bits.
 *
 *   ax, ay, az      the unit normal: finite, |ax*ax + ay*ay + az*az - 1| <= 8 * 2^-52 (the caller
 *                   divides its axis by sqrt(axis.axis) once); az is ignored in 2-D
 *   table           n_groups rows of eight f64, 64-byte aligned: {x_0, x_1, x_2, used (1.0 / 0.0),
 *                   mu_0, mu_1, mu_2, e_g}; x in NORMALISED coordinates (2-D: x_2 = 0.0);
 *                   {NaN, NaN, NaN, 0, 0, 0, 0, 0} for an unused group
 *   fit_out         8 f64 {hbar (NaN without a used group), a.c + R * hbar, W, groups used,
 *                   valid (1.0 / 0.0), 0, 0, 0}
 *   acc             n_groups records of ten int64, cleared and filled by this call
 *   workspace       tfrt_flatfield_error_workspace_bytes(n, n_groups) bytes (0: bad arguments)
 * Everything else as for tfrt_focus_error.  Bad arguments are refused with TFRT_E_BADARG /
 * TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_flatfield_error_workspace_bytes(int64_t n, int32_t n_groups);
int tfrt_flatfield_error(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                         int32_t dimension, const int32_t* mask, const int32_t* group,
                         int64_t n_source, const int32_t* perm, int32_t n_groups, double x0,
                         double x1, double y0, double y1, double z0, double z1, int32_t pbits,
                         double min_det, double ax, double ay, double az, double* grad,
                         int64_t grad_stride, double* error_out, int64_t* acc, double* table,
                         double* fit_out, int32_t variant, void* workspace,
                         size_t workspace_bytes, void* stream);

/* GoalError on the fixed-shape columns of an in-place trace (tfrt_scene3d.in_place == 2: the
 * finished rows at the rays' own columns, a mask in the place of a ray count) -- the form that can
 * be added to a coupled error of the same step (tfrt_error_combine).  Two launches (the columns,
 * the sum), no host read, no allocation, no atomics: captured with the rest of a step.
 *
 * A column i COUNTS if mask is NULL or mask[i] >= 0, and its source ray s = perm ? perm[i] : i lies
 * inside [0, n_source); a column whose s lies outside does not count and nothing is read out of
 * bounds, whatever perm holds.  For a counting column and each field c, every operation an IEEE
 * f64 operation rounded on its own (no contraction):
 *   o = (double) rows[fields[c]][i],  d = o - goal(c, s),  the error term is d * d,
 *   grad[fields[c]][i] = 2 * d
 * with goal(c, s) = goal[c * goal_stride + s * goal_ray_stride] (both layouts of
 * tfrt_goal_error3d).  The rows named by `fields` are written for EVERY column, 0.0 where a column
 * does not count; no other row is written.
 *   error_out = {sum, terms, terms > 0 ? sum / terms : NaN},  terms = n_fields * counting columns.
 * The sum has a fixed shape and order -- per lane over its columns (grid-stride), a fixed-shape
 * workgroup sum, then one workgroup over the workgroups' partial sums in index order --: two runs
 * give the same bits.
 *
 *   rows, stride, n   the ray block in the state dtype (TFRT_F32 / TFRT_F64 / TFRT_F16), entry
 *                     (row, i) at rows[row * stride + i]; 0 <= n < 2^31 (n == 0 is legal:
 *                     {0, 0, NaN})
 *   n_rows            4 or 6: the rows of the block (2-D / 3-D geometry)
 *   mask              n int32 or NULL (tfrt_ray_out.face of the in-place trace)
 *   perm, n_source    n int32, the source ray of column i, or NULL: column i is source ray i;
 *                     0 <= n_source < 2^31, as for tfrt_spot_error
 *   fields, n_fields  1 .. n_rows distinct rows in [0, n_rows), passed as tfrt_goal_error3d
 *                     passes them
 *   goal              f64 table with one entry per field and SOURCE ray
 *   grad, grad_stride f64 block, entry (row, i) at grad[row * grad_stride + i]
 *   workspace         tfrt_goal_error_columns_workspace_bytes(n) bytes (0: bad arguments)
 * Bad arguments are refused with TFRT_E_BADARG / TFRT_E_WORKSPACE before any launch.
 */
size_t tfrt_goal_error_columns_workspace_bytes(int64_t n);
int tfrt_goal_error_columns(const void* rows, int64_t stride, int64_t n, int32_t state_dtype,
                            int32_t n_rows, const int32_t* mask, const int32_t* perm,
                            int64_t n_source, const int32_t* fields, int32_t n_fields,
                            const double* goal, int64_t goal_stride, int64_t goal_ray_stride,
                            double* grad, int64_t grad_stride, double* error_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* SumError: the weighted sum of K error terms of one step, 1 <= K <= 8, in ONE launch.  Every term
 * has left a gradient seed block on the same columns and its error triple on the device; the
 * reverse sweep is linear in its seed, so the combined seed block and the combined error are all
 * a step of the sum needs.  The descriptors are a host array copied into the kernel arguments.
 *
 *   c_k = weights[k]                                          reduce == 0 (sum)
 *   c_k = terms_k > 0 ? weights[k] / terms_k : 0.0            reduce == 1 (mean),
 * terms_k = terms[k].error[1] read on the device: no ray count ever reaches the host.
 * Gradients, for every row r < n_rows and column i < n: the terms whose row_mask has bit r, in
 * index order, acc = c_k * g_k[r][i] for the first, acc = acc + c_k * g_k[r][i] for every later
 * one, every product and every sum rounded on its own; a row named by no term is written 0.0.
 * The first product is not added to a zero: one term with weight 1.0 comes back with its own
 * bits, signed zeros included.
 * Error: E = c_0 * e_0[0], then E = E + c_k * e_k[0] in index order; error_out = {E, 1, E} -- one
 * error term, as tfrt_density_error reports itself.  coeff_out[k] = c_k.  One thread of the
 * launch writes error_out and coeff_out; they depend only on what earlier launches wrote.
 *
 *   terms[k].grad      f64 block, entry (row, i) at grad[row * stride + i]; NULL in EVERY term (or
 *                      n == 0): only the errors are combined -- the step without a reverse sweep
 *   terms[k].stride    n <= stride < 2^31
 *   terms[k].row_mask  bit r: the term has written row r of its block (no bit at n_rows or above)
 *   terms[k].error     the term's 3 f64 {sum, terms, mean} on the device
 *   weights            n_terms f64 on the device; reduce: 0 = sum, 1 = mean
 *   n, n_rows          0 <= n < 2^31 columns, 4 or 6 rows
 *   grad_out           f64 block of n_rows rows of out_stride; it must not overlap a term's block
 *                      (n_rows rows of its stride): TFRT_E_BADARG
 *   error_out          3 f64;  coeff_out: n_terms f64
 * A lane takes two neighbouring columns with one 16-byte access per term and row where every
 * block is 16-byte aligned and every stride even, one column otherwise; the bits do not depend on
 * which.  (sum_k rows_k + n_rows) * 8 B * n of traffic, no LDS, no atomics, no host read.
 */
typedef struct tfrt_combine_term {
  const double* grad;
  int64_t stride;
  uint32_t row_mask;
  const double* error;
} tfrt_combine_term;
int tfrt_error_combine(const tfrt_combine_term* terms, int32_t n_terms, const double* weights,
                       int32_t reduce, int64_t n, int32_t n_rows, double* grad_out,
                       int64_t out_stride, double* error_out, double* coeff_out, void* stream);

/* tfrt_goal_error3d_deferred and tfrt_trace3d_backward in ONE launch, for a trace over coherent
 * rays (tfrt_scene3d.coherent_rays, not deterministic, max_passes <= 8; TFRT_E_UNSUPPORTED
 * otherwise -- call the two entry points instead): the lane that walks a finished ray's chain of
 * slots back forms that ray's residuals itself -- output row minus goal row, the output as stored
 * in `finished` (state dtype) -- seeds the walk with 2 (output - goal) and leaves the squared
 * residuals in per-wavefront partial sums (a fixed order: the error is bit-identical from run to
 * run).  No seed block is written and read back, one dependent launch less per step.
 *   finished        the finished-ray block tfrt_trace3d_forward wrote (rays + capacity; ids unused:
 *                   a chain knows its source ray)
 *   fields, goal    as for tfrt_goal_error3d; goal rows are indexed by the source ray in the
 *                   trace's order
 *   goal_workspace  tfrt_trace3d_backward_goal_workspace_bytes(n_rays) bytes (the partial sums)
 *   pending         filled in like tfrt_goal_error3d_deferred's: finish with
 *                   tfrt_sgd_process_multi_finish or tfrt_goal_finish
 *   grad_face_verts (M,9) f64, ACCUMULATED into (cleared beforehand: tfrt_scene3d.clear_buffer);
 *                   the four sums with tfrt_scene3d.face_sums, as for tfrt_trace3d_backward
 * Everything else as for tfrt_trace3d_backward (grad_active / grad_stopped / grad_dead may be
 * given as well; the finished rows' gradient is the goal's). */
size_t tfrt_trace3d_backward_goal_workspace_bytes(int64_t n_rays);
int tfrt_trace3d_backward_goal(const void* src_rays, int64_t src_stride, int64_t n_rays,
                               const tfrt_scene3d* scene, double new_ray_length,
                               double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                               const tfrt_ray_out* finished, const int32_t* fields,
                               int32_t n_fields, const double* goal, int64_t goal_stride,
                               int64_t goal_ray_stride, double* error_out, int64_t* tests_total,
                               void* goal_workspace, size_t goal_workspace_bytes,
                               tfrt_goal_pending* pending, const double* grad_active,
                               int64_t cap_active, const double* grad_stopped,
                               int64_t cap_stopped, const double* grad_dead, int64_t cap_dead,
                               double* grad_face_verts, double* grad_src_rays,
                               const int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Benchmark instrumentation (the only global state in the library; not used by the product
 * path).  While enabled, the launches of the hot kernels made by tfrt_trace3d_forward /
 * tfrt_trace3d_backward / tfrt_intersect3d are bracketed by HIP event pairs recorded on the
 * launch stream, one record per pass and kind:
 *   TFRT_PROF_INTERSECT   the pass's intersect launch(es): k_intersect_beam + k_intersect_group,
 *                         or k_intersect_group, or k_intersect3d
 *   TFRT_PROF_REACT       k_react3d
 *   TFRT_PROF_BACKWARD    k_backward3d (one per pass, last pass first)
 *   TFRT_PROF_ACCUMULATE  k_face_accumulate (one per reverse sweep)
 * tfrt_profile_read_kind synchronises the events of one kind and writes the elapsed
 * milliseconds, in launch order, into ms[0..max_records); it returns the record count (or a
 * negative error).  tfrt_profile_read = the intersect records.  tfrt_profile_enable(0|1) also
 * clears the records. */
#define TFRT_PROF_INTERSECT 0
#define TFRT_PROF_REACT 1
#define TFRT_PROF_BACKWARD 2
#define TFRT_PROF_ACCUMULATE 3
int tfrt_profile_enable(int enable);
int tfrt_profile_read(float* ms, int32_t max_records);
int tfrt_profile_read_kind(int32_t kind, float* ms, int32_t max_records);

/* ------------------------------------------------------------------------------------------
 * Seam-level single kernels (same math, no pass loop).
 */

/* OpticalSystem3D._intersection, tfrt/engine.py:1103-1166: nearest valid triangle per ray.
 * Outputs are (n_rays) arrays: x,y,z,ray_u,trig_u,trig_v f64; valid u8; gather_trig i32
 * (0 where invalid, like tf.argmin over an all-sentinel column). */
size_t tfrt_intersect3d_workspace_bytes(int64_t n_rays, int64_t n_faces);
int tfrt_intersect3d(const void* rays, int64_t stride, int64_t n_rays, int32_t state_dtype,
                     const double* face_verts, int64_t n_faces, double intersect_epsilion,
                     double size_epsilion, double ray_start_epsilion, double* x, double* y,
                     double* z, uint8_t* valid, double* ray_u, double* trig_u, double* trig_v,
                     int32_t* gather_trig, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * The public pairwise functions of tfrt/geometry.py (dense outputs, forward only).
 *
 * Outputs are row-major (n_rows, n_cols) grids, f64 (valid: u8).  Every operand array of a
 * set is read as p[col * col_stride + row * row_stride]:
 *   - tf.meshgrid forms (line_intersect, geometry.py:27-78; line_triangle_intersect, :191-251;
 *     line_circle_intersect, :338-402): first set (n_cols values) strides (1, 0), second set
 *     (n_rows values) strides (0, 1) -- the meshgrid copies of the reference are never made;
 *   - element-wise "raw" forms (raw_line_intersect, :96-167; raw_line_triangle_intersect,
 *     :275-320; raw_line_circle_intersect, :420-547): n_rows = 1, both sets strides (1, 0).
 * Same operation order and "safe value" masking as the reference: invalid elements hold the
 * reference's placeholder results (u = v = 1, ...), never NaN from a zero denominator.
 */
/* first = {x1s,y1s,x1e,y1e}, second = {x2s,y2s,x2e,y2e}; u: parameter on the first line, v: on
 * the second; valid = |denominator| >= epsilion. */
int tfrt_line_intersect(int64_t n_cols, int64_t n_rows, const double* const first[4],
                        int64_t first_col_stride, int64_t first_row_stride,
                        const double* const second[4], int64_t second_col_stride,
                        int64_t second_row_stride, double epsilion, double* x, double* y,
                        uint8_t* valid, double* u, double* v, void* stream);

/* rays = {rx1,ry1,rz1,rx2,ry2,rz2}, triangles = {xp,yp,zp,x1,y1,z1,x2,y2,z2} (pivot, first,
 * second vertex).  No range tests on ray_u / trig_u / trig_v (engine.py:1138-1141 does those). */
int tfrt_line_triangle_intersect(int64_t n_cols, int64_t n_rows, const double* const rays[6],
                                 int64_t ray_col_stride, int64_t ray_row_stride,
                                 const double* const triangles[9], int64_t tri_col_stride,
                                 int64_t tri_row_stride, double epsilion, double* x, double* y,
                                 double* z, uint8_t* valid, double* ray_u, double* trig_u,
                                 double* trig_v, void* stream);

/* lines = {xs,ys,xe,ye}, circles = {xc,yc,r}; plus / minus = {x,y,u,v} of the two roots of the
 * quadratic (v = angle of the hit on the circle), *_valid = root exists. */
int tfrt_line_circle_intersect(int64_t n_cols, int64_t n_rows, const double* const lines[4],
                               int64_t line_col_stride, int64_t line_row_stride,
                               const double* const circles[3], int64_t circle_col_stride,
                               int64_t circle_row_stride, double epsilion, double* const plus[4],
                               uint8_t* plus_valid, double* const minus[4], uint8_t* minus_valid,
                               void* stream);

/* geometry.snells_law_3D, tfrt/geometry.py:671-753.  All arrays (n) f64; norm is (n,3).
 * Writes the new ray (start = old end). */
int tfrt_snell3d(int64_t n, const double* x_start, const double* y_start, const double* z_start,
                 const double* x_end, const double* y_end, const double* z_end,
                 const double* norm, const double* n_in, const double* n_out,
                 double new_ray_length, double* out6 /* 6 x n */, void* stream);

/* geometry.snells_law_2D, tfrt/geometry.py:565-653.  out4 = 4 x n (xs,ys,xe,ye). */
int tfrt_snell2d(int64_t n, const double* x_start, const double* y_start, const double* x_end,
                 const double* y_end, const double* norm, const double* n_in,
                 const double* n_out, double new_ray_length, double* out4, void* stream);

/* Arithmetic self-test (no reference counterpart): out[i] = a[i] / b[i], sqrt(a[i]),
 * 1.0 / sqrt(a[i]) or a[i] + b[i] * b[i] (product and sum rounded separately), evaluated on the
 * device with the library's own compile flags.  The decisions of the trace (valid masks, nearest
 * hit, ties) equal the reference's eager float64 TensorFlow ops only if these are correctly
 * rounded; tests compare them with the host's IEEE results bit for bit. */
#define TFRT_SELFTEST_DIV 0
#define TFRT_SELFTEST_SQRT 1
#define TFRT_SELFTEST_RSQRT 2
#define TFRT_SELFTEST_MULADD 3
/* the reverse sweep's own reciprocal and reciprocal square root (hardware estimate + two Newton
 * steps, csrc/trace_math.h adj_rcp / adj_rsqrt; `b` unused): not correctly rounded by design --
 * the test bounds their error against the host's IEEE results */
#define TFRT_SELFTEST_ADJ_RCP 4
#define TFRT_SELFTEST_ADJ_RSQRT 5
int tfrt_selftest_f64(int op, int64_t n, const double* a, const double* b, double* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * 2-D: segments + arcs (OpticalSystem2D, tfrt/engine.py:254-866).
 */
typedef struct tfrt_scene2d {
  const double* seg;         /* (Ms,4) f64: x_start,y_start,x_end,y_end */
  const int32_t* seg_cat;    /* (Ms) */
  const int32_t* seg_mat_in; /* (Ms) or NULL */
  const int32_t* seg_mat_out;
  const double* seg_n_in;    /* (Ms) or NULL ("value" mode) */
  const double* seg_n_out;
  int64_t n_segments;
  const double* arc;         /* (Ma,5) f64: x_center,y_center,angle_start,angle_end,radius */
  const int32_t* arc_cat;
  const int32_t* arc_mat_in;
  const int32_t* arc_mat_out;
  const double* arc_n_in;
  const double* arc_n_out;
  int64_t n_arcs;
  const double* n_table;
  int64_t n_table_stride;
  int32_t n_materials;
  double intersect_epsilion, size_epsilion, ray_start_epsilion;
  /* Reverse sweep only.  0 (default, the reference): the gradient of a totally reflected ray
   * is NaN -- geometry.py:640-646 evaluates asin(theta2) with |theta2| > 1 in the unselected
   * branch of tf.where, and 0 * (d asin) = NaN flows into every boundary entry the ray touched
   * up to the reflecting one; tfrt_sgd_process zeroes such entries (optimizer.py:226-229).
   * 1: the reflect branch's own finite gradient (new_angle = norm + theta1 + pi) instead. */
  int32_t finite_tir_gradient;
  /* Bit-reproducible reverse sweeps: `deterministic`, the struct's last field (appended there to
   * keep every other offset); the entries this rule makes NaN are NaN in both of its modes. */
  /* Reverse sweeps only (tfrt_trace2d_backward, tfrt_trace2d_backward_goal,
   * tfrt_trace2d_backward_rows), "value" mode (n_table NULL, *_n_in / *_n_out given): f64,
   * ACCUMULATED into, or NULL (not asked) -- d error / d seg_n_in[k], seg_n_out[k] (Ms each) and
   * d error / d arc_n_in[k], arc_n_out[k] (Ma each), the 2-D counterpart of
   * tfrt_scene3d.grad_n_in / grad_n_out (tfrt/operation.py:255-307 reads the two fields as
   * ordinary tensors).  An index that is 0 (the "safe" ratio replaced it by 1) gets 0.  Ignored in
   * "index" mode and by tfrt_trace2d_forward. */
  double* grad_seg_n_in;
  double* grad_seg_n_out;
  double* grad_arc_n_in;
  double* grad_arc_n_out;
  /* Reverse sweeps only (tfrt_trace2d_backward, tfrt_trace2d_backward_goal,
   * tfrt_trace2d_backward_rows), the 2-D counterpart of tfrt_scene3d.deterministic.  0 (default):
   * grad_seg, grad_arc and the four grad_*_n_* blocks are summed with float64 atomics, whose last
   * bits depend on the order in which they arrive.  1: ordered mode -- the sweep runs twice; the
   * first run finds every output entry's largest finite term, the second rounds each term to a
   * 64-bit integer at a power-of-two scale taken from that maximum (2^-40 of it while an entry
   * receives at most 2^22 terms -- rays x passes of the call, per pass for tfrt_trace2d_backward --
   * one bit coarser per doubling beyond, so that no sum can overflow), sums the integers (exact,
   * hence order-independent) and adds sum / scale into the output: bit-identical results on every
   * run and for any order of the source rays.  A non-finite term makes its entry NaN, as its float
   * sum would be (the TIR rule of finite_tir_gradient is unchanged).  The forward pass and the
   * built-in goal's error sum are bit-reproducible in either mode.  Needs the workspace
   * tfrt_trace2d_workspace_bytes reports for the scene's n_segments and n_arcs. */
  int32_t deterministic;
} tfrt_scene2d;

/* OpticalSystem2D._segment_intersection, tfrt/engine.py:688-749 (rays: 4 x stride block). */
int tfrt_segment_intersection(const void* rays, int64_t stride, int64_t n_rays,
                              int32_t state_dtype, const double* seg, int64_t n_segments,
                              double intersect_epsilion, double size_epsilion,
                              double ray_start_epsilion, double* x, double* y, uint8_t* valid,
                              double* ray_u, double* seg_u, int32_t* gather_segment,
                              void* stream);

/* OpticalSystem2D._arc_intersection, tfrt/engine.py:768-866. */
int tfrt_arc_intersection(const void* rays, int64_t stride, int64_t n_rays, int32_t state_dtype,
                          const double* arc, int64_t n_arcs, double intersect_epsilion,
                          double size_epsilion, double ray_start_epsilion, double* x, double* y,
                          uint8_t* valid, double* ray_u, double* arc_u, int32_t* gather_arc,
                          void* stream);

/* Workspace of one 2-D trace and its reverse sweeps; n_segments and n_arcs size only the
 * accumulators of the ordered sweeps (tfrt_scene2d.deterministic, 17 B per output entry). */
size_t tfrt_trace2d_workspace_bytes(int64_t n_rays, int64_t n_segments, int64_t n_arcs,
                                    int32_t max_passes, int32_t state_dtype);

/* OpticalEngine.ray_trace for dimension 2 (process_projection_2D, tfrt/engine.py:1544-1986,
 * + snells_law_2D).  In a mixed segment+arc system every pass emits, per class, the
 * segment-hit rays first and then the arc-hit rays (engine.py:1955-1981); the face index
 * written is the merged segment index, or n_segments + merged arc index. */
int tfrt_trace2d_forward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                         const tfrt_scene2d* scene, double new_ray_length,
                         double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                         uint32_t flags, tfrt_ray_out* finished, tfrt_ray_out* active,
                         tfrt_ray_out* stopped, tfrt_ray_out* dead, void* unfinished,
                         int32_t* unfinished_id, int32_t* counts, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Reverse sweep of tfrt_trace2d_forward (the tape part of tfrt/optimizer.py:216-220 for a
 * 2-D system, e.g. dev/optimize_single_arc.py where the variable is an arc's centre/radius).
 *   grad_seg (Ms,4) f64 and grad_arc (Ma,5) f64 are ACCUMULATED into (caller zeroes); the
 *   angle_start/angle_end columns of grad_arc stay zero (they only feed comparisons).
 *   grad_src_rays 4 x n_rays f64 or NULL.
 *   scene->grad_{seg,arc}_n_{in,out}: the per-primitive index gradients, when given. */
int tfrt_trace2d_backward(const void* src_rays, int64_t src_stride, int64_t n_rays,
                          const tfrt_scene2d* scene, double new_ray_length,
                          double dead_ray_length, int32_t max_passes, int32_t state_dtype,
                          const double* grad_finished, int64_t cap_finished,
                          const double* grad_active, int64_t cap_active,
                          const double* grad_stopped, int64_t cap_stopped,
                          const double* grad_dead, int64_t cap_dead, double* grad_seg,
                          double* grad_arc, double* grad_src_rays, const int32_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The built-in goal error (tfrt_goal_error3d's form) folded into the 2-D reverse sweep: ONE
 * launch for the error, its seed 2 (output - goal) and the whole sweep of every pass, in place of
 * tfrt_goal_error3d + max_passes launches of tfrt_trace2d_backward's kernel.  One lane per source
 * ray walks the ray's chain through the tape; a chain that finishes forms its residuals from the
 * row stored in `finished` (state dtype) and leaves their squares in per-wavefront partial sums
 * (a fixed order: the error is bit-identical from run to run).  Any max_passes.
 *   src_rays .. state_dtype, counts, workspace  as for tfrt_trace2d_forward (same call's tape)
 *   finished        the finished-ray block that forward call wrote (rays + capacity; ids unused)
 *   fields[c]       row of the 4-row block (0..3 = x_start, y_start, x_end, y_end), n_fields 1..4
 *   goal            as for tfrt_goal_error3d, rows indexed by the source ray
 *   goal_workspace  tfrt_trace2d_backward_goal_workspace_bytes(n_rays) bytes (the partial sums)
 *   pending         filled in like tfrt_goal_error3d_deferred's: finish with
 *                   tfrt_sgd_process_multi_finish or tfrt_goal_finish ({sum, terms, mean} with
 *                   terms = finished rays x n_fields; tests_total gets the trace's test count)
 *   grad_seg (Ms,4), grad_arc (Ma,5) f64, ACCUMULATED into (caller zeroes), either may be NULL;
 *   lanes that share a primitive are summed inside the wavefront before the global atomic.
 *   scene->grad_{seg,arc}_n_{in,out}: the per-primitive index gradients, when given (summed
 *   inside the wavefront the same way).
 * No class gradients besides the goal's and no source-ray gradient. */
size_t tfrt_trace2d_backward_goal_workspace_bytes(int64_t n_rays);
int tfrt_trace2d_backward_goal(const void* src_rays, int64_t src_stride, int64_t n_rays,
                               const tfrt_scene2d* scene, double new_ray_length,
                               int32_t max_passes, int32_t state_dtype,
                               const tfrt_ray_out* finished, const int32_t* fields,
                               int32_t n_fields, const double* goal, int64_t goal_stride,
                               int64_t goal_ray_stride, double* error_out, int64_t* tests_total,
                               void* goal_workspace, size_t goal_workspace_bytes,
                               tfrt_goal_pending* pending, double* grad_seg, double* grad_arc,
                               const int32_t* counts, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Any row-wise error over the same chains (fused_step.RowwiseError on a 2-D engine): the finished
 * rays as FIXED-SHAPE columns, one per source ray, then the reverse sweep of
 * tfrt_trace2d_backward_goal seeded from the error's gradient with respect to those columns.
 * Between the two calls the caller evaluates the error terms and their gradient (torch autograd,
 * element-wise); no ray count is read on the host, so the sequence can be captured in a graph.
 *   src_rays .. state_dtype, counts, workspace, finished   as for tfrt_trace2d_backward_goal
 * tfrt_trace2d_rows:
 *   rows (4 rows of rows_stride >= n_rays, state dtype)  column i = the row of `finished` source ray
 *                   i's chain ended in, bit for bit; a chain that did not finish gets a finite
 *                   stand-in, source ray i itself
 *   row_face (n_rays) int32  the finished ray's primitive (segment index, Ms + arc index), -1 for
 *                   a chain that did not finish: the mask
 *   Every column is written exactly once: nothing to clear before.
 * tfrt_trace2d_backward_rows:
 *   err_terms       f64, term c of ray i at c * err_stride + i * err_ray_stride, n_terms >= 1;
 *                   summed over the chains that finished in per-wavefront partials (a fixed order)
 *   grad_rows (4 rows of grad_stride >= n_rays, f64)  d error / d rows, or NULL (zero); rows 0, 1
 *                   seed the start gradient and rows 2, 3 the hit gradient of the chain's last
 *                   link, where tfrt_trace2d_backward_goal puts 2 (out - goal)
 *   Both are read only for chains that finished: masked columns may hold NaN or inf.
 *   error_out, tests_total, goal_workspace, pending  as for tfrt_trace2d_backward_goal (terms =
 *                   finished rays x n_terms; tests_total gets the trace's test count when the
 *                   pending sum is finished)
 *   grad_seg (Ms,4), grad_arc (Ma,5) f64, ACCUMULATED into (caller zeroes), either may be NULL;
 *   scene->grad_{seg,arc}_n_{in,out} as for tfrt_trace2d_backward_goal. */
int tfrt_trace2d_rows(const void* src_rays, int64_t src_stride, int64_t n_rays,
                      int32_t max_passes, int32_t state_dtype, const tfrt_ray_out* finished,
                      void* rows, int64_t rows_stride, int32_t* row_face, const int32_t* counts,
                      void* workspace, size_t workspace_bytes, void* stream);
int tfrt_trace2d_backward_rows(const void* src_rays, int64_t src_stride, int64_t n_rays,
                               const tfrt_scene2d* scene, double new_ray_length,
                               int32_t max_passes, int32_t state_dtype,
                               const tfrt_ray_out* finished, const double* err_terms,
                               int32_t n_terms, int64_t err_stride, int64_t err_ray_stride,
                               const double* grad_rows, int64_t grad_stride, double* error_out,
                               int64_t* tests_total, void* goal_workspace,
                               size_t goal_workspace_bytes, tfrt_goal_pending* pending,
                               double* grad_seg, double* grad_arc, const int32_t* counts,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ray order.  The reference's ray sets are ORDERED: every class lists, pass after pass, its rays
 * in the order of the source set (OpticalEngine.ray_trace / single_pass own both: tfrt/engine.py:
 * 2311-2330, the per-pass boolean_mask of :2069-2111, the ray-set properties :1379-1403).  The
 * trace is fastest over rays in a COHERENT order (tfrt_scene3d.coherent_rays).  These four entry
 * points give a caller both: order the source, trace the permuted block, put every class back.
 * Nothing synchronises and every launch has data-independent arguments: a source whose rays are
 * re-drawn every optimiser step (dev/hexalens.py:36-48 builds its source from RandomUniformCircle,
 * tfrt/distributions.py:1590-1592) is ordered inside the step's launch graph.
 *
 * tfrt_ray_order: index[j] = the ray that comes j-th along a Hilbert curve through the points where
 * the rays' lines pass the middle of the scene (foot of the perpendicular from the mean centroid of
 * 64 sampled faces -- or, face_verts == NULL, from the mean end point of 256 sampled rays -- in the
 * plane perpendicular to `axis`, 3 doubles on the HOST, or NULL: the mean direction of the sampled
 * rays; rays without a common direction, |mean| <= 1/2: octahedral map of the directions).  The
 * key has 2 b bits, b = ceil(log2(n) / 2) in [4, 13]; ties keep the source order (a stable
 * radix sort), so index == argsort(keys, stable).  keys_out (n_rays u32, natural order) or NULL. */
size_t tfrt_ray_order_workspace_bytes(int64_t n_rays);
int tfrt_ray_order(const void* rays, int64_t stride, int64_t n_rays, int32_t state_dtype,
                   const double* face_verts, int64_t n_faces, const double* axis, int32_t* index,
                   uint32_t* keys_out, void* workspace, size_t workspace_bytes, void* stream);

/* dst[:, j] = src[:, index[j]] for a 6-row ray block (through 8-element records: one random
 * access per ray instead of six).  src and dst must not overlap. */
size_t tfrt_permute_rays_workspace_bytes(int64_t n_rays, int32_t state_dtype);
int tfrt_permute_rays(const void* src_rays, int64_t src_stride, int64_t n_rays,
                      int32_t state_dtype, const int32_t* index, void* dst_rays,
                      int64_t dst_stride, void* workspace, size_t workspace_bytes, void* stream);

/* dst[k * dst_stride + j] = src[k * src_stride + index[j]], k < n_rows, j < min(n, *n_valid):
 * per-ray rows of any element size (1, 2, 4 or 8 bytes) through an index -- the n(lambda) table
 * and goal rows of an ordered source, the rows of an output class on their way back.  n_valid: a
 * count on the device (entries of `index` beyond it are not read) or NULL. */
int tfrt_gather_rows(const void* src, int64_t src_stride, int32_t n_rows, int32_t elem_bytes,
                     const int32_t* index, int64_t n, const int32_t* n_valid, void* dst,
                     int64_t dst_stride, void* stream);

/* tfrt_scene3d.cluster_order made on the device: the permutation of the faces that makes every
 * aligned run of `leaf` (16: the trace kernels' clusters) and of `group` (128: their superclusters)
 * consecutive entries a compact patch -- recursive median split of the face centroids along the
 * longest axis of their bounding box, the left part a multiple of `group` (of `leaf` below that);
 * faces eight times larger than the median face go last.  No counterpart in the reference (it
 * tests every ray against every face, tfrt/engine.py:1103-1166); once per mesh topology.  No host
 * sync.  group must be a multiple of leaf. */
size_t tfrt_cluster_order_workspace_bytes(int64_t n_faces, int32_t leaf, int32_t group);
int tfrt_cluster_order(const double* face_verts, int64_t n_faces, int32_t leaf, int32_t group,
                       int32_t* order, void* workspace, size_t workspace_bytes, void* stream);

/* One output class of a trace over permuted rays (source ray j of the trace = original ray
 * index[j]) back in the reference's order: inside every pass by original ray index.
 *   ray_id      the class's tfrt_ray_out.ray_id (ids in the trace's numbering), n_rows rows at most
 *   seg_n / seg_base / seg_stride / n_segments   rows and first row of the class in pass p at
 *               seg_n[p * seg_stride] / seg_base[...]: counts + TFRT_CLS_x and counts + 4 +
 *               TFRT_CLS_x with stride TFRT_COUNTS_PER_PASS, max_passes segments (<= 1024).
 *               Both NULL: one segment of n_rows rows (the unfinished set).
 *   total_rows  device count of the class's rows (counts + 8 max_passes + TFRT_CLS_x) or NULL: n_rows
 *   index       the permutation the trace ran over, or NULL (identity: the rows only get ranked)
 *   inv         out, row j of the restored class = row inv[j] of the trace's output   (or NULL)
 *   dest_of     out, the inverse: row r of the output goes to row dest_of[r]          (or NULL)
 *   ray_id_out  out, original ray index of restored row j                             (or NULL)
 * Rows of the restored class: gather with tfrt_gather_rows(.., inv, ..); gradients w.r.t. restored
 * rows on their way into tfrt_trace3d_backward: gather with dest_of. */
size_t tfrt_restore_order_workspace_bytes(int64_t n_src, int32_t n_segments);
int tfrt_restore_order(const int32_t* ray_id, int64_t n_rows, const int32_t* seg_n,
                       const int32_t* seg_base, int32_t seg_stride, int32_t n_segments,
                       const int32_t* total_rows, const int32_t* index, int64_t n_src,
                       int32_t* inv, int32_t* dest_of, int32_t* ray_id_out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Source rays made on the device, in place.  Replaces, for sources that re-draw their rays at
 * every update (dev/hexalens.py:36-48; SGD_Optimizer.single_step calls optical_system.update()
 * first, tfrt/optimizer.py:217): the Random* distributions' _update (tfrt/distributions.py:
 * 1375-1393 square, 1586-1598 circle, 1751-1775 / 1814-1850 spherical caps: tf.random.uniform
 * pushed through the distribution's formula), BasePointTransformation (:2014-2120) and the
 * assembly of the rays by AperatureSource / PointSource / AngularSource._update
 * (tfrt/sources.py:464-1095, undense sources: sample i of every input makes ray i).
 *
 * Random numbers come from a counter-based generator (Philox4x32-10): sample i of a distribution
 * at epoch e is a pure function of (seed, stream, e, i), so rays and points can be written into
 * the caller's persistent buffers by one launch, in any order (through `index`), any number of
 * times, and only the epoch counters -- on the device, advanced by tfrt_epoch_advance -- change
 * from one optimiser step to the next.  The stream of numbers differs from TensorFlow's (whose
 * generator the reference leaves unseeded): parity here is the distribution, not the sequence. */
#define TFRT_PTS_TABLE 0          /* row i of `table` (a static distribution, already transformed) */
#define TFRT_PTS_CIRCLE 1         /* r = sqrt(u0), theta = theta_mod(2 pi u1): (0, R r cos, R r sin) */
#define TFRT_PTS_SQUARE 2         /* (0, -xs + 2 xs u0, -ys + 2 ys u1) */
#define TFRT_PTS_SPHERE_UNIFORM 3 /* phi = acos(lo + (1 - lo) u0), theta = theta_mod(pi (1 + sqrt 5) u1) */
#define TFRT_PTS_SPHERE_LAMBERT 4 /* phi = acos(sqrt(lo + (1 - lo) u0)), lo = cos^2(angular_size) */
/* Points that follow a 2-D density (ArbitraryBasePoints over an ArbitraryDistribution,
 * tfrt/distributions.py:2635-2798 and :2123-2280): with p = {x_min, x_max, y_min, y_max}, x_min < x_max, y_min < y_max,
 *   bx = x_min + (x_max - x_min) u0,  by = y_min + (y_max - y_min) u1,
 *   x = Qx(bx),  cell = floor((x - x_min) x_count / (x_max - x_min)),  y = Qy[cell](by),
 * the point before the transformation (0, x, y).  Q(v) over a table (xs, ys) of m knots is scipy's
 * linear interp1d: k = clamp(first index with xs[k] >= v, 1, m - 1), the line through knots k - 1
 * and k; xs is non-decreasing and may hold equal neighbours.  A sample whose cell is outside
 * [0, min(x_count, y_count)) keeps y = 0 (the reference visits the x cells with range(y_count)).
 * `density` is ONE packed f64 device buffer of 2 (x_count + 1) + 2 x_count (y_count + 1) numbers:
 *   [Qx.xs (x_count + 1) | Qx.ys (x_count + 1) | x_count x (Qy.xs (y_count + 1) | Qy.ys (y_count + 1))]
 * `rank_density` (or NULL) has the same layout and counts: aux0 / aux1 are rank_scale times its map
 * of the same (bx, by); 0 without it.  Search, cell and interpolation run in float64 wherever the
 * program is evaluated (the result is rounded to the evaluation's type at the end), so that the
 * order's float32 keys belong to the very rays that are traced: a cell chosen in float32 could take
 * another y curve. */
#define TFRT_PTS_DENSITY 5
typedef struct tfrt_points_program {
  int32_t kind;          /* TFRT_PTS_* */
  int32_t stream;        /* distinguishes the distributions that share a seed */
  int64_t count;         /* samples of the distribution */
  const double* table;   /* TFRT_PTS_TABLE: (count, 3) f64 */
  /* circle: {radius, theta_start, theta_end, -}; square: {x_size, -, -, y_size} (centre to
   * edge); spheres: {radius, theta_start, theta_end, lo}, lo = cos(angular_size) [uniform] or its
   * square [Lambertian]; density: {x_min, x_max, y_min, y_max} */
  double p[4];
  double scale[3], quat[4], shift[3]; /* BasePointTransformation: scale, unit quaternion (w, x, y, z), translation */
  int32_t has_scale, has_quat, has_shift;
  int32_t reserved0;
  uint64_t seed;
  const int64_t* epoch;  /* device counter (one int64): the number of updates so far */
  /* TFRT_PTS_DENSITY only (zero otherwise) */
  int32_t x_count, y_count; /* cells of the density grid, >= 1 */
  const double* density; /* the packed quantile tables (see TFRT_PTS_DENSITY) */
  const double* rank_density; /* the rank distribution's, same counts and limits; or NULL */
  double rank_scale;
} tfrt_points_program;

#define TFRT_SRC_APERTURE 0 /* start = a[i], end = b[i]                                      sources.py:918-1095 */
#define TFRT_SRC_POINT 1    /* start = center, end = center + L rot(b[i])                    sources.py:464-675 */
#define TFRT_SRC_ANGULAR 2  /* start = center + rot(a[i]), end = start + L rot(b[i])         sources.py:678-915 */
/* A stored pool of rays, re-sampled with replacement and jittered at every update (PrecompiledSource,
 * tfrt/sources.py:1099-1358): ray i at epoch e is pool row
 *   row = pool_downsample ? min(floor(u0 * pool_count), pool_count - 1) : i,
 * u0 the first number of Philox(pool_seed, pool_stream, e, i) -- the product in float64 wherever the
 * program is evaluated, so that the order's float32 keys belong to the very rays that are traced --,
 * plus sigma_start / sigma_end times standard normals: Box-Muller, sqrt(-2 log(1 - u)) (cos, sin)(2 pi v),
 * on the pair (u, v) of stream pool_stream + 1 + axis, which gives the axis's (start, end) normals.
 * An axis whose sigma is 0 is not touched: the coordinate is the stored one bit for bit.  `a`, `b`,
 * center, quat, ray_length and swap are unused. */
#define TFRT_SRC_POOL 3
typedef struct tfrt_source3d_program {
  int32_t kind;          /* TFRT_SRC_* */
  int32_t swap;          /* start and end exchanged (start_on_center / start_on_base false) */
  tfrt_points_program a; /* start points / base points (unused by TFRT_SRC_POINT) */
  tfrt_points_program b; /* end points / direction vectors */
  double center[3];
  double quat[4];        /* central angle as a unit quaternion */
  int32_t has_quat, reserved0;
  double ray_length;
  int64_t n_rays;        /* every input has 1 or n_rays samples */
  /* TFRT_SRC_POOL only (zero otherwise) */
  const double* pool;    /* (pool_count, 6) f64 ROW-major: one 48-byte record x_start ... z_end per stored ray */
  int64_t pool_count;    /* 1 ... INT32_MAX */
  double sigma_start[3], sigma_end[3]; /* standard deviations of the jitter per axis, >= 0 */
  int32_t pool_downsample; /* 0: ray i is row i (n_rays == pool_count) */
  int32_t pool_stream;   /* streams pool_stream ... pool_stream + 3 of the seed */
  uint64_t pool_seed;
  const int64_t* pool_epoch; /* device counter; may be NULL when nothing is sampled or jittered */
} tfrt_source3d_program;

/* tfrt_ray_order for rays first .. first + n_rays of a source program, without the rays ever being
 * written in source order: index[j] = the j-th ray (counted from `first`) in the coherent order.
 * Workspace: tfrt_ray_order_workspace_bytes(n_rays).  tfrt_source3d_generate(program, index, first,
 * ...) then makes the ordered block. */
int tfrt_source3d_order(const tfrt_source3d_program* program, int64_t first, int64_t n_rays,
                        const double* face_verts, int64_t n_faces, const double* axis,
                        int32_t* index, uint32_t* keys_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The same order up to ties, made faster, for a source that is re-drawn before every optimiser step
 * (distributions.py:1586-1598: the order is made again every step): most significant digit first --
 * ONE stable scatter by the key's high digit, then every bucket of it is sorted by the low digit in
 * LDS (one workgroup per bucket) -- five launches instead of the two-pass sort's eight.  Rays with
 * the SAME key (the same cell of the key grid: about one ray per cell) land in an order that may vary
 * from run to run.  A trace's results do not depend on the order of its rays (tfrt_scene3d.ray_slot
 * numbers them as the caller does); only the rounding of sums over rays does, as with any atomic
 * accumulation.  Not for deterministic runs.  Same arguments and workspace as tfrt_source3d_order. */
int tfrt_source3d_order_cells(const tfrt_source3d_program* program, int64_t first, int64_t n_rays,
                              const double* face_verts, int64_t n_faces, const double* axis,
                              int32_t* index, uint32_t* keys_out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* epochs[k][0] += 1 for k < n (n <= 8 distinct device counters, host array of pointers): one
 * launch for all the distributions a source draws from. */
int tfrt_epoch_advance(int64_t* const* epochs, int32_t n, void* stream);

/* Samples first + index[j] (NULL: first + j), j < n, of one distribution at its current epoch: the points after
 * the transformation as (n, 3) f64 rows (point_columns 3) or the distribution's own plane as
 * (n, 2) rows (point_columns 2: components y, z), and the two numbers its rank properties are made
 * of (circle: r in [0, 1] and theta; spheres: phi and theta; square: the point before the
 * transformation; density: the rank point's two components) -- each output may be NULL. */
int tfrt_points_generate(const tfrt_points_program* program, const int32_t* index,
                         int64_t first, int64_t n, double* points, int32_t point_columns, double* aux0, double* aux1,
                         void* stream);

/* Rays first + index[j] (NULL: first + j), j < n (`first`: a rank's shard of the source), of the
 * source at the current epochs of its distributions:
 * `rays` a 6 x stride block of the state dtype and / or `fields` a 6 x field_stride f64 block
 * (x_start ... z_end: the source's field columns); either may be NULL. */
int tfrt_source3d_generate(const tfrt_source3d_program* program, const int32_t* index,
                           int64_t first, int64_t n, int32_t state_dtype, void* rays, int64_t stride, double* fields,
                           int64_t field_stride, void* stream);

/* TFRT_SRC_POOL: rows[j] = the pool row of ray first + index[j] (NULL: first + j), j < n, at the
 * current epoch -- the row tfrt_source3d_generate and the order's keys read for that ray (the same
 * device function), so that a caller can gather every stored field that is not geometry. */
int tfrt_source3d_pool_rows(const tfrt_source3d_program* program, const int32_t* index,
                            int64_t first, int64_t n, int32_t* rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * 2-D sources made on the device.  Replaces, for 2-D sources that re-draw their rays at every
 * update (dev/light_guide.py:45-49): the _update of RandomUniformAngularDistribution,
 * RandomLambertianAngularDistribution, RandomUniformBeam and RandomUniformAperaturePoints
 * (tfrt/distributions.py: tf.random.uniform pushed through the distribution's formula) and the
 * 2-D branches of AperatureSource / PointSource / AngularSource._update (tfrt/sources.py:464-1095,
 * undense sources).  The generator, the epoch counters and their meaning are those of the 3-D
 * programs above; as there, parity with the reference is the distribution, not the sequence.
 *
 * A samples program is a 1-D distribution: sample i is made of ONE uniform number u, the first of
 * Philox4x32-10(seed, stream, epoch, i) (the second is unused), as v = lo + (hi - lo) u, in
 * float64.  It yields a value -- an angle (one column) or a point (two columns) -- and a rank. */
#define TFRT_SMP_TABLE 0          /* value = row i of `table`; no rank (0) */
#define TFRT_SMP_UNIFORM_ANGLE 1  /* angle = v in [lo, hi]; rank = angle / rank_scale,
                                     rank_scale = max(|lo|, |hi|, 1e-300) */
#define TFRT_SMP_LAMBERT_ANGLE 2  /* rank = v, lo = sin(min_angle), hi = sin(max_angle); angle = asin(rank) */
#define TFRT_SMP_BEAM 3           /* rank = v in [r0, r1] = [lo, hi]; point = p0 * rank (p0: the beam's endpoint) */
#define TFRT_SMP_APERTURE_POINTS 4 /* rank = u (lo = 0, hi = 1); point = p0 + rank * (p1 - p0) */
typedef struct tfrt_samples_program {
  int32_t kind;          /* TFRT_SMP_* */
  int32_t stream;        /* distinguishes the distributions that share a seed */
  int64_t count;         /* samples of the distribution */
  const double* table;   /* TFRT_SMP_TABLE: (count, columns) f64 rows */
  int32_t columns;       /* TFRT_SMP_TABLE: 1 (angles) or 2 (points); the other kinds have their own */
  int32_t reserved0;
  double lo, hi;         /* limits of the uniform draw, lo <= hi */
  double rank_scale;     /* TFRT_SMP_UNIFORM_ANGLE */
  double p0[2], p1[2];   /* TFRT_SMP_BEAM: endpoint, -; TFRT_SMP_APERTURE_POINTS: start, end */
  uint64_t seed;
  const int64_t* epoch;  /* device counter (one int64): the number of updates so far */
} tfrt_samples_program;

/* TFRT_SRC_APERTURE: start = a[i], end = b[i] (both point-valued);
 * TFRT_SRC_POINT:    start = center, end = start + L (cos t, sin t), t = b[i] + central_angle;
 * TFRT_SRC_ANGULAR:  start = center + R(central_angle) a[i], end as for TFRT_SRC_POINT
 * (a point-valued, b angle-valued; `swap` exchanges start and end).
 * TFRT_SRC_POOL:     a stored pool of 2-D rays, re-sampled with replacement and jittered at every
 * update (a 2-D PrecompiledSource): the draw of the 3-D pool program with two axes.  Ray i at epoch e
 * -- e = *pool_epoch, read only when the program down-samples or has a positive sigma; otherwise 0,
 * and the pointer may be NULL -- is pool row
 *   row = pool_downsample ? clamp(floor(u0 * pool_count), 0, pool_count - 1) : i,
 * u0 the first number of Philox4x32-10(pool_seed, pool_stream, e, i), the product in float64.  Every
 * axis q in {0, 1} with a positive sigma takes the pair (u, v) of stream pool_stream + 1 + q at
 * (e, i) and r = sqrt(-2 log(1 - u)): the start point moves by sigma_start[q] r cos(2 pi v), the end
 * point by sigma_end[q] r sin(2 pi v).  A coordinate whose sigma is 0 is the stored one bit for bit.
 * All of it in float64, rounded once to the state dtype.  `a`, `b`, center, central_angle, rot,
 * ray_length and swap are unused by this kind. */
typedef struct tfrt_source2d_program {
  int32_t kind;          /* TFRT_SRC_APERTURE / TFRT_SRC_POINT / TFRT_SRC_ANGULAR / TFRT_SRC_POOL */
  int32_t swap;          /* start and end exchanged (start_on_center / start_on_base false) */
  tfrt_samples_program a; /* start points / base points (unused by TFRT_SRC_POINT) */
  tfrt_samples_program b; /* end points / angles */
  double center[2];
  double central_angle;
  double rot[2];         /* cos, sin of central_angle, made on the host: R(central_angle) turns the
                            base points of TFRT_SRC_ANGULAR (the same for every ray) */
  double ray_length;
  int64_t n_rays;        /* every input has 1 or n_rays samples */
  /* TFRT_SRC_POOL only (zero otherwise) */
  const double* pool;    /* (pool_count, 4) f64 ROW-major: one 32-byte record x_start, y_start, x_end, y_end per stored ray */
  int64_t pool_count;    /* 1 ... INT32_MAX */
  double sigma_start[2], sigma_end[2]; /* standard deviations of the jitter per axis, >= 0 */
  int32_t pool_downsample; /* 0: ray i is row i (n_rays == pool_count) */
  int32_t pool_stream;   /* streams pool_stream ... pool_stream + 2 of the seed */
  uint64_t pool_seed;
  const int64_t* pool_epoch; /* device counter; may be NULL when nothing is sampled or jittered */
} tfrt_source2d_program;

/* Samples first + index[j] (NULL: first + j), j < n, of one 1-D distribution at its current epoch:
 * `values` (n, value_columns) f64 rows -- value_columns must be the program's own (1: angles, 2:
 * points) -- and / or `ranks` (n) f64; either may be NULL.  Refused with TFRT_E_BADARG before any
 * launch: a kind out of range, a random kind without an epoch counter, lo > hi (or a NaN limit),
 * a table without storage or with columns other than 1 or 2. */
int tfrt_samples_generate(const tfrt_samples_program* program, const int32_t* index,
                          int64_t first, int64_t n, double* values, int32_t value_columns,
                          double* ranks, void* stream);

/* Rays first + index[j] (NULL: first + j), j < n, of a 2-D source at the current epochs of its
 * distributions: `rays` a 4 x stride block of the state dtype and / or `fields` a 4 x field_stride
 * f64 block (x_start, y_start, x_end, y_end); either may be NULL.  The block is the float64 result
 * rounded once to the state dtype.  Refused like tfrt_samples_generate, and when an input is not
 * point- / angle-valued as the kind needs, or has neither one sample nor n_rays.  A TFRT_SRC_POOL
 * program is refused when `pool` is NULL, pool_count is not in 1 ... INT32_MAX, a sigma is negative
 * or not finite, pool_epoch is NULL although the program down-samples or perturbs, or it does not
 * down-sample and n_rays != pool_count. */
int tfrt_source2d_generate(const tfrt_source2d_program* program, const int32_t* index,
                           int64_t first, int64_t n, int32_t state_dtype, void* rays, int64_t stride,
                           double* fields, int64_t field_stride, void* stream);

/* TFRT_SRC_POOL: rows[j] = the pool row of ray first + index[j] (NULL: first + j), j < n, at the
 * current epoch -- the row tfrt_source2d_generate reads for that ray (the same device function), so
 * that a caller can gather every stored field that is not geometry.  Refused like
 * tfrt_source2d_generate, and for a program of another kind. */
int tfrt_source2d_pool_rows(const tfrt_source2d_program* program, const int32_t* index,
                            int64_t first, int64_t n, int32_t* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TFRT_HIP_H */
