// Device functions of the source programs (tfrt_points_program / tfrt_source3d_program and their 2-D
// counterparts tfrt_samples_program / tfrt_source2d_program): shared by
// csrc/tfrt_source.hip (rays and points into the caller's buffers) and csrc/tfrt_order.hip (the
// coherent order of a program's rays without ever writing them in source order).
#pragma once
#include <cfloat>
#include <cstdint>
#include "tfrt_common.h"
#include "density_map.h"

namespace tfrt {

__device__ __forceinline__ void philox_round(uint32_t c[4], const uint32_t k[2]) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0];
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
  c[0] = n0;
  c[1] = (uint32_t)p1;
  c[2] = n2;
  c[3] = (uint32_t)p0;
}

// two uniform float64 in [0, 1) (53 bits each) for (seed, stream, epoch, sample)
__device__ __forceinline__ void uniform2(uint64_t seed, uint32_t stream, uint64_t epoch,
                                         uint64_t sample, double* u0, double* u1) {
  uint32_t c[4] = {(uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)epoch,
                   (uint32_t)(epoch >> 32)};
  uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32) ^ stream};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k);
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  const uint64_t a = ((uint64_t)c[0] << 32) | c[1], b = ((uint64_t)c[2] << 32) | c[3];
  *u0 = (double)(a >> 11) * 0x1.0p-53;
  *u1 = (double)(b >> 11) * 0x1.0p-53;
}

// (the programs evaluate in float64 for the rays and points they hand out, and in float32 for the
// coherent order's keys, where a cell of the key grid is 2^-10 of the extent)
__device__ __forceinline__ double m_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float m_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double m_fmod(double x, double y) { return fmod(x, y); }
__device__ __forceinline__ float m_fmod(float x, float y) { return fmodf(x, y); }
__device__ __forceinline__ double m_acos(double x) { return acos(x); }
__device__ __forceinline__ float m_acos(float x) { return acosf(x); }
__device__ __forceinline__ double m_fmax(double x, double y) { return fmax(x, y); }
__device__ __forceinline__ float m_fmax(float x, float y) { return fmaxf(x, y); }
__device__ __forceinline__ void m_sincos(double x, double* s, double* c) { sincos(x, s, c); }
__device__ __forceinline__ void m_sincos(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ void m_sincospi(double x, double* s, double* c) { sincospi(x, s, c); }
__device__ __forceinline__ void m_sincospi(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ double m_log(double x) { return log(x); }
__device__ __forceinline__ float m_log(float x) { return logf(x); }

template <typename F>
__device__ __forceinline__ void quat_rotate(const double qd[4], F v[3]) {
  // v' = v + w t + u x t, t = 2 u x v   (q = (w, u) a unit quaternion)
  const F q[4] = {(F)qd[0], (F)qd[1], (F)qd[2], (F)qd[3]};
  const F t0 = (F)2 * (q[2] * v[2] - q[3] * v[1]);
  const F t1 = (F)2 * (q[3] * v[0] - q[1] * v[2]);
  const F t2 = (F)2 * (q[1] * v[1] - q[2] * v[0]);
  const F r0 = v[0] + q[0] * t0 + (q[2] * t2 - q[3] * t1);
  const F r1 = v[1] + q[0] * t1 + (q[3] * t0 - q[1] * t2);
  const F r2 = v[2] + q[0] * t2 + (q[1] * t1 - q[2] * t0);
  v[0] = r0;
  v[1] = r1;
  v[2] = r2;
}

// TFRT_PTS_DENSITY: the plane point xy and the rank point rk of the uniform pair (u0, u1), in
// float64 whatever the caller evaluates in.
__device__ __forceinline__ void density_point(const tfrt_points_program& pg, double u0, double u1,
                                              double xy[2], double rk[2]) {
  const double bx = pg.p[0] + (pg.p[1] - pg.p[0]) * u0;
  const double by = pg.p[2] + (pg.p[3] - pg.p[2]) * u1;
  density_map(pg.density, pg.x_count, pg.y_count, pg.p, bx, by, &xy[0], &xy[1]);
  rk[0] = rk[1] = 0.0;
  if (pg.rank_density != nullptr) {
    density_map(pg.rank_density, pg.x_count, pg.y_count, pg.p, bx, by, &rk[0], &rk[1]);
    rk[0] *= pg.rank_scale;
    rk[1] *= pg.rank_scale;
  }
}

constexpr double TWO_PI = 6.283185307179586476925286766559;
constexpr double GOLDEN_TURN = 3.14159265358979323846 * (1.0 + 2.2360679774997896964);  // pi (1 + sqrt 5)

// Sample `i` of a points program: the 3-D point (after the transformation) and the two numbers the
// distribution's rank properties are made of (circle: r in [0, 1], theta; sphere: phi, theta;
// density: the rank point).  DENSITY: the program may be a TFRT_PTS_DENSITY one -- the host picks the
// instantiation by the program's kind, as for the pool (see eval_ray): inlined into the one kernel
// of all kinds, the two binary searches cost the order's key kernel 21 VGPRs (108 -> 129) and a
// wavefront of occupancy whatever the kind; behind a call, 17.
template <typename F, bool DENSITY = false>
__device__ __forceinline__ void eval_points(const tfrt_points_program& pg, int64_t i, F out[3],
                                            F aux[2]) {
  F p[3] = {(F)0, (F)0, (F)0};
  aux[0] = aux[1] = (F)0;
  if (pg.kind == TFRT_PTS_TABLE) {
    const double* row = pg.table + 3 * i;
    p[0] = (F)row[0];
    p[1] = (F)row[1];
    p[2] = (F)row[2];
  } else {
    double ud0, ud1;
    uniform2(pg.seed, pg.stream, (uint64_t)*pg.epoch, (uint64_t)i, &ud0, &ud1);
    const F u0 = (F)ud0, u1 = (F)ud1;
    const F P0 = (F)pg.p[0], P1 = (F)pg.p[1], P2 = (F)pg.p[2], P3 = (F)pg.p[3];
    // theta = turns * pi, folded into the wedge [theta_start, theta_end) when there is one
    // (distributions.py:1396-1447); sine and cosine straight from the half-turns when there is
    // none (sincospi: no range reduction against a rounded pi)
    const bool wedge = !(pg.p[1] == 0.0 && pg.p[2] == TWO_PI);
    auto angle = [&](F half_turns, F* th, F* sn, F* cs) {
      F t = half_turns * (F)3.14159265358979323846;
      if (wedge) {
        const F span = P2 - P1;
        F m = m_fmod(t, span);
        if (m != (F)0 && ((m < (F)0) != (span < (F)0))) m += span;   // (sign of the divisor)
        t = m + P1;
        m_sincos(t, sn, cs);
      } else {
        m_sincospi(half_turns, sn, cs);
      }
      *th = t;
    };
    if (pg.kind == TFRT_PTS_CIRCLE) {            // p = {radius, theta_start, theta_end}
      const F r = m_sqrt(u0);
      F th, sn, cs;
      angle((F)2 * u1, &th, &sn, &cs);
      p[1] = P0 * (r * cs);
      p[2] = P0 * (r * sn);
      aux[0] = r;
      aux[1] = th;
    } else if (pg.kind == TFRT_PTS_SQUARE) {     // p = {x_size, -, -, y_size}
      p[1] = -P0 + ((F)2 * P0) * u0;
      p[2] = -P3 + ((F)2 * P3) * u1;
      aux[0] = p[1];
      aux[1] = p[2];
    } else if (DENSITY && pg.kind == TFRT_PTS_DENSITY) {    // p = {x_min, x_max, y_min, y_max}
      double xy[2], rk[2];
      density_point(pg, ud0, ud1, xy, rk);
      p[1] = (F)xy[0];
      p[2] = (F)xy[1];
      aux[0] = (F)rk[0];
      aux[1] = (F)rk[1];
    } else {                                     // p = {radius, theta_start, theta_end, lower bound}
      const F c = P3 + ((F)1 - P3) * u0;
      // cos(phi) = c (uniform cap) or sqrt(c) (Lambertian: cos^2 is uniform); sin from it
      const F cp = pg.kind == TFRT_PTS_SPHERE_LAMBERT ? m_sqrt(c) : c;
      const F sp = m_sqrt(m_fmax((F)0, ((F)1 - cp) * ((F)1 + cp)));
      F th, sn, cs;
      angle((F)(1.0 + 2.2360679774997896964) * u1, &th, &sn, &cs);   // theta = pi (1 + sqrt 5) u
      p[0] = P0 * cp;
      p[1] = P0 * (sp * cs);
      p[2] = P0 * (sp * sn);
      aux[0] = m_acos(cp);
      aux[1] = th;
    }
    // BasePointTransformation (distributions.py:2014-2120): scale, rotate, translate
    if (pg.has_scale) {
      p[0] *= (F)pg.scale[0];
      p[1] *= (F)pg.scale[1];
      p[2] *= (F)pg.scale[2];
    }
    if (pg.has_quat) quat_rotate<F>(pg.quat, p);
    if (pg.has_shift) {
      p[0] += (F)pg.shift[0];
      p[1] += (F)pg.shift[1];
      p[2] += (F)pg.shift[2];
    }
  }
  out[0] = p[0];
  out[1] = p[1];
  out[2] = p[2];
}

// TFRT_SRC_POOL, 3-D and 2-D alike (SP: tfrt_source3d_program / tfrt_source2d_program, whose pool
// fields carry the same names; the axes are counted from sigma_start).
template <typename SP>
constexpr int pool_axes() {
  return (int)(sizeof(SP::sigma_start) / sizeof(double));
}

// The stored row ray i is made from at `epoch`.  Float64 whatever the caller evaluates in: a
// float32 product could name another row than the one that is traced.
template <typename SP>
__device__ __forceinline__ int64_t pool_row(const SP& sp, int64_t i, uint64_t epoch) {
  const int64_t last = sp.pool_count - 1;
  int64_t row = i;
  if (sp.pool_downsample) {
    double u0, u1;
    uniform2(sp.pool_seed, (uint32_t)sp.pool_stream, epoch, (uint64_t)i, &u0, &u1);
    row = (int64_t)floor(u0 * (double)sp.pool_count);
  }
  return row < 0 ? 0 : (row > last ? last : row);   // (never outside the pool, whatever `i` is)
}

template <typename SP>
__device__ __forceinline__ bool pool_perturbs(const SP& sp) {
  bool any = false;
#pragma unroll
  for (int q = 0; q < pool_axes<SP>(); ++q)
    any = any || sp.sigma_start[q] > 0.0 || sp.sigma_end[q] > 0.0;
  return any;
}

// ray i of a pool: the record of its row (48 bytes in 3-D, 32 in 2-D: the start point, then the end
// point), every axis with a sigma moved by sigma * z
template <typename F, typename SP>
__device__ __forceinline__ void eval_pool(const SP& sp, int64_t i, F* s, F* e) {
  constexpr int AXES = pool_axes<SP>();
  const bool jitter = pool_perturbs(sp);
  const uint64_t epoch = (sp.pool_downsample || jitter) ? (uint64_t)*sp.pool_epoch : 0;
  const double* rec = sp.pool + 2 * AXES * pool_row(sp, i, epoch);
#pragma unroll
  for (int q = 0; q < AXES; ++q) {
    s[q] = (F)rec[q];
    e[q] = (F)rec[AXES + q];
  }
  if (!jitter) return;
#pragma unroll
  for (int q = 0; q < AXES; ++q) {
    if (!(sp.sigma_start[q] > 0.0 || sp.sigma_end[q] > 0.0)) continue;
    double u, v;
    uniform2(sp.pool_seed, (uint32_t)(sp.pool_stream + 1 + q), epoch, (uint64_t)i, &u, &v);
    // (1 - u in (0, 1] in float64: the logarithm stays finite, |z| <= sqrt(106 log 2) = 8.57)
    const F r = m_sqrt((F)-2 * m_log((F)(1.0 - u)));
    F sn, cs;
    m_sincospi((F)(2.0 * v), &sn, &cs);
    if (sp.sigma_start[q] > 0.0) s[q] += (F)sp.sigma_start[q] * (r * cs);
    if (sp.sigma_end[q] > 0.0) e[q] += (F)sp.sigma_end[q] * (r * sn);
  }
}

// ray i of the source (natural numbering).  POOL: the program is a TFRT_SRC_POOL one -- the host
// picks the instantiation by the program's kind, so that the kernels of the procedural kinds carry
// nothing of the pool's code or registers, and the pool's nothing of theirs.  DENSITY: one of the
// inputs is a TFRT_PTS_DENSITY program (source_program_density), in the same way.
template <bool POOL = false, bool DENSITY = false, typename F>
__device__ __forceinline__ void eval_ray(const tfrt_source3d_program& sp, int64_t i, F s[3],
                                         F e[3]) {
  if constexpr (POOL) {
    eval_pool<F>(sp, i, s, e);
    return;
  }
  F a[3] = {(F)0, (F)0, (F)0}, b[3] = {(F)0, (F)0, (F)0}, aux[2];
  const int64_t ia = sp.a.count == 1 ? 0 : i, ib = sp.b.count == 1 ? 0 : i;
  if (sp.kind == TFRT_SRC_APERTURE) {
    eval_points<F, DENSITY>(sp.a, ia, s, aux);
    eval_points<F, DENSITY>(sp.b, ib, e, aux);
    return;
  }
  eval_points<F, DENSITY>(sp.b, ib, b, aux);   // the direction vectors
  if (sp.has_quat) quat_rotate<F>(sp.quat, b);
  if (sp.kind == TFRT_SRC_ANGULAR) {
    eval_points<F, DENSITY>(sp.a, ia, a, aux);
    if (sp.has_quat) quat_rotate<F>(sp.quat, a);
  }
  F st[3], en[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    st[q] = (F)sp.center[q] + a[q];
    en[q] = st[q] + (F)sp.ray_length * b[q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    s[q] = sp.swap ? en[q] : st[q];
    e[q] = sp.swap ? st[q] : en[q];
  }
}

// ------------------------------------------------------------------------------------ 2-D
// Sample `i` of a 1-D samples program, in float64: its value (v[0] an angle, or v[0], v[1] a point)
// and its rank.  One Philox call per sample: the first number only (distributions.py: _uniform's
// low + (high - low) * u, then the distribution's own formula).
__device__ __forceinline__ void eval_sample(const tfrt_samples_program& pg, int64_t i, double v[2],
                                            double* rank) {
  v[0] = v[1] = 0.0;
  *rank = 0.0;
  if (pg.kind == TFRT_SMP_TABLE) {
    // (never outside the table, whatever an `index` entry says; count >= 1 when anything is launched)
    const int64_t r = i < 0 ? 0 : (i >= pg.count ? pg.count - 1 : i);
    const double* row = pg.table + pg.columns * r;
    v[0] = row[0];
    if (pg.columns == 2) v[1] = row[1];
    return;
  }
  double u, unused;
  uniform2(pg.seed, (uint32_t)pg.stream, (uint64_t)*pg.epoch, (uint64_t)i, &u, &unused);
  const double d = pg.lo + (pg.hi - pg.lo) * u;
  if (pg.kind == TFRT_SMP_UNIFORM_ANGLE) {
    v[0] = d;
    *rank = d / pg.rank_scale;
  } else if (pg.kind == TFRT_SMP_LAMBERT_ANGLE) {
    v[0] = asin(d);
    *rank = d;
  } else if (pg.kind == TFRT_SMP_BEAM) {
    v[0] = pg.p0[0] * d;
    v[1] = pg.p0[1] * d;
    *rank = d;
  } else {                                       // TFRT_SMP_APERTURE_POINTS (lo = 0, hi = 1: d = u)
    v[0] = pg.p0[0] + d * (pg.p1[0] - pg.p0[0]);
    v[1] = pg.p0[1] + d * (pg.p1[1] - pg.p0[1]);
    *rank = d;
  }
}

// ray i of a 2-D source (the 2-D branches of sources.py's _internal_update): s, e = (x, y).
// POOL: as for eval_ray -- the host picks the instantiation by the program's kind.
template <bool POOL = false>
__device__ __forceinline__ void eval_ray2(const tfrt_source2d_program& sp, int64_t i, double s[2],
                                          double e[2]) {
  if constexpr (POOL) {
    eval_pool<double>(sp, i, s, e);
    return;
  }
  const int64_t ia = sp.a.count == 1 ? 0 : i, ib = sp.b.count == 1 ? 0 : i;
  double rank;
  if (sp.kind == TFRT_SRC_APERTURE) {
    eval_sample(sp.a, ia, s, &rank);
    eval_sample(sp.b, ib, e, &rank);
    return;
  }
  double ang[2], st[2] = {sp.center[0], sp.center[1]};
  eval_sample(sp.b, ib, ang, &rank);
  if (sp.kind == TFRT_SRC_ANGULAR) {
    double base[2];
    eval_sample(sp.a, ia, base, &rank);
    st[0] += sp.rot[0] * base[0] - sp.rot[1] * base[1];   // (cos, sin from the host: uniform)
    st[1] += sp.rot[1] * base[0] + sp.rot[0] * base[1];
  }
  double sn, cs;
  sincos(ang[0] + sp.central_angle, &sn, &cs);
  const double en[2] = {st[0] + sp.ray_length * cs, st[1] + sp.ray_length * sn};
  s[0] = sp.swap ? en[0] : st[0];
  s[1] = sp.swap ? en[1] : st[1];
  e[0] = sp.swap ? st[0] : en[0];
  e[1] = sp.swap ? st[1] : en[1];
}

// Host-side validity of the programs: everything a kernel dereferences or indexes by
// (tfrt_points_generate, tfrt_source3d_generate and tfrt_source3d_order refuse what fails here with
// TFRT_E_BADARG instead of launching on it).
inline bool points_program_ok(const tfrt_points_program* pg) {
  if (!pg || pg->count < 0) return false;
  if (pg->kind == TFRT_PTS_TABLE) return pg->count == 0 || pg->table != nullptr;
  if (pg->kind < TFRT_PTS_TABLE || pg->kind > TFRT_PTS_DENSITY) return false;
  if (pg->kind == TFRT_PTS_DENSITY) {
    // the tables the searches read, their sizes, a rectangle with an inside (a NaN limit fails too)
    if (pg->density == nullptr || pg->x_count < 1 || pg->y_count < 1) return false;
    if (!(pg->p[0] < pg->p[1] && pg->p[2] < pg->p[3])) return false;
    if (!(pg->p[0] >= -DBL_MAX && pg->p[1] <= DBL_MAX && pg->p[2] >= -DBL_MAX && pg->p[3] <= DBL_MAX))
      return false;
  }
  return pg->epoch != nullptr;
}

// a pool program: the pool and its size, the widths, the counter whenever a kernel reads it
template <typename SP>
inline bool pool_program_ok(const SP* sp) {
  if (sp->pool == nullptr || sp->pool_count <= 0 || sp->pool_count > (int64_t)INT32_MAX)
    return false;
  bool jitter = false;
  for (int q = 0; q < pool_axes<SP>(); ++q) {
    const double a = sp->sigma_start[q], b = sp->sigma_end[q];
    if (!(a >= 0.0 && a <= DBL_MAX && b >= 0.0 && b <= DBL_MAX)) return false;   // (negative, inf, NaN)
    jitter = jitter || a > 0.0 || b > 0.0;
  }
  if ((sp->pool_downsample || jitter) && sp->pool_epoch == nullptr) return false;
  return sp->pool_downsample || sp->n_rays == sp->pool_count;
}

// a valid procedural program one of whose inputs is a TFRT_PTS_DENSITY one: the DENSITY kernels
inline bool source_program_density(const tfrt_source3d_program* sp) {
  return sp->kind != TFRT_SRC_POOL && (sp->b.kind == TFRT_PTS_DENSITY ||
                                       (sp->kind != TFRT_SRC_POINT && sp->a.kind == TFRT_PTS_DENSITY));
}

inline bool source_program_ok(const tfrt_source3d_program* sp) {
  if (!sp || sp->n_rays < 0) return false;
  if (sp->kind == TFRT_SRC_POOL) return pool_program_ok(sp);
  if (sp->kind < TFRT_SRC_APERTURE || sp->kind > TFRT_SRC_ANGULAR) return false;
  if (!points_program_ok(&sp->b)) return false;
  if (sp->kind != TFRT_SRC_POINT && !points_program_ok(&sp->a)) return false;
  // (undense: every input has one sample or one per ray)
  const int64_t ca = sp->kind == TFRT_SRC_POINT ? 1 : sp->a.count, cb = sp->b.count;
  return (ca == 1 || ca == sp->n_rays) && (cb == 1 || cb == sp->n_rays);
}

// columns of a samples program's value: 1 (an angle), 2 (a point), 0: not a valid program
inline int samples_program_columns(const tfrt_samples_program* pg) {
  if (!pg || pg->count < 0) return 0;
  if (pg->kind == TFRT_SMP_TABLE) {
    if (pg->columns != 1 && pg->columns != 2) return 0;
    return (pg->count == 0 || pg->table != nullptr) ? pg->columns : 0;
  }
  if (pg->kind < TFRT_SMP_TABLE || pg->kind > TFRT_SMP_APERTURE_POINTS) return 0;
  if (pg->epoch == nullptr || !(pg->lo <= pg->hi)) return 0;     // (a NaN limit fails too)
  return pg->kind <= TFRT_SMP_LAMBERT_ANGLE ? 1 : 2;
}

inline bool source2d_program_ok(const tfrt_source2d_program* sp) {
  if (!sp || sp->n_rays < 0) return false;
  if (sp->kind == TFRT_SRC_POOL) return pool_program_ok(sp);
  if (sp->kind < TFRT_SRC_APERTURE || sp->kind > TFRT_SRC_ANGULAR) return false;
  // aperture: two point sets; point / angular: angles, and base points for the latter
  if (samples_program_columns(&sp->b) != (sp->kind == TFRT_SRC_APERTURE ? 2 : 1)) return false;
  if (sp->kind != TFRT_SRC_POINT && samples_program_columns(&sp->a) != 2) return false;
  const int64_t ca = sp->kind == TFRT_SRC_POINT ? 1 : sp->a.count, cb = sp->b.count;
  return (ca == 1 || ca == sp->n_rays) && (cb == 1 || cb == sp->n_rays);
}

}  // namespace tfrt
