// The per-group arithmetic of CentroidError (tfrt_centroid.hip; the definition, operation by
// operation, is in include/tfrt_hip.h at tfrt_centroid_error): the centroid of a record -- a
// group's, or a parent's, which is the integer sum of its groups' records --, whether a row of
// `targets` pins its group, and a group's residual against its target with the terms it adds to the
// error.  Float64 and int64 only, every operation rounded on its own.  Compiles for the host as
// well (the convention of distortion_math.h), so that tests/centroid_host checks it without a GPU.
//
// One field: the y components of every centroid and target are 0.0 and the same expressions run.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

constexpr int CENTROID_USED_OUT = 2;     // {groups_used, parents_used}

// The domain constants of the records (tfrt_spot_error's), `two`: a second field.
struct CentroidGrid {
  double x0, qsx, y0, qsy;
  bool two;
};

// A record {count, Sx, Sy, 0} with rays (count > 0): its weight w = (double) count and its centroid
// c, as tfrt_spot_error computes it.  Without rays: w = 0.0, c = 0.0.
struct CentroidRecord {
  bool rays;
  double w, cx, cy;
};

TFRT_HD CentroidRecord centroid_record(const int64_t* rec, const CentroidGrid& g) {
#pragma clang fp contract(off)
  CentroidRecord q;
  q.rays = rec[0] > 0;
  q.w = q.cx = q.cy = 0.0;
  if (q.rays) {
    q.w = (double)rec[0];
    q.cx = g.x0 + ((double)rec[1] / q.w) / g.qsx;
    if (g.two) q.cy = g.y0 + ((double)rec[2] / q.w) / g.qsy;
  }
  return q;
}

// targets mode: the target t of a group from its row of `targets` (k f64); false -- the group is
// not pinned -- if an entry of the row is not finite.
TFRT_HD bool centroid_target(const double* row, bool two, double* t) {
  t[0] = row[0];
  t[1] = two ? row[1] : 0.0;
  return std::isfinite(t[0]) && std::isfinite(t[1]);
}

// parents mode: is the parent label legal?
TFRT_HD bool centroid_parent_ok(int32_t parent, int32_t n_parents) {
  return parent >= 0 && parent < n_parents;
}

// The residual of a group: r = c - t for a USED group (it has rays and a target), which adds
// w (rx rx) to e[0] and w (ry ry) to e[1]; 0.0 for a group with rays and no target; NaN for a group
// without rays.  Returns whether the group is used.
TFRT_HD bool centroid_residual(const CentroidRecord& q, bool has_target, const double* t,
                               double* r, double* e) {
#pragma clang fp contract(off)
  if (!q.rays) {
    r[0] = r[1] = __builtin_nan("");
    return false;
  }
  r[0] = r[1] = 0.0;
  if (!has_target) return false;
  r[0] = q.cx - t[0];
  r[1] = q.cy - t[1];
  e[0] += q.w * (r[0] * r[0]);
  e[1] += q.w * (r[1] * r[1]);
  return true;
}

}  // namespace tfrt
