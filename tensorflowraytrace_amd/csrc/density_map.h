// The map of TFRT_PTS_DENSITY: a uniform point of a rectangle onto a point that follows a 2-D
// density (ArbitraryDistribution.__call__, tfrt/distributions.py:2123-2280): an x quantile curve,
// the x cell the result lands in, that cell's y quantile curve.  Float64 only.  Compiles for the
// host as well (the convention of trace_math.h), so that tests/density_map checks it without a GPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif

namespace tfrt {

// scipy's linear interp1d over the m >= 2 knots (xs, ys), xs non-decreasing:
// k = clamp(lower_bound(xs, v), 1, m - 1), the line through knots k - 1 and k.  Equal neighbours
// (a stretch of zero density) are never divided by for v inside the table: the lower bound is the
// FIRST knot >= v, so xs[k - 1] < v <= xs[k].  Reads xs[0 .. m - 1] only, whatever v is (a NaN
// takes k = 1).
TFRT_HD double density_interp(const double* xs, const double* ys, int m, double v) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xs[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int k = lo < 1 ? 1 : (lo > m - 1 ? m - 1 : lo);
  const double x0 = xs[k - 1], y0 = ys[k - 1];
  return (ys[k] - y0) / (xs[k] - x0) * (v - x0) + y0;
}

// (bx, by) in [x_min, x_max] x [y_min, y_max] (lim = {x_min, x_max, y_min, y_max}) through the
// packed tables of tfrt_points_program.density:
//   [Qx.xs (x_count + 1) | Qx.ys (x_count + 1) | x_count x (Qy.xs (y_count + 1) | Qy.ys (y_count + 1))]
// The reference visits the x cells with `for i in range(y_count)`: a sample whose cell is not in
// [0, min(x_count, y_count)) keeps y = 0.
TFRT_HD void density_map(const double* tables, int x_count, int y_count, const double lim[4],
                         double bx, double by, double* x, double* y) {
  const int mx = x_count + 1, my = y_count + 1;
  const double xo = density_interp(tables, tables + mx, mx, bx);
  const double cell = floor((xo - lim[0]) * (double)x_count / (lim[1] - lim[0]));
  double yo = 0.0;
  if (cell >= 0.0 && cell < (double)y_count && cell < (double)x_count) {
    const double* col = tables + 2 * mx + (int64_t)cell * (2 * my);
    yo = density_interp(col, col + my, my, by);
  }
  *x = xo;
  *y = yo;
}

}  // namespace tfrt
