// What the errors that splat rays onto a grid of bins share (tfrt_density.hip, tfrt_mixing.hip):
// the constants of a splat or seed launch, the classification of a column -- does not count,
// inside the closed domain with its bins and bilinear weights, outside with its distances -- and
// the fixed point a weight enters its bin with.  The definition is in include/tfrt_hip.h at
// tfrt_density_error (weighted: tfrt_density_error_weighted); the launches are described at the
// top of tfrt_density.hip.  Device inlines and templates only, so that each file that launches
// kernels on them carries its own instantiations (as spot_records.h and residual_seed.h).
#pragma once
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"

namespace tfrt {

constexpr int DENSITY_LDS_BINS = 4096;   // 32 KiB of int64 per workgroup
constexpr int DENSITY_MAX_BINS = 65536;
constexpr int DENSITY_MAX_GRID = 512;    // workgroups of the splat (two per CU of a 256-CU chip)
constexpr int DENSITY_RAYS_PER_BLOCK = 4 * BLOCK;

struct DensityGrid {
  double x0, x1, sx, y0, y1, sy, oob;
  int32_t nx, ny, row_x, row_y;   // row_x, row_y: field codes (direction_fields.h)
};

// The weights of tfrt_density_error_weighted: one f64 in [0, 1] per SOURCE ray; column i is
// source ray perm[i] (perm null: i).
struct DensityWeights {
  const double* weight;
  const int32_t* perm;
  int64_t n_source;
};

// The constants of a splat or seed launch: the grid, then (WEIGHTED) the weights.
template <bool WEIGHTED>
struct DensityArgs : DensityGrid, weights_base<WEIGHTED, DensityWeights> {
  static constexpr bool weighted = WEIGHTED;
};

// What one column does.  kind 0: does not count (masked, or a non-finite coordinate; WEIGHTED: or
// no weight that counts); 1: inside the closed domain, spread over (ja|jb, ia|ib) with tx, ty;
// 2: outside, ex / ey and their signs.
struct DensityRay {
  int kind;
  int ia, ib, ja, jb;
  double tx, ty;     // kind 1: the upper weights; kind 2: ex, ey
  double dx, dy;     // kind 2: d ex / d x, d ey / d y (-1, 0, +1)
};

__device__ __forceinline__ void density_axis(double v, double lo, double scale, int nb, int& a,
                                             int& b, double& t) {
#pragma clang fp contract(off)
  const double u = (v - lo) * scale - 0.5;
  const double f = floor(u);
  t = u - f;
  // (f lies in [-1, nb]: v is inside the closed domain)
  const int i0 = (int)f;
  a = min(max(i0, 0), nb - 1);
  b = min(max(i0 + 1, 0), nb - 1);
}

// WEIGHTED: `w` receives the weight of the column's source ray (it is left alone without), and a
// column that counts (kinds 1 and 2) without a source ray or with a weight outside [0, 1] does not
// count (kind 0 -- "does not count" ends alike wherever it is found, so the order of the checks
// does not show).  Nothing is read out of bounds, whatever perm holds.
template <typename T, int DIM, bool WEIGHTED>
__device__ __forceinline__ DensityRay density_classify(const T* __restrict__ rows, int64_t stride,
                                                       const int32_t* __restrict__ mask, int64_t i,
                                                       const DensityArgs<WEIGHTED>& g,
                                                       LinkDir<DIM>& link, double& w) {
#pragma clang fp contract(off)
  DensityRay r;
  r.kind = 0;
  r.ia = r.ib = r.ja = r.jb = 0;
  r.tx = r.ty = r.dx = r.dy = 0.0;
  if (mask == nullptr || mask[i] >= 0) {
    const bool two = g.row_y >= 0;
    double x, y;
    read_fields<T, DIM>(rows, stride, i, g.row_x, g.row_y, x, y, link);
    if (isfinite(x) && isfinite(y)) {
      const bool out = x < g.x0 || x > g.x1 || (two && (y < g.y0 || y > g.y1));
      if (out) {
        r.kind = 2;
        r.tx = outside_by(x, g.x0, g.x1), r.dx = outside_sign(x, g.x0, g.x1);
        if (two) r.ty = outside_by(y, g.y0, g.y1), r.dy = outside_sign(y, g.y0, g.y1);
      } else {
        r.kind = 1;
        density_axis(x, g.x0, g.sx, g.nx, r.ia, r.ib, r.tx);
        if (two) density_axis(y, g.y0, g.sy, g.ny, r.ja, r.jb, r.ty);
      }
    }
  }
  if constexpr (WEIGHTED) {
    w = 0.0;
    if (r.kind != 0) {
      const int64_t s = g.perm != nullptr ? (int64_t)g.perm[i] : i;
      const bool has = s >= 0 && s < g.n_source;
      // (a NaN fails both comparisons)
      if (has) w = g.weight[s];
      if (!has || !(w >= 0.0 && w <= 1.0)) r.kind = 0;
    }
  }
  return r;
}

__device__ __forceinline__ unsigned long long density_fixed(double w) {
#pragma clang fp contract(off)
  // round half to even (v_rndne_f64); w in [0, 1], so the product is exact and at most 2^32
  return (unsigned long long)(long long)rint(w * 4294967296.0);
}

}  // namespace tfrt
