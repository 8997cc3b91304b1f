// The seed launch of the errors that charge a GROUP'S CENTROID, shared by the files that launch it
// (tfrt_distortion.hip and tfrt_centroid.hip): one lane per column, the classification of
// spot_records.h, one 16-byte load of the residual of the ray's own group from a (G, 2) table, and
// the gradient rows of EVERY column.  What the table holds is the caller's business
// (DistortionError: c - (A p + t); CentroidError: c - target).  A template only, so that each file
// that launches it carries its own instantiations (as k_spot_accumulate of spot_records.h).
#pragma once
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"
#include "spot_records.h"

namespace tfrt {

constexpr int DISTORTION_SEED_MAX_GRID = 2048;   // workgroups of the seed launch

// The gradient rows of every column: 2 r of the ray's own group for a ray inside, the penalty's
// derivative for one outside (tfrt_spot_error's), zeros for the rest.
template <typename T, int DIM>
__global__ __launch_bounds__(BLOCK) void k_distortion_seed(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotArgs<false> g,
    const double2* __restrict__ residual, double* __restrict__ grad, int64_t grad_stride) {
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
      // (this ray is in its own group's record: the group is used, its residual is a number)
      const double2 res = residual[r.label];
      gx = 2.0 * res.x;
      gy = 2.0 * res.y;
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

}  // namespace tfrt
