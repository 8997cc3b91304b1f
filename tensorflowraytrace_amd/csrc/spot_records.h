// The group records of SpotError, shared by the files that fill them (tfrt_spot.hip,
// tfrt_distortion.hip and tfrt_centroid.hip): the constants of a launch, the layout of a record,
// the classification of a column and the accumulate launch -- {1, qx, qy} (weighted: the limbs)
// into the record of the ray's group, the out-of-domain penalty and the number of counting columns
// as one partial per workgroup.  The definition is in include/tfrt_hip.h at tfrt_spot_error; the launches are
// described at the top of tfrt_spot.hip.  Templates only, so that each file that launches them
// carries its own instantiations (as k_error_clear of error_sums.h).
#pragma once
#include "tfrt_common.h"
#include "direction_fields.h"
#include "error_sums.h"

namespace tfrt {

constexpr int SPOT_LDS_GROUPS = 1024;      // 3 planes of int64: 24 KiB per workgroup
constexpr int SPOT_WEIGHTED_LDS_GROUPS = 512;   // weighted, 6 planes of int64: 24 KiB
constexpr int SPOT_MAX_WBITS = 20;
constexpr int SPOT_MAX_GROUPS = 1 << 20;
constexpr int SPOT_MAX_GRID = 512;         // workgroups of the accumulate launch
constexpr int SPOT_RAYS_PER_BLOCK = 4 * BLOCK;
constexpr int SPOT_SEED_MAX_GRID = 8192;   // workgroups of the seed launch
constexpr int FINISH_BLOCK = 1024;
constexpr int FINISH_WAVES = FINISH_BLOCK / 64;

struct SpotGrid {
  double x0, x1, qsx, y0, y1, qsy, oob, qmax;
  int64_t n_source;
  int32_t n_groups, row_x, row_y;   // row_x, row_y: field codes (direction_fields.h)
};

// The weights of tfrt_spot_error_weighted: one f64 in [0, 1] per SOURCE ray.
struct SpotWeights {
  const double* weight;
  double one, inv;           // 2^wbits, 2^-wbits
  int32_t h;                 // qbits / 2: the low limb's bits
};

// The constants of an accumulate or seed launch: the grid, then (WEIGHTED) the weights.
template <bool WEIGHTED>
struct SpotArgs : SpotGrid, weights_base<WEIGHTED, SpotWeights> {
  static constexpr bool weighted = WEIGHTED;
};

// The record of a group: SLOTS int64 in global memory, of which the first PLANES are in use --
// {count, Sx, Sy, 0}, or WEIGHTED one 64-byte line {W, Xhi, Xlo, Yhi, Ylo, count, 0, 0} with the
// moments W * x in two limbs.  The table in LDS keeps the slots in use as planes of G int64 each, in
// the record's order (consecutive labels in consecutive banks).
template <bool WEIGHTED>
struct SpotRecord {
  static constexpr int PLANES = WEIGHTED ? 6 : 3;
  static constexpr int SLOTS = WEIGHTED ? 8 : 4;

  // slot p of group `label`: in the LDS table of G groups (LDS), else in the records `acc`
  template <bool LDS>
  static __device__ __forceinline__ unsigned long long* slot(unsigned long long* table,
                                                             unsigned long long* acc, int G,
                                                             int label, int p) {
    if (LDS) return table + (p * G + label);
    return acc + SLOTS * (int64_t)label + p;
  }

  // the sum over the group's rays of (weight x) coordinate `axis` (0: x, 1: y), as a double: what
  // the centroid divides by the mass in slot 0
  static __device__ __forceinline__ double moment(const long long* rec, int axis,
                                                  const SpotArgs<WEIGHTED>& g) {
#pragma clang fp contract(off)
    if constexpr (WEIGHTED)
      return ldexp((double)rec[1 + 2 * axis], g.h) + (double)rec[2 + 2 * axis];
    else
      return (double)rec[1 + axis];
  }
};

// What one column does.  kind 0: masked off; 3: counts, but contributes nothing (a non-finite
// coordinate, or no spot); 1: inside the closed domain; 2: outside, ex / ey and their signs.
struct SpotRay {
  int kind;
  int label;
  double x, y;       // kind 1: the coordinates; kind 2: ex, ey
  double dx, dy;     // kind 2: d ex / d x, d ey / d y (-1, 0, +1)
};

// WEIGHTED: `wq` = rint(w * 2^wbits) and `wr` = wq * 2^-wbits receive the weight of the column's
// source ray (they are left alone without), and a column with a spot (kinds 1 and 2) whose weight
// does not count or quantises to 0 is in no spot (kind 3 -- every "no spot" case ends alike, so
// the order of the checks does not show).  The weight is read behind the index check that the label
// lookup needs anyway; the read of perm is the one that served the label.
template <typename T, int DIM, bool WEIGHTED>
__device__ __forceinline__ SpotRay spot_classify(const T* __restrict__ rows, int64_t stride,
                                                 const int32_t* __restrict__ mask,
                                                 const int32_t* __restrict__ group,
                                                 const int32_t* __restrict__ perm, int64_t i,
                                                 const SpotArgs<WEIGHTED>& g, LinkDir<DIM>& link,
                                                 double& wq, double& wr) {
#pragma clang fp contract(off)
  SpotRay r;
  r.kind = 0;
  r.label = 0;
  r.x = r.y = r.dx = r.dy = 0.0;
  if (mask == nullptr || mask[i] >= 0) {
    r.kind = 3;
    const bool two = g.row_y >= 0;
    double x, y;
    read_fields<T, DIM>(rows, stride, i, g.row_x, g.row_y, x, y, link);
    if (isfinite(x) && isfinite(y)) {
      // (nothing is read out of bounds, whatever perm and group hold)
      const int64_t s = perm != nullptr ? (int64_t)perm[i] : i;
      if (s >= 0 && s < g.n_source) {
        const int label = group[s];
        if (label >= 0 && label < g.n_groups) {
          r.label = label;
          const bool out = x < g.x0 || x > g.x1 || (two && (y < g.y0 || y > g.y1));
          if (out) {
            r.kind = 2;
            r.x = outside_by(x, g.x0, g.x1), r.dx = outside_sign(x, g.x0, g.x1);
            if (two) r.y = outside_by(y, g.y0, g.y1), r.dy = outside_sign(y, g.y0, g.y1);
          } else {
            r.kind = 1;
            r.x = x;
            r.y = y;
          }
        }
      }
    }
  }
  if constexpr (WEIGHTED) {
    wq = wr = 0.0;
    if (r.kind == 1 || r.kind == 2) {
      const int64_t s = perm != nullptr ? (int64_t)perm[i] : i;
      // (a NaN fails both comparisons; the product with a power of two is exact)
      const double w = g.weight[s];
      wq = w >= 0.0 && w <= 1.0 ? rint(w * g.one) : 0.0;
      wr = wq * g.inv;
      if (wq == 0.0) r.kind = 3;
    }
  }
  return r;
}

__device__ __forceinline__ unsigned long long spot_fixed(double v, double lo, double qs,
                                                         double qmax) {
#pragma clang fp contract(off)
  // round half to even (v_rndne_f64); the clamp keeps the closed domain inside [0, 2^qbits]
  return (unsigned long long)(long long)fmin(fmax(rint((v - lo) * qs), 0.0), qmax);
}

// {1, qx, qy} -> the record of the ray's group; WEIGHTED: {wq, wq * qx in two limbs, wq * qy in two
// limbs, 1}, the penalty times wr last.
template <typename T, bool LDS, int DIM, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void k_spot_accumulate(
    const T* __restrict__ rows, int64_t stride, int64_t n, const int32_t* __restrict__ mask,
    const int32_t* __restrict__ group, const int32_t* __restrict__ perm, SpotArgs<WEIGHTED> g,
    unsigned long long* __restrict__ acc, double* __restrict__ pen_partial,
    long long* __restrict__ cnt_partial) {
#pragma clang fp contract(off)
  using Record = SpotRecord<WEIGHTED>;
  extern __shared__ unsigned long long table[];   // LDS variant: Record::PLANES planes of G each
  __shared__ double wsum[WAVES];
  __shared__ long long wcnt[WAVES];
  const int G = g.n_groups;
  const bool two = g.row_y >= 0;
  unsigned long long low = 0ull;   // WEIGHTED: the low limb's mask
  if constexpr (WEIGHTED) low = (1ull << g.h) - 1ull;
  if (LDS) {
    for (int e = threadIdx.x; e < Record::PLANES * G; e += BLOCK) table[e] = 0ull;
    __syncthreads();
  }
  double pen = 0.0;
  long long counting = 0;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * BLOCK) {
    LinkDir<DIM> link;
    double wq = 0.0, wr = 0.0;
    const SpotRay r =
        spot_classify<T, DIM, WEIGHTED>(rows, stride, mask, group, perm, i, g, link, wq, wr);
    counting += r.kind != 0 ? 1 : 0;
    if (r.kind == 2) {
      pen += weighed<WEIGHTED>(g.oob * (r.x * r.x + r.y * r.y), wr);
    } else if (r.kind == 1) {
      // (the weight as an integer: what a WEIGHTED record sums in the place of 1)
      const unsigned long long q = WEIGHTED ? (unsigned long long)(long long)wq : 1ull;
      const unsigned long long qx = spot_fixed(r.x, g.x0, g.qsx, g.qmax);
      const unsigned long long qy = two ? spot_fixed(r.y, g.y0, g.qsy, g.qmax) : 0ull;
      if constexpr (WEIGHTED) {
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 0), q);
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 1), q * (qx >> g.h));
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 2), q * (qx & low));
        if (two) {
          atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 3), q * (qy >> g.h));
          atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 4), q * (qy & low));
        }
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 5), 1ull);
      } else {
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 0), q);
        atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 1), qx);
        if (two) atomicAdd(Record::template slot<LDS>(table, acc, G, r.label, 2), qy);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int e = threadIdx.x; e < Record::PLANES * G; e += BLOCK) {
      const unsigned long long v = table[e];
      const int plane = e / G, label = e - plane * G;
      if (v != 0ull) atomicAdd(Record::template slot<false>(table, acc, G, label, plane), v);
    }
  }
  const double s = error_block_sum<WAVES>(pen, wsum);
  const long long c = error_block_sum<WAVES>(counting, wcnt);
  if (threadIdx.x == 0) {
    pen_partial[blockIdx.x] = s;
    cnt_partial[blockIdx.x] = c;
  }
}

}  // namespace tfrt
