// The order in which an in-place trace and its reverse sweep hand their wavefronts out, shared by
// the kernel that makes it (k_wave_schedule, device) and by the CPU test harness in
// tests/wave_schedule_host (host).  No torch, no HIP types.
//
// No reference counterpart: the reference has no wavefronts.  The hardware starts the workgroups
// of a launch in index order, and a launch ends with its last wavefront.  With more wavefronts
// than the chip holds at once, the expensive ones should therefore start first and the cheap ones
// last (list scheduling by longest processing time).  What a wavefront will cost is taken from
// what it cost in an earlier trace of the same rays in the same order: the count rows that
// k_trace_inplace leaves (InplaceTape.wcount).
//
// The schedule is a permutation sched[0 .. G) of the G = ceil(N / 64) GROUPS of 64 consecutive
// rays: the workgroup with index b of the reverse sweep (64 rays per wavefront) takes group
// sched[b].  A trace whose wavefronts hold 32 rays has `per` = 2 wavefronts to a group, and its
// workgroup b takes wavefront sched[b / per] * per + b % per.  Groups are listed by cost class,
// the heaviest class first, in ascending index inside a class: the stable order keeps neighbours
// on the rays' space-filling curve neighbours in time, for the scene's cache lines.  Equal costs
// throughout give the identity.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef TFRT_HD
#if defined(__HIPCC__)
#define TFRT_HD __host__ __device__ __forceinline__
#else
#define TFRT_HD inline
#endif
#endif

namespace tfrt {

// Cost classes.  Few: inside a class the order is the rays' own, and the end of the launch only
// needs the long wavefronts gone early, not a full sort.  Measured on the 1M-ray step, medians of
// five runs (profiles/r07_schedule_bench_runs.txt): index order 0.2393 ms, 4 classes 0.2331,
// 8 classes 0.2305, 16 classes 0.2284.
#ifndef TFRT_WAVE_SCHED_CLASSES   // (tuning builds set it: scratch/build_variants.py; at most 16)
#define TFRT_WAVE_SCHED_CLASSES 16
#endif
constexpr int WAVE_SCHED_CLASSES = TFRT_WAVE_SCHED_CLASSES;
static_assert(WAVE_SCHED_CLASSES >= 1 && WAVE_SCHED_CLASSES <= 16, "cost classes");

// A wavefront's cost in hundredths of a microsecond, from the lives recorded per faces screened
// (profiles/r04_wave_timeline.txt: 11.7 / 14.7 / 16.2 / 19.6 / 23.8 us for <= 4 / 8 / 16 / 32 / 64
// faces, one pass): ~10.5 us per pass entered and ~0.45 us per candidate face tested against the
// bundle.  Only the ORDER of the costs matters; nothing reads them as times.
constexpr uint32_t WAVE_COST_PASS = 1050;
constexpr uint32_t WAVE_COST_FACE = 45;
// (saturation: the sum stays inside 32 bits whatever the rows hold)
constexpr uint32_t WAVE_COST_MAX_PASSES = 1u << 16;
constexpr uint32_t WAVE_COST_MAX_FACES = 1u << 24;

TFRT_HD uint32_t wave_cost(uint32_t passes, uint32_t faces) {
  if (passes > WAVE_COST_MAX_PASSES) passes = WAVE_COST_MAX_PASSES;
  if (faces > WAVE_COST_MAX_FACES) faces = WAVE_COST_MAX_FACES;
  return WAVE_COST_PASS * passes + WAVE_COST_FACE * faces;
}

// The cost of group g from the count rows of a trace of P passes: wcount[p * wstride + w], rows
// 0 .. P-1 the class counts of wavefront w in pass p (non-zero: it entered that pass), row P + 1
// the candidate faces it tested.  A group of `per` wavefronts: the passes of the one that went
// furthest, the faces of all.
TFRT_HD uint32_t wave_group_cost(const uint32_t* wcount, size_t wstride, int P, int nwaves, int per,
                                 int g) {
  uint32_t passes = 0, faces = 0;
  for (int k = 0; k < per; ++k) {
    const int w = g * per + k;
    if (w >= nwaves) break;
    uint32_t entered = 0;
    for (int p = 0; p < P; ++p) entered += wcount[(size_t)p * wstride + w] != 0u ? 1u : 0u;
    if (entered > passes) passes = entered;
    const uint32_t f = wcount[(size_t)(P + 1) * wstride + w];
    faces += f > WAVE_COST_MAX_FACES - faces ? WAVE_COST_MAX_FACES - faces : f;
  }
  return wave_cost(passes, faces);
}

// Class of a cost, linear between the launch's cheapest (class 0) and dearest group.
TFRT_HD int wave_class(uint32_t cost, uint32_t cmin, uint32_t cmax) {
  const uint64_t span = (uint64_t)(cmax - cmin) + 1u;
  return (int)((uint64_t)(cost - cmin) * (uint64_t)WAVE_SCHED_CLASSES / span);
}

// The schedule, serially: the definition k_wave_schedule restates in parallel.  `sched` has
// ceil(nwaves / per) entries.
inline void wave_schedule_serial(const uint32_t* wcount, size_t wstride, int P, int nwaves, int per,
                                 int32_t* sched) {
  const int G = (nwaves + per - 1) / per;
  uint32_t cmin = 0xFFFFFFFFu, cmax = 0u;
  for (int g = 0; g < G; ++g) {
    const uint32_t c = wave_group_cost(wcount, wstride, P, nwaves, per, g);
    if (c < cmin) cmin = c;
    if (c > cmax) cmax = c;
  }
  int at = 0;
  for (int cls = WAVE_SCHED_CLASSES - 1; cls >= 0; --cls)
    for (int g = 0; g < G; ++g)
      if (wave_class(wave_group_cost(wcount, wstride, P, nwaves, per, g), cmin, cmax) == cls)
        sched[at++] = g;
}

}  // namespace tfrt
