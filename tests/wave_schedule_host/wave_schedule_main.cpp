// Stand-alone check of csrc/wave_schedule.h (host compile; built with the address and
// undefined-behaviour sanitizers by tests/test_wave_schedule_host.py).  Every case makes count
// rows as k_trace_inplace leaves them, builds the schedule with wave_schedule_serial and checks
// the definition: a permutation of the groups, classes never rising along it, ascending indices
// inside a class -- and, independently, that it is std::stable_sort by descending class.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "wave_schedule.h"

using namespace tfrt;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAILED %s: ", #cond);         \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      ++failures;                                \
    }                                            \
  } while (0)

struct Rows {
  int P, nwaves, per;
  size_t wstride;
  std::vector<uint32_t> w;   // (P + 2) x wstride, the padding poisoned
  Rows(int P_, int nwaves_, int per_)
      : P(P_), nwaves(nwaves_), per(per_), wstride(((size_t)nwaves_ + 63) / 64 * 64),
        w((size_t)(P_ + 2) * wstride, 0xDEADBEEFu) {
    for (int p = 0; p < P + 2; ++p)
      for (int k = 0; k < nwaves; ++k) at(p, k) = 0u;
  }
  uint32_t& at(int p, int k) { return w[(size_t)p * wstride + k]; }
  int groups() const { return (nwaves + per - 1) / per; }
};

// the schedule of `r`, checked against the definition; returns it
static std::vector<int32_t> checked(const Rows& r, const char* what) {
  const int G = r.groups();
  std::vector<int32_t> sched((size_t)G, -1);
  wave_schedule_serial(r.w.data(), r.wstride, r.P, r.nwaves, r.per, sched.data());
  std::vector<uint32_t> cost((size_t)G);
  for (int g = 0; g < G; ++g) cost[g] = wave_group_cost(r.w.data(), r.wstride, r.P, r.nwaves, r.per, g);
  const uint32_t cmin = *std::min_element(cost.begin(), cost.end());
  const uint32_t cmax = *std::max_element(cost.begin(), cost.end());
  std::vector<int> cls((size_t)G);
  for (int g = 0; g < G; ++g) {
    cls[g] = wave_class(cost[g], cmin, cmax);
    CHECK(cls[g] >= 0 && cls[g] < WAVE_SCHED_CLASSES, "%s: class %d of group %d", what, cls[g], g);
  }
  std::vector<int> seen((size_t)G, 0);
  for (int k = 0; k < G; ++k) {
    const int g = sched[k];
    CHECK(g >= 0 && g < G, "%s: entry %d is %d", what, k, g);
    if (g < 0 || g >= G) return sched;
    ++seen[g];
  }
  for (int g = 0; g < G; ++g) CHECK(seen[g] == 1, "%s: group %d listed %d times", what, g, seen[g]);
  for (int k = 1; k < G; ++k) {
    const int a = sched[k - 1], b = sched[k];
    CHECK(cls[a] >= cls[b], "%s: class rises at %d", what, k);
    CHECK(cls[a] != cls[b] || a < b, "%s: not stable at %d", what, k);
  }
  if (cmax > cmin) {
    const int top = (int)(std::max_element(cost.begin(), cost.end()) - cost.begin());
    CHECK(cls[top] == WAVE_SCHED_CLASSES - 1, "%s: the dearest group is in class %d", what, cls[top]);
    CHECK(cls[sched[0]] == WAVE_SCHED_CLASSES - 1, "%s: the first entry is in class %d", what, cls[sched[0]]);
  }
  std::vector<int32_t> want((size_t)G);
  std::iota(want.begin(), want.end(), 0);
  std::stable_sort(want.begin(), want.end(), [&](int a, int b) { return cls[a] > cls[b]; });
  CHECK(want == sched, "%s: differs from a stable sort by descending class", what);
  return sched;
}

static bool identity(const std::vector<int32_t>& s) {
  for (size_t k = 0; k < s.size(); ++k)
    if (s[k] != (int32_t)k) return false;
  return true;
}

static void random_rows(Rows& r, std::mt19937& rng) {
  std::uniform_int_distribution<int> passes(1, r.P), faces(0, 64), byte(1, 64);
  for (int k = 0; k < r.nwaves; ++k) {
    const int entered = passes(rng);
    for (int p = 0; p < entered; ++p) r.at(p, k) = (uint32_t)byte(rng) << (8 * (p % 4));
    r.at(r.P + 1, k) = (uint32_t)(faces(rng) * entered);
    r.at(r.P, k) = r.at(r.P + 1, k) * 40u;   // (pairs: not part of the cost)
  }
}

int main() {
  std::mt19937 rng(7);
  const int sizes[] = {1, 63, 64, 65, 15625};
  for (int n : sizes)
    for (int per = 1; per <= 2; ++per) {
      char what[64];
      // random work rows
      Rows r(3, n, per);
      random_rows(r, rng);
      std::snprintf(what, sizeof what, "random, %d wavefronts, %d per group", n, per);
      checked(r, what);
      // all costs equal: the identity
      Rows e(3, n, per);
      for (int k = 0; k < n; ++k) {
        e.at(0, k) = 64u;
        e.at(1, k) = 64u << 8;
        e.at(4, k) = 7u;
      }
      if (per == 2 && n % 2 == 1) e.at(4, n - 1) = 14u, e.at(0, n - 1) = 1u;   // (a last group of one)
      std::snprintf(what, sizeof what, "equal costs, %d wavefronts, %d per group", n, per);
      CHECK(identity(checked(e, what)), "%s: not the identity", what);
      // work rows all zero (no trace has run): the identity
      Rows z(3, n, per);
      std::snprintf(what, sizeof what, "zero rows, %d wavefronts, %d per group", n, per);
      CHECK(identity(checked(z, what)), "%s: not the identity", what);
      // one outlier: it goes first, everybody else keeps the order they had
      Rows o(3, n, per);
      random_rows(o, rng);
      const int out = n / 2;
      o.at(o.P + 1, out) = 0xFFFFFFFFu;   // (saturates)
      std::snprintf(what, sizeof what, "one outlier, %d wavefronts, %d per group", n, per);
      const std::vector<int32_t> s = checked(o, what);
      CHECK(s[0] == out / per, "%s: the outlier's group is at %d", what,
            (int)(std::find(s.begin(), s.end(), out / per) - s.begin()));
      for (size_t k = 2; k < s.size(); ++k) CHECK(s[k - 1] < s[k], "%s: the rest is reordered at %zu", what, k);
    }
  // the cost follows the recorded lives: more faces or more passes cost more
  CHECK(wave_cost(1, 4) < wave_cost(1, 64) && wave_cost(1, 64) < wave_cost(2, 64), "cost order");
  CHECK(wave_cost(0xFFFFFFFFu, 0xFFFFFFFFu) >= wave_cost(1u << 16, 1u << 24), "cost saturates");
  CHECK(wave_class(5, 5, 5) == 0 && wave_class(0xFFFFFFFFu, 0, 0xFFFFFFFFu) == WAVE_SCHED_CLASSES - 1,
        "class ends");
  if (failures == 0) std::printf("wave_schedule.h: all checks passed\n");
  return failures == 0 ? 0 : 1;
}
