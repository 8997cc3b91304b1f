// Stand-alone check of next_up_f (csrc/trace_math.h; host compile, built and run by
// tests/test_next_up_host.py): equal to std::nextafterf(x, +infinity) bit for bit on the special
// values and on a million random bit patterns (NaNs and subnormals among them).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "trace_math.h"

static uint32_t bits_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}
static float float_of(uint32_t b) {
  float x;
  std::memcpy(&x, &b, 4);
  return x;
}

static int failures = 0;
static void check(uint32_t b) {
  const float x = float_of(b);
  const uint32_t want = bits_of(std::nextafterf(x, INFINITY)), got = bits_of(tfrt::next_up_f(x));
  if (want != got) {
    if (++failures <= 20) std::printf("FAILED %08x: nextafterf %08x, next_up_f %08x\n", b, want, got);
  }
}

int main() {
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX,
                           INFINITY, -INFINITY, NAN};
  for (float x : special) check(bits_of(x));
  // +-min subnormal, the largest subnormals, the floats next to +-1
  const uint32_t patterns[] = {0x00000001u, 0x80000001u, 0x007FFFFFu, 0x807FFFFFu,
                               0x3F7FFFFFu, 0xBF800001u, 0x7F7FFFFEu, 0xFF7FFFFFu};
  for (uint32_t b : patterns) check(b);
  std::mt19937 rng(20250117u);
  for (int k = 0; k < 1000000; ++k) check((uint32_t)rng());
  if (failures != 0) {
    std::printf("%d mismatches\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
