// csrc/mixing_math.h on the host (tests/test_mixing_error_host.py compiles this with g++ and the
// address and undefined-behaviour sanitizers): reads a histogram Hq[G][B] and the groups' sums of
// squared differences, forms the integer margins as the kernels do and writes what mixing_math.h
// makes of them -- every cell's squared difference and pull, every group's error and its term of
// E_mix.  The float sums over the bins and over the groups are the caller's (the numpy
// reference's): this program checks the per-cell and per-group arithmetic, not an order of
// summation.
//
//   mixing_main <in> <out>
//
// in:  int64 G, B | int64 hq[G][B] | f64 sums[G]  (the reference's sum over b of d * d per group)
// out: int64 nq[G] | int64 pq[B] | int64 Nq | f64 N, scale | f64 sq[G][B] | f64 pull[G][B] |
//      f64 e[G] | f64 term[G] | f64 used[G]
//      (a group without mass: sq, pull and term 0.0, e NaN)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mixing_math.h"

template <typename V>
static bool get(FILE* f, std::vector<V>& v) {
  return v.empty() || fread(v.data(), sizeof(V), v.size(), f) == v.size();
}
template <typename V>
static bool put(FILE* f, const std::vector<V>& v) {
  return v.empty() || fwrite(v.data(), sizeof(V), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mixing_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(2);
  if (!get(in, head)) return 3;
  const int64_t G = head[0], B = head[1];
  if (G < 1 || G > tfrt::MIXING_MAX_GROUPS || B < 1 || G * B > tfrt::MIXING_MAX_CELLS) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  std::vector<int64_t> hq(G * B);
  std::vector<double> sums(G);
  if (!get(in, hq) || !get(in, sums)) return 3;
  fclose(in);

  // the margins: what k_mixing_margins sums, and the pool's mass
  std::vector<int64_t> nq(G, 0), pq(B, 0), total(1, 0);
  for (int64_t g = 0; g < G; ++g)
    for (int64_t b = 0; b < B; ++b) {
      nq[g] += hq[g * B + b];
      pq[b] += hq[g * B + b];
    }
  for (int64_t g = 0; g < G; ++g) total[0] += nq[g];
  const tfrt::MixingPool pool = tfrt::mixing_pool(total[0], B);
  std::vector<double> consts = {pool.n, pool.scale};

  std::vector<double> sq(G * B, 0.0), pull(G * B, 0.0), e(G), term(G, 0.0), used(G, 0.0);
  for (int64_t g = 0; g < G; ++g) {
    const bool has = nq[g] > 0;
    used[g] = has ? 1.0 : 0.0;
    for (int64_t b = 0; b < B && has; ++b)
      sq[g * B + b] = tfrt::mixing_cell(hq[g * B + b], nq[g], pq[b], pool, &pull[g * B + b]);
    e[g] = tfrt::mixing_group_error(has, B, sums[g]);
    if (has) term[g] = tfrt::mixing_term(nq[g], pool, e[g]);
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, nq) || !put(out, pq) || !put(out, total) || !put(out, consts) ||
      !put(out, sq) || !put(out, pull) || !put(out, e) || !put(out, term) || !put(out, used) ||
      fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("groups %lld bins %lld\n", (long long)G, (long long)B);
  return 0;
}
