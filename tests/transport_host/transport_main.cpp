// csrc/transport_math.h on the host (tests/test_transport_error_host.py compiles this with g++
// and the address and undefined-behaviour sanitizers): reads a set of points, their validity and
// their ranks, writes every direction's projection, sort key and interpolated target.
//
//   transport_main <in> <out>
//
// in:  int64 n, K, Q, two | f64 x0, ix, y0, iy | f64 cs[K][2] | f64 tables[K][Q + 1] |
//      f64 x[n] | f64 y[n] | int32 valid[n] | int32 rank2[K][n] | int32 n_valid
// out: uint32 keys[K][n] | f64 p[K][n] | f64 t[K][n]   (p, t: 0 where a point is not valid)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "transport_math.h"

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
    fprintf(stderr, "usage: transport_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(4);
  std::vector<double> dom(4);
  if (!get(in, head) || !get(in, dom)) return 3;
  const int64_t n = head[0], K = head[1], Q = head[2];
  const bool two = head[3] != 0;
  if (n < 0 || K < 1 || K > tfrt::TRANSPORT_MAX_DIRECTIONS || Q < 2 ||
      Q > tfrt::TRANSPORT_MAX_KNOTS) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  std::vector<double> cs(2 * K), x(n), y(n);
  // (one exact-size allocation per table: a read past T[Q] is the sanitizer's to find)
  std::vector<std::vector<double>> tables(K, std::vector<double>(Q + 1));
  std::vector<int32_t> valid(n), rank2(K * n), nv(1);
  if (!get(in, cs)) return 3;
  for (auto& t : tables)
    if (!get(in, t)) return 3;
  if (!get(in, x) || !get(in, y) || !get(in, valid) || !get(in, rank2) || !get(in, nv)) return 3;
  fclose(in);

  std::vector<uint32_t> keys(K * n);
  std::vector<double> p(K * n, 0.0), t(K * n, 0.0);
  for (int64_t k = 0; k < K; ++k) {
    const tfrt::TransportDirection d =
        two ? tfrt::transport_direction(cs[2 * k], cs[2 * k + 1]) : tfrt::transport_direction(1.0, 0.0);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t at = k * n + i;
      keys[at] = tfrt::TRANSPORT_KEY_INVALID;
      if (!valid[i]) continue;
      const double xi = tfrt::transport_normalise(x[i], dom[0], dom[1]);
      const double eta = two ? tfrt::transport_normalise(y[i], dom[2], dom[3]) : 0.0;
      p[at] = two ? tfrt::transport_project(d.c, d.s, xi, eta) : xi;
      keys[at] = tfrt::transport_key(d, p[at]);
      t[at] = tfrt::transport_target(tables[k].data(), (int)Q, rank2[at], nv[0]);
    }
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, keys) || !put(out, p) || !put(out, t) || fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("points %lld directions %lld knots %lld\n", (long long)n, (long long)K, (long long)Q);
  return 0;
}
