// csrc/distortion_math.h on the host (tests/test_distortion_error_host.py compiles this with g++
// and the address and undefined-behaviour sanitizers): reads a record table and the object points
// and writes what distortion_math.h makes of them -- every group's weight, point and centroid,
// its terms of the two fit passes, the fit from the sums the caller hands in, and the residual
// table with every group's error terms.  The sums over the groups are the caller's (the numpy
// reference's): this program checks the per-group arithmetic, not an order of summation.
//
//   distortion_main <in> <out>
//
// in:  int64 G, k, fit_kind, used | f64 x0, qsx, y0, qsy, min_cond | f64 means[4] {pmx, pmy, cmx,
//      cmy} | f64 S[7] | int64 acc[G][4] | f64 points[G][k]
// out: f64 group[G][5] {w, px, py, cx, cy} | f64 mean_terms[G][5] | f64 moment_terms[G][7] |
//      f64 fit[8] | f64 residual[G][2] | f64 error_terms[G][2]
//      (an unused group: zeros, and NaN in `residual`)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "distortion_math.h"

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
    fprintf(stderr, "usage: distortion_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(4);
  std::vector<double> consts(5), means(4), S(tfrt::DISTORTION_MOMENT_SUMS);
  if (!get(in, head) || !get(in, consts) || !get(in, means) || !get(in, S)) return 3;
  const int64_t G = head[0], k = head[1], fit_kind = head[2], used = head[3];
  if (G < 1 || (k != 1 && k != 2) || (fit_kind != 0 && fit_kind != 1) || used < 0 || used > G) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  std::vector<int64_t> acc(4 * G);
  std::vector<double> points(k * G);
  if (!get(in, acc) || !get(in, points)) return 3;
  fclose(in);
  tfrt::DistortionGrid grid;
  grid.x0 = consts[0], grid.qsx = consts[1], grid.y0 = consts[2], grid.qsy = consts[3];
  grid.two = k == 2;

  std::vector<double> group(5 * G, 0.0), mean_terms(tfrt::DISTORTION_MEAN_SUMS * G, 0.0);
  std::vector<double> moment_terms(tfrt::DISTORTION_MOMENT_SUMS * G, 0.0);
  std::vector<double> fit(tfrt::DISTORTION_FIT_OUT), residual(2 * G), error_terms(2 * G, 0.0);
  const bool valid = tfrt::distortion_fit(S.data(), means.data(), (long long)used, (int)fit_kind,
                                          grid.two, consts[4], fit.data());
  for (int64_t g = 0; g < G; ++g) {
    const tfrt::DistortionGroup q = tfrt::distortion_group(&acc[4 * g], &points[k * g], grid);
    if (q.used) {
      double* at = &group[5 * g];
      at[0] = q.w, at[1] = q.px, at[2] = q.py, at[3] = q.cx, at[4] = q.cy;
      tfrt::distortion_mean_terms(q, &mean_terms[tfrt::DISTORTION_MEAN_SUMS * g]);
      tfrt::distortion_moment_terms(q, means.data(),
                                    &moment_terms[tfrt::DISTORTION_MOMENT_SUMS * g]);
    }
    tfrt::distortion_residual(q, means.data(), fit.data(), valid, &residual[2 * g],
                              &error_terms[2 * g]);
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, group) || !put(out, mean_terms) || !put(out, moment_terms) ||
      !put(out, fit) || !put(out, residual) || !put(out, error_terms) || fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("groups %lld fields %lld valid %d\n", (long long)G, (long long)k, valid ? 1 : 0);
  return 0;
}
