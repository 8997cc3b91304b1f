// csrc/centroid_math.h on the host (tests/test_centroid_error_host.py compiles this with g++ and
// the address and undefined-behaviour sanitizers): reads a record table and the targets, or the
// parent labels, and writes what centroid_math.h makes of them -- every group's weight and
// centroid, the parents' records (the integer sums of their groups') and centroids, the residual
// table and every group's error terms.  The float sums over the groups are the caller's (the
// numpy reference's): this program checks the per-group arithmetic, not an order of summation.
//
//   centroid_main <in> <out>
//
// in:  int64 G, k, P (0: targets mode) | f64 x0, qsx, y0, qsy | int64 acc[G][4] |
//      P == 0: f64 targets[G][k];  P > 0: int32 parents[G]
// out: f64 group[G][3] {w, cx, cy} | f64 residual[G][2] | f64 error_terms[G][2] | f64 used[G] |
//      int64 parent_acc[P][4] | f64 parent[P][3] {w, Cx, Cy}
//      (a group or parent without rays: zeros, and NaN in `residual`)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "centroid_math.h"

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
    fprintf(stderr, "usage: centroid_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(3);
  std::vector<double> consts(4);
  if (!get(in, head) || !get(in, consts)) return 3;
  const int64_t G = head[0], k = head[1], P = head[2];
  if (G < 1 || (k != 1 && k != 2) || P < 0 || P > (1 << 20)) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  std::vector<int64_t> acc(4 * G);
  std::vector<double> targets(P == 0 ? k * G : 0);
  std::vector<int32_t> parents(P > 0 ? G : 0);
  if (!get(in, acc) || !get(in, targets) || !get(in, parents)) return 3;
  fclose(in);
  tfrt::CentroidGrid grid;
  grid.x0 = consts[0], grid.qsx = consts[1], grid.y0 = consts[2], grid.qsy = consts[3];
  grid.two = k == 2;

  // the parents' records: what k_centroid_parents adds, group by group
  std::vector<int64_t> parent_acc(4 * P, 0);
  for (int64_t g = 0; g < G && P > 0; ++g) {
    if (acc[4 * g] <= 0 || !tfrt::centroid_parent_ok(parents[g], (int32_t)P)) continue;
    for (int s = 0; s < 3; ++s) parent_acc[4 * (int64_t)parents[g] + s] += acc[4 * g + s];
  }
  std::vector<double> parent(3 * P, 0.0);
  for (int64_t p = 0; p < P; ++p) {
    const tfrt::CentroidRecord Q = tfrt::centroid_record(&parent_acc[4 * p], grid);
    parent[3 * p] = Q.w, parent[3 * p + 1] = Q.cx, parent[3 * p + 2] = Q.cy;
  }

  std::vector<double> group(3 * G, 0.0), residual(2 * G), error_terms(2 * G, 0.0), used(G, 0.0);
  for (int64_t g = 0; g < G; ++g) {
    const tfrt::CentroidRecord q = tfrt::centroid_record(&acc[4 * g], grid);
    group[3 * g] = q.w, group[3 * g + 1] = q.cx, group[3 * g + 2] = q.cy;
    double t[2] = {0.0, 0.0};
    bool has = false;
    if (q.rays) {
      if (P == 0) {
        has = tfrt::centroid_target(&targets[k * g], grid.two, t);
      } else if (tfrt::centroid_parent_ok(parents[g], (int32_t)P)) {
        const tfrt::CentroidRecord Q = tfrt::centroid_record(&parent_acc[4 * (int64_t)parents[g]],
                                                             grid);
        has = Q.rays;
        t[0] = Q.cx, t[1] = Q.cy;
      }
    }
    used[g] = tfrt::centroid_residual(q, has, t, &residual[2 * g], &error_terms[2 * g]) ? 1.0 : 0.0;
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, group) || !put(out, residual) || !put(out, error_terms) ||
      !put(out, used) || !put(out, parent_acc) || !put(out, parent) || fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("groups %lld fields %lld parents %lld\n", (long long)G, (long long)k, (long long)P);
  return 0;
}
