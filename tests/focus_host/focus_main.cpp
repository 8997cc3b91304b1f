// csrc/focus_math.h on the host (tests/test_focus_error_host.py compiles this with g++ and the
// address and undefined-behaviour sanitizers): reads a set of lines (end point, direction, length),
// which of them count and their groups, and writes what focus_math.h makes of them -- the box
// test, the normalised end points, every ray's ten fixed-point slots, the groups' records, the
// solved table with its determinants, and every ray's term and gradient.
//
//   focus_main <in> <out>
//
// in:  int64 n, dim, G, pbits | f64 lo[3], hi[3], c[3], R, iR, min_det |
//      f64 e[dim][n] | f64 u[dim][n] | f64 L[n] | int32 counts[n] | int32 label[n]
// out: int32 inside[n] | f64 m[dim][n] | int64 q[n][10] | int64 acc[G][10] | f64 table[G][4] |
//      f64 det[G] | f64 term[n] | f64 g_start[dim][n] | f64 g_end[dim][n]
//      (m, q, term, g: 0 where a column does not count / has no term)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "focus_math.h"

template <typename V>
static bool get(FILE* f, std::vector<V>& v) {
  return v.empty() || fread(v.data(), sizeof(V), v.size(), f) == v.size();
}
template <typename V>
static bool put(FILE* f, const std::vector<V>& v) {
  return v.empty() || fwrite(v.data(), sizeof(V), v.size(), f) == v.size();
}

struct Data {
  int64_t n, G, pbits;
  tfrt::FocusBox box;
  double min_det;
  std::vector<double> e, u, L;
  std::vector<int32_t> counts, label;
  std::vector<int32_t> inside;
  std::vector<double> m, table, det, term, gs, ge;
  std::vector<int64_t> q, acc;
};

template <int DIM>
static void run(Data& d) {
  const int64_t n = d.n;
  const double one = ldexp(1.0, (int)d.pbits), inv = ldexp(1.0, -(int)d.pbits);
  for (int64_t i = 0; i < n; ++i) {
    double e[DIM], u[DIM], m[DIM];
    for (int a = 0; a < DIM; ++a) e[a] = d.e[a * n + i], u[a] = d.u[a * n + i];
    d.inside[i] = tfrt::focus_inside<DIM>(e, d.box) ? 1 : 0;
    if (!d.counts[i]) continue;
    tfrt::focus_normalise<DIM>(e, d.box, m);
    for (int a = 0; a < DIM; ++a) d.m[a * n + i] = m[a];
    int64_t* q = &d.q[tfrt::FOCUS_SLOTS * i];
    tfrt::focus_record<DIM>(u, m, one, q);
    for (int p = 0; p < tfrt::FOCUS_SLOTS; ++p) d.acc[tfrt::FOCUS_SLOTS * d.label[i] + p] += q[p];
  }
  std::vector<uint8_t> has(d.G);
  for (int64_t k = 0; k < d.G; ++k) {
    bool h;
    d.det[k] = tfrt::focus_solve<DIM>(&d.acc[tfrt::FOCUS_SLOTS * k], inv, d.min_det,
                                      &d.table[4 * k], h);
    d.table[4 * k + 3] = h ? 1.0 : 0.0;
    has[k] = h;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (!d.counts[i] || !has[d.label[i]]) continue;
    double u[DIM], m[DIM], gs[DIM], ge[DIM];
    for (int a = 0; a < DIM; ++a) u[a] = d.u[a * n + i], m[a] = d.m[a * n + i];
    d.term[i] = tfrt::focus_term<DIM>(u, m, &d.table[4 * d.label[i]], d.box.R, d.L[i], gs, ge);
    for (int a = 0; a < DIM; ++a) d.gs[a * n + i] = gs[a], d.ge[a * n + i] = ge[a];
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: focus_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(4);
  std::vector<double> box(12);
  if (!get(in, head) || !get(in, box)) return 3;
  Data d;
  d.n = head[0], d.G = head[2], d.pbits = head[3];
  const int64_t n = d.n, dim = head[1], G = d.G;
  if (n < 0 || (dim != 2 && dim != 3) || G < 1 || d.pbits < 1 ||
      d.pbits > tfrt::FOCUS_MAX_PBITS) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  for (int a = 0; a < 3; ++a) d.box.lo[a] = box[a], d.box.hi[a] = box[3 + a], d.box.c[a] = box[6 + a];
  d.box.R = box[9], d.box.iR = box[10], d.min_det = box[11];
  d.e.resize(dim * n), d.u.resize(dim * n), d.L.resize(n), d.counts.resize(n), d.label.resize(n);
  if (!get(in, d.e) || !get(in, d.u) || !get(in, d.L) || !get(in, d.counts) || !get(in, d.label))
    return 3;
  fclose(in);
  for (int64_t i = 0; i < n; ++i)
    if (d.counts[i] && (d.label[i] < 0 || d.label[i] >= G)) {
      fprintf(stderr, "a counting column without a group\n");
      return 3;
    }
  d.inside.assign(n, 0), d.m.assign(dim * n, 0.0), d.q.assign(tfrt::FOCUS_SLOTS * n, 0);
  d.acc.assign(tfrt::FOCUS_SLOTS * G, 0), d.table.assign(4 * G, 0.0), d.det.assign(G, 0.0);
  d.term.assign(n, 0.0), d.gs.assign(dim * n, 0.0), d.ge.assign(dim * n, 0.0);
  if (dim == 3)
    run<3>(d);
  else
    run<2>(d);
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, d.inside) || !put(out, d.m) || !put(out, d.q) || !put(out, d.acc) ||
      !put(out, d.table) || !put(out, d.det) || !put(out, d.term) || !put(out, d.gs) ||
      !put(out, d.ge) || fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("columns %lld dimension %lld groups %lld\n", (long long)n, (long long)dim, (long long)G);
  return 0;
}
