// csrc/flatfield_math.h on the host (tests/test_flatfield_error_host.py compiles this with g++ and
// the address and undefined-behaviour sanitizers): reads a set of lines (end point, direction,
// length), which of them count and their groups, and writes what focus_math.h and flatfield_math.h
// make of them -- the groups' records, the (G, 8) table {x, used, mu, e_g}, the plane, the error
// triple and every ray's gradient.  The sums over the groups are taken in the definition's fixed
// shape and order (1,024 threads, groups j, j + 1024, ...; xor butterflies in each wave of 64; the
// 16 waves in index order), restated here in plain loops.
//
//   flatfield_main <in> <out>
//
// in:  int64 n, dim, G, pbits | f64 lo[3], hi[3], c[3], R, iR, min_det | f64 axis[3] |
//      f64 e[dim][n] | f64 u[dim][n] | f64 L[n] | int32 counts[n] | int32 label[n]
// out: int64 acc[G][10] | f64 table[G][8] | f64 fit[8] | f64 error[3] |
//      f64 g_start[dim][n] | f64 g_end[dim][n]      (g: 0 where a column has no term)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "flatfield_math.h"

template <typename V>
static bool get(FILE* f, std::vector<V>& v) {
  return v.empty() || fread(v.data(), sizeof(V), v.size(), f) == v.size();
}
template <typename V>
static bool put(FILE* f, const std::vector<V>& v) {
  return v.empty() || fwrite(v.data(), sizeof(V), v.size(), f) == v.size();
}

constexpr int THREADS = 1024;

// the fixed shape of a sum over the groups: `part` holds one partial per thread
static double block_sum(std::vector<double> part) {
  for (int w = 0; w < THREADS / 64; ++w)
    for (int d = 32; d > 0; d >>= 1)
      for (int l = 0; l < d; ++l) part[64 * w + l] = part[64 * w + l] + part[64 * w + l + d];
  double s = 0.0;
  for (int w = 0; w < THREADS / 64; ++w) s = s + part[64 * w];
  return s;
}

struct Data {
  int64_t n, G, pbits;
  tfrt::FocusBox box;
  double min_det, axis[3];
  std::vector<double> e, u, L;
  std::vector<int32_t> counts, label;
  std::vector<double> table, fit, error, gs, ge;
  std::vector<int64_t> acc;
};

template <int DIM>
static void run(Data& d) {
  const int64_t n = d.n, G = d.G;
  const double one = ldexp(1.0, (int)d.pbits), inv = ldexp(1.0, -(int)d.pbits);
  for (int64_t i = 0; i < n; ++i) {
    if (!d.counts[i]) continue;
    double e[DIM], u[DIM], m[DIM];
    int64_t q[tfrt::FOCUS_SLOTS];
    for (int a = 0; a < DIM; ++a) e[a] = d.e[a * n + i], u[a] = d.u[a * n + i];
    tfrt::focus_normalise<DIM>(e, d.box, m);
    tfrt::focus_record<DIM>(u, m, one, q);
    for (int p = 0; p < tfrt::FOCUS_SLOTS; ++p) d.acc[tfrt::FOCUS_SLOTS * d.label[i] + p] += q[p];
  }
  // first pass
  std::vector<double> W(THREADS, 0.0), S(THREADS, 0.0), inside(THREADS, 0.0);
  std::vector<double> x(3 * G), y(3 * G), h(G, 0.0);
  std::vector<uint8_t> used(G);
  int64_t n_used = 0, terms = 0;
  for (int64_t k = 0; k < G; ++k) {
    bool has;
    const int64_t* rec = &d.acc[tfrt::FOCUS_SLOTS * k];
    tfrt::flatfield_solve<DIM>(rec, inv, d.min_det, d.axis, &x[3 * k], &y[3 * k], has);
    used[k] = has;
    if (!has) continue;
    const double cnt = (double)rec[0];
    h[k] = tfrt::focus_dot<DIM>(d.axis, &x[3 * k]);
    W[k % THREADS] += cnt;
    S[k % THREADS] += cnt * h[k];
    n_used += 1;
    terms += rec[0];
  }
  const double Wsum = block_sum(W), Ssum = block_sum(S);
  const double hbar = Ssum / Wsum;
  const bool valid = n_used >= 2;
  // second pass
  for (int64_t k = 0; k < G; ++k) {
    double* row = &d.table[tfrt::FLATFIELD_ROW * k];
    double mu[3] = {0.0, 0.0, 0.0}, e = 0.0;
    if (used[k] && valid) {
      e = tfrt::flatfield_group<DIM>(h[k], hbar, d.box.R, &y[3 * k], mu);
      inside[k % THREADS] += (double)d.acc[tfrt::FOCUS_SLOTS * k] * e;
    }
    for (int b = 0; b < 3; ++b) row[b] = used[k] ? x[3 * k + b] : __builtin_nan("");
    row[3] = used[k] ? 1.0 : 0.0;
    row[4] = mu[0], row[5] = mu[1], row[6] = mu[2], row[7] = e;
  }
  const double in = block_sum(inside);
  d.error[0] = in, d.error[1] = (double)terms;
  d.error[2] = terms > 0 ? in / (double)terms : __builtin_nan("");
  d.fit[0] = hbar, d.fit[1] = tfrt::focus_dot<DIM>(d.axis, d.box.c) + d.box.R * hbar;
  d.fit[2] = Wsum, d.fit[3] = (double)n_used, d.fit[4] = valid ? 1.0 : 0.0;
  for (int64_t i = 0; i < n; ++i) {
    if (!d.counts[i] || !used[d.label[i]] || !valid) continue;
    double e[DIM], u[DIM], m[DIM], gs[DIM], ge[DIM];
    for (int a = 0; a < DIM; ++a) e[a] = d.e[a * n + i], u[a] = d.u[a * n + i];
    tfrt::focus_normalise<DIM>(e, d.box, m);
    const double* row = &d.table[tfrt::FLATFIELD_ROW * d.label[i]];
    tfrt::flatfield_ray<DIM>(u, m, row, row + 4, d.box.R, d.L[i], gs, ge);
    for (int a = 0; a < DIM; ++a) d.gs[a * n + i] = gs[a], d.ge[a * n + i] = ge[a];
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: flatfield_main <in> <out>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> head(4);
  std::vector<double> box(15);
  if (!get(in, head) || !get(in, box)) return 3;
  Data d;
  d.n = head[0], d.G = head[2], d.pbits = head[3];
  const int64_t n = d.n, dim = head[1], G = d.G;
  if (n < 0 || (dim != 2 && dim != 3) || G < 1 || d.pbits < 1 ||
      d.pbits > tfrt::FOCUS_MAX_PBITS) {
    fprintf(stderr, "bad header\n");
    return 3;
  }
  for (int a = 0; a < 3; ++a) {
    d.box.lo[a] = box[a], d.box.hi[a] = box[3 + a], d.box.c[a] = box[6 + a];
    d.axis[a] = box[12 + a];
  }
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
  d.acc.assign(tfrt::FOCUS_SLOTS * G, 0), d.table.assign(tfrt::FLATFIELD_ROW * G, 0.0);
  d.fit.assign(tfrt::FLATFIELD_FIT_OUT, 0.0), d.error.assign(3, 0.0);
  d.gs.assign(dim * n, 0.0), d.ge.assign(dim * n, 0.0);
  if (dim == 3)
    run<3>(d);
  else
    run<2>(d);
  FILE* out = fopen(argv[2], "wb");
  if (!out || !put(out, d.acc) || !put(out, d.table) || !put(out, d.fit) || !put(out, d.error) ||
      !put(out, d.gs) || !put(out, d.ge) || fclose(out) != 0) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  printf("columns %lld dimension %lld groups %lld\n", (long long)n, (long long)dim, (long long)G);
  return 0;
}
