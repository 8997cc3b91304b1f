// csrc/combine_math.h on the host, under the address and undefined-behaviour sanitizers: the
// coefficients, the combined error and seed block of tfrt_error_combine and the residual, term and
// seed of tfrt_goal_error_columns, computed with the header's own functions in the kernels' order
// from exact-size allocations.  tests/test_error_combine_host.py writes the input, reads the
// output and compares it bit for bit with tests/error_combine_reference.py.
//
//   input : int64 {K, n, n_rows, reduce, m, n_source}
//           f64 weights[K], f64 terms[K], f64 errors[K], int32 row_mask[K],
//           f64 grads[K][n_rows][n], f64 o[m], int64 s[m], f64 goal[n_source]
//   output: f64 coeff[K], f64 E, f64 out[n_rows][n], f64 term[m], f64 seed[m]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "combine_math.h"

template <typename T>
static bool take(FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<int64_t> head;
  if (!take(in, head, 6)) return 3;
  const int64_t K = head[0], n = head[1], n_rows = head[2], reduce = head[3], m = head[4],
                n_source = head[5];
  if (K < 1 || K > tfrt::COMBINE_MAX_TERMS || n < 0 || n_rows < 1 || n_rows > 6 || m < 0 ||
      n_source < 0)
    return 3;
  std::vector<double> weights, terms, errors, grads, o, goal;
  std::vector<int32_t> row_mask;
  std::vector<int64_t> s;
  if (!take(in, weights, K) || !take(in, terms, K) || !take(in, errors, K) ||
      !take(in, row_mask, K) || !take(in, grads, (size_t)(K * n_rows * n)) || !take(in, o, m) ||
      !take(in, s, m) || !take(in, goal, n_source))
    return 3;
  fclose(in);

  std::vector<double> coeff(K), out((size_t)(n_rows * n)), term(m), seed(m);
  for (int64_t k = 0; k < K; ++k)
    coeff[k] = tfrt::combine_coefficient(weights[k], terms[k], (int)reduce);
  double E = 0.0;
  for (int64_t k = 0; k < K; ++k)
    E = k == 0 ? tfrt::combine_first(coeff[k], errors[k])
               : tfrt::combine_next(E, coeff[k], errors[k]);
  for (int64_t r = 0; r < n_rows; ++r)
    for (int64_t i = 0; i < n; ++i) {
      double acc = 0.0;
      bool have = false;
      for (int64_t k = 0; k < K; ++k) {
        if (!((row_mask[k] >> r) & 1)) continue;
        const double g = grads[(size_t)((k * n_rows + r) * n + i)];
        acc = have ? tfrt::combine_next(acc, coeff[k], g) : tfrt::combine_first(coeff[k], g);
        have = true;
      }
      out[(size_t)(r * n + i)] = acc;
    }
  for (int64_t j = 0; j < m; ++j) {
    double t = 0.0, sd = 0.0;
    if (tfrt::goal_source_ok(s[j], n_source)) {
      const double d = tfrt::goal_residual(o[j], goal[(size_t)s[j]]);
      t = tfrt::goal_term(d);
      sd = tfrt::goal_seed(d);
    }
    term[j] = t;
    seed[j] = sd;
  }

  FILE* dst = fopen(argv[2], "wb");
  if (!dst) return 4;
  bool ok = fwrite(coeff.data(), 8, K, dst) == (size_t)K && fwrite(&E, 8, 1, dst) == 1;
  if (!out.empty()) ok = ok && fwrite(out.data(), 8, out.size(), dst) == out.size();
  if (m > 0) ok = ok && fwrite(term.data(), 8, m, dst) == (size_t)m &&
                  fwrite(seed.data(), 8, m, dst) == (size_t)m;
  fclose(dst);
  return ok ? 0 : 4;
}
