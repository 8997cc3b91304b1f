// CPU harness around tensorflowraytrace_amd/csrc/density_map.h (TEST ONLY): the search and
// interpolation of the TFRT_PTS_DENSITY points program, compiled for the host, as a program of its
// own.  Built by tests/test_density_program_host.py with g++; never loaded by the product package.
//
//   density_map_main IN OUT
// IN:  int64 x_count, y_count, n | double lim[4] | double tables[2 (x_count + 1) +
//      2 x_count (y_count + 1)] | double bx[n] | double by[n]
// OUT: double x[n] | double y[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "density_map.h"

static bool read_all(FILE* f, void* dst, size_t bytes) { return fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t head[3];
  double lim[4];
  if (!read_all(in, head, sizeof head) || !read_all(in, lim, sizeof lim)) return 4;
  const int64_t xc = head[0], yc = head[1], n = head[2];
  if (xc < 1 || yc < 1 || n < 0 || xc > 4096 || yc > 4096) return 5;
  std::vector<double> tables(2 * (xc + 1) + 2 * xc * (yc + 1)), bx(n), by(n), x(n), y(n);
  if (!read_all(in, tables.data(), tables.size() * sizeof(double)) ||
      !read_all(in, bx.data(), n * sizeof(double)) || !read_all(in, by.data(), n * sizeof(double)))
    return 4;
  fclose(in);
  for (int64_t i = 0; i < n; ++i)
    tfrt::density_map(tables.data(), (int)xc, (int)yc, lim, bx[i], by[i], &x[i], &y[i]);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 3;
  const bool ok = fwrite(x.data(), sizeof(double), n, out) == (size_t)n &&
                  fwrite(y.data(), sizeof(double), n, out) == (size_t)n;
  fclose(out);
  return ok ? 0 : 6;
}
