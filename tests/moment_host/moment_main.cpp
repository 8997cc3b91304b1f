// Stand-alone host program over moment_math.h (tests/test_moment_error_host.py builds it with the
// address and undefined-behaviour sanitizers): reads a file of
//   int64 {G, two, mode, mbits}, f64 {x0, msx, y0, msy},
//   G records of four int64 {n, Sx, Sy, 0}, G records of nine int64 (the limb sums),
//   mode 0: G rows of k3 f64 (k3 = 3 with two fields, else 1)
// and writes, per group, 16 f64: {rays, used, n, cx, cy, Cxx, Cxy, Cyy, Dxx, Dxy, Dyy, e, kx, Fxx,
// Fxy, Fyy}.  Every vector is an exact-size allocation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "moment_math.h"

using namespace tfrt;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t head[4];
  double grid[4];
  if (std::fread(head, 8, 4, in) != 4 || std::fread(grid, 8, 4, in) != 4) return 4;
  const int64_t G = head[0];
  const bool two = head[1] != 0;
  const int mode = (int)head[2];
  const int k3 = two ? 3 : 1;
  MomentGrid g;
  g.x0 = grid[0], g.msx = grid[1], g.y0 = grid[2], g.msy = grid[3];
  g.mbits = (int32_t)head[3], g.h = g.mbits / 2, g.two = two;
  std::vector<int64_t> acc(4 * G), mom(MOMENT_SLOTS * G);
  std::vector<double> target(mode == MOMENT_TARGET ? k3 * G : 0);
  if (std::fread(acc.data(), 8, acc.size(), in) != acc.size()) return 5;
  if (std::fread(mom.data(), 8, mom.size(), in) != mom.size()) return 6;
  if (std::fread(target.data(), 8, target.size(), in) != target.size()) return 7;
  std::fclose(in);

  std::vector<double> out(16 * G);
  for (int64_t k = 0; k < G; ++k) {
    const int64_t rec[3] = {acc[4 * k], acc[4 * k + 1], acc[4 * k + 2]};
    const MomentGroup q =
        moment_group(rec, mom.data() + MOMENT_SLOTS * k, g, mode,
                     mode == MOMENT_TARGET ? target.data() + k3 * k : nullptr);
    double* o = out.data() + 16 * k;
    o[0] = q.rays ? 1.0 : 0.0, o[1] = q.used ? 1.0 : 0.0, o[2] = q.n;
    o[3] = q.cx, o[4] = q.cy;
    for (int c = 0; c < 3; ++c) o[5 + c] = q.C[c], o[8 + c] = q.D[c], o[13 + c] = q.F[c];
    o[11] = q.e;
    o[12] = q.rays ? (double)moment_centre(rec[0], rec[1]) : -1.0;
  }
  FILE* to = std::fopen(argv[2], "wb");
  if (!to) return 8;
  if (std::fwrite(out.data(), 8, out.size(), to) != out.size()) return 9;
  std::fclose(to);
  return 0;
}
