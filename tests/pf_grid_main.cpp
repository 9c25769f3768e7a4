// Stand-alone driver of csrc/acmpc_pf_grid.cpp for tests/test_pf_grid.py (host compiler, AddressSanitizer and UBSan):
//   pf_grid_main IN OUT
// IN:  int64 m[3], then the three polylines as float64 [m][2].
// OUT: float64 x0, y0, cell; int64 nx, ny; then per polyline start (int32), index (int32), x, y (float64) and the same four
//      for the 3 x 3 blocks, every array as an int64 length and its elements.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "acmpc_pf_grid.h"

namespace {

template <typename T>
bool put(std::FILE* f, const std::vector<T>& v) {
  const int64_t n = static_cast<int64_t>(v.size());
  return std::fwrite(&n, sizeof n, 1, f) == 1 && std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (in == nullptr) return 3;
  int64_t m[3];
  std::vector<double> track[3];
  bool ok = std::fread(m, sizeof m[0], 3, in) == 3;
  for (int t = 0; t < 3 && ok; ++t) {
    ok = m[t] >= 0;
    if (ok) track[t].resize(2 * static_cast<size_t>(m[t]));
    ok = ok && std::fread(track[t].data(), sizeof(double), track[t].size(), in) == track[t].size();
  }
  std::fclose(in);
  if (!ok) return 4;

  const acmpc::pf::PfGrid grid = acmpc::pf::build_pf_grid(track);

  std::FILE* out = std::fopen(argv[2], "wb");
  if (out == nullptr) return 5;
  const double box[3] = {grid.geometry.x0, grid.geometry.y0, grid.geometry.cell};
  const int64_t shape[2] = {grid.geometry.nx, grid.geometry.ny};
  ok = std::fwrite(box, sizeof box[0], 3, out) == 3 && std::fwrite(shape, sizeof shape[0], 2, out) == 2;
  for (int t = 0; t < 3; ++t) ok = ok && put(out, grid.start[t]) && put(out, grid.index[t]) && put(out, grid.x[t]) && put(out, grid.y[t]);
  ok = ok && put(out, grid.block_start) && put(out, grid.block_index) && put(out, grid.block_x) && put(out, grid.block_y);
  return (std::fclose(out) == 0 && ok) ? 0 : 6;
}
