// Bins the three polylines of the particle filter's map into one grid geometry (acmpc_pf_grid.h).
#include "acmpc_pf_grid.h"

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace acmpc::pf {

PfGrid build_pf_grid(const std::vector<double> (&track)[3]) {
  PfGrid grid;
  GridGeometry& g = grid.geometry;
  double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int t = 0; t < 3; ++t)
    for (size_t m = 0; m + 1 < track[t].size(); m += 2) {
      const double x = track[t][m], y = track[t][m + 1];
      if (!std::isfinite(x) || !std::isfinite(y)) continue;
      lo[0] = std::min(lo[0], x);
      hi[0] = std::max(hi[0], x);
      lo[1] = std::min(lo[1], y);
      hi[1] = std::max(hi[1], y);
    }
  if (lo[0] <= hi[0]) {   // (a map without a finite point keeps nx = ny = 0: no cells, and only the unused entries below)
    double cell = kGridCell;
    for (;;) {
      const double nx = std::floor((hi[0] - lo[0]) / cell) + 1.0, ny = std::floor((hi[1] - lo[1]) / cell) + 1.0;
      if (nx * ny <= static_cast<double>(kGridMaxCells)) {
        g.nx = static_cast<int>(nx);
        g.ny = static_cast<int>(ny);
        break;
      }
      cell *= 2.0;
    }
    g.x0 = lo[0];
    g.y0 = lo[1];
    g.cell = cell;
  }
  const size_t cells = static_cast<size_t>(g.nx) * g.ny;
  for (int t = 0; t < 3; ++t) {
    const size_t M = track[t].size() / 2;
    std::vector<int> cell_of(M, -1);
    std::vector<int>& start = grid.start[t];
    start.assign(cells + 1, 0);
    for (size_t m = 0; m < M; ++m) {
      const double x = track[t][2 * m], y = track[t][2 * m + 1];
      if (!std::isfinite(x) || !std::isfinite(y)) continue;
      // the same expression the kernel uses for a particle: a point and a particle at the same place share a cell
      const int ix = std::min(std::max(static_cast<int>(std::floor((x - g.x0) / g.cell)), 0), g.nx - 1);
      const int iy = std::min(std::max(static_cast<int>(std::floor((y - g.y0) / g.cell)), 0), g.ny - 1);
      cell_of[m] = iy * g.nx + ix;
      ++start[cell_of[m] + 1];
    }
    for (size_t c = 0; c < cells; ++c) start[c + 1] += start[c];
    const size_t kept = std::max<size_t>(static_cast<size_t>(start[cells]), 1);
    grid.index[t].assign(kept, 0);
    grid.x[t].assign(kept, 0.0);
    grid.y[t].assign(kept, 0.0);
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (size_t m = 0; m < M; ++m) {   // ascending m: ascending indices inside a cell
      if (cell_of[m] < 0) continue;
      const size_t j = static_cast<size_t>(fill[cell_of[m]]++);
      grid.index[t][j] = static_cast<int>(m);
      grid.x[t][j] = track[t][2 * m];
      grid.y[t][j] = track[t][2 * m + 1];
    }
  }
  // the 3 x 3 block round every cell as one run: its rows in order, each row a run of the cell-ordered arrays
  grid.block_start.assign(3 * cells + 1, 0);
  for (int t = 0; t < 3; ++t) {
    const std::vector<int>& start = grid.start[t];
    for (int iy = 0; iy < g.ny; ++iy)
      for (int ix = 0; ix < g.nx; ++ix) {
        grid.block_start[t * cells + static_cast<size_t>(iy) * g.nx + ix] = static_cast<int>(grid.block_index.size());
        const int x_lo = std::max(ix - 1, 0), x_hi = std::min(ix + 1, g.nx - 1);
        for (int cy = std::max(iy - 1, 0); cy <= std::min(iy + 1, g.ny - 1); ++cy) {
          const int j0 = start[static_cast<size_t>(cy) * g.nx + x_lo], j1 = start[static_cast<size_t>(cy) * g.nx + x_hi + 1];
          grid.block_index.insert(grid.block_index.end(), grid.index[t].begin() + j0, grid.index[t].begin() + j1);
          grid.block_x.insert(grid.block_x.end(), grid.x[t].begin() + j0, grid.x[t].begin() + j1);
          grid.block_y.insert(grid.block_y.end(), grid.y[t].begin() + j0, grid.y[t].begin() + j1);
        }
      }
  }
  grid.block_start[3 * cells] = static_cast<int>(grid.block_index.size());
  if (grid.block_index.empty()) {
    grid.block_index.assign(1, 0);
    grid.block_x.assign(1, 0.0);
    grid.block_y.assign(1, 0.0);
  }
  return grid;
}

}  // namespace acmpc::pf
