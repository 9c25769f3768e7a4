// The uniform grid over the map's points that the particle filter's nearest-point searches walk (acmpc_pf_score.hip):
// built once per handle on the host.  Host only - no HIP here - so that the builder is tested on its own
// (tests/test_pf_grid.py).
#pragma once

#include <vector>

namespace acmpc {
namespace pf __attribute__((visibility("hidden"))) {

// cells of kGridCell metres over the box of all finite points; twice as wide, and again, while that would be more than
// kGridMaxCells of them
constexpr double kGridCell = 8.0;
constexpr long long kGridMaxCells = 1 << 20;

struct GridGeometry {
  double x0, y0, cell;
  int nx, ny;
};

struct PfGrid {
  GridGeometry geometry{};   // nx = ny = 0: the map has no finite point, and there is nothing to search
  // per polyline: cell c (row-major, nx * ny of them) holds entries [start[c], start[c + 1]) of index / x / y - the points
  // in cell order, ascending point index inside a cell, each with the index it has in the polyline
  std::vector<int> start[3], index[3];
  std::vector<double> x[3], y[3];
  // the 3 x 3 block of cells round every cell as ONE run, all three polylines in one set of arrays: block (t, c) holds
  // entries [block_start[t * cells + c], block_start[t * cells + c + 1]) - the rows of the block in order, the cells of a
  // row in order
  std::vector<int> block_start, block_index;
  std::vector<double> block_x, block_y;
  // (index / x / y and their block_ counterparts hold one unused entry where they would be empty: nothing is allocated
  // with a size of zero)
};

// track[t]: polyline t as x0, y0, x1, y1, ...  Non-finite points are left out (the exhaustive scan never picks them
// either: a NaN distance is never smaller).
PfGrid build_pf_grid(const std::vector<double> (&track)[3]);

}  // namespace pf
}  // namespace acmpc
