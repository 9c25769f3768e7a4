"""The particle filter's grid builder (csrc/acmpc_pf_grid.cpp: build_pf_grid) on the CPU: tests/pf_grid_main.cpp is compiled
with it by a host compiler under AddressSanitizer and UBSan and run as an ordinary child process, and what it writes is
checked exactly against the definition of the grid stated here in NumPy float64.  The kernels that search the grid
(csrc/acmpc_pf_score.hip) trust these arrays blindly: an index out of place is a wrong nearest point or a read out of bounds."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ac-mpc_amd"))

import pf_scenes  # noqa: E402
from acmpc_amd import _build  # noqa: E402

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
CELL, MAX_CELLS = 8.0, 1 << 20   # kGridCell, kGridMaxCells


def host_compiler():
    """g++, else the clang++ that ships beside hipcc - never hipcc itself, which would compile the .cpp as HIP."""
    found = shutil.which("g++")
    if found is None:
        hipcc = os.path.realpath(_build.find_hipcc())
        rocm = os.path.dirname(os.path.dirname(hipcc))
        for cand in (os.path.join(rocm, "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
                     os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
            if os.path.exists(cand):
                found = cand
                break
    assert found is not None, "no host C++ compiler: neither g++ nor the clang++ beside hipcc"
    return found


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("pf_grid") / "pf_grid_main")
    compiler = host_compiler()
    # g++ links the sanitizers' runtimes as shared libraries by default, and ASan then refuses to start in a process that has
    # any other library preloaded in front of it; linked into the program (clang++'s default) it starts anywhere
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler).startswith("g++") else []
    subprocess.run([compiler, *FLAGS, *static, "-I", _build.CSRC_DIR, os.path.join(_build.CSRC_DIR, "acmpc_pf_grid.cpp"),
                    os.path.join(ROOT, "tests", "pf_grid_main.cpp"), "-o", binary], check=True)
    return binary


def build_grid(program, track, tmp_path):
    """Runs the program on the three polylines; returns (x0, y0, cell, nx, ny), per polyline (start, index, x, y), the blocks' four."""
    lines = [np.ascontiguousarray(track[k], dtype=np.float64).reshape(-1, 2) for k in ("centre", "left", "right")]
    source, result = str(tmp_path / "map.bin"), str(tmp_path / "grid.bin")
    with open(source, "wb") as handle:
        handle.write(np.array([len(line) for line in lines], dtype=np.int64).tobytes())
        for line in lines:
            handle.write(line.tobytes())
    done = subprocess.run([program, source, result], capture_output=True, text=True)
    assert done.returncode == 0, "exit status %d\n%s" % (done.returncode, done.stderr[-4000:])
    raw = open(result, "rb").read()
    x0, y0, cell = np.frombuffer(raw, np.float64, 3, 0)
    nx, ny = (int(v) for v in np.frombuffer(raw, np.int64, 2, 24))
    at, arrays = 40, []
    for dtype in [np.int32, np.int32, np.float64, np.float64] * 4:
        n = int(np.frombuffer(raw, np.int64, 1, at)[0])
        arrays.append(np.frombuffer(raw, dtype, n, at + 8))
        at += 8 + n * np.dtype(dtype).itemsize
    assert at == len(raw)
    return lines, (x0, y0, cell, nx, ny), [arrays[4 * t:4 * t + 4] for t in range(3)], arrays[12:]


def expected_geometry(lines):
    points = np.concatenate(lines)
    points = points[np.isfinite(points).all(axis=1)]
    if len(points) == 0:
        return None
    lo, hi = points.min(axis=0), points.max(axis=0)
    cell = CELL
    while True:   # the smallest 8 * 2^k with nx * ny <= 2^20
        nx, ny = np.floor((hi - lo) / cell) + 1.0
        if nx * ny <= MAX_CELLS:
            return lo[0], lo[1], cell, int(nx), int(ny)
        cell *= 2.0


def concatenated_runs(first, last):
    """Indices first[0] .. last[0] - 1, first[1] .. last[1] - 1, ... in one array."""
    length = last - first
    return np.repeat(first - (np.cumsum(length) - length), length) + np.arange(length.sum())


def check_grid(lines, geometry, per_line, blocks):
    x0, y0, cell, nx, ny = geometry
    expected = expected_geometry(lines)
    if expected is None:   # no finite point: no cells, and the one-entry placeholder arrays
        assert (nx, ny) == (0, 0)
        for start, index, x, y in per_line + [blocks]:
            assert start.tolist() == [0] and index.tolist() == [0] and x.tolist() == [0.0] and y.tolist() == [0.0]
        return
    assert (x0, y0, cell, nx, ny) == expected
    cells = nx * ny
    block_parts = []
    for line, (start, index, x, y) in zip(lines, per_line):
        finite = np.flatnonzero(np.isfinite(line).all(axis=1))
        assert start.shape == (cells + 1,) and start[0] == 0 and (np.diff(start) >= 0).all() and start[cells] == len(finite)
        kept = max(len(finite), 1)
        assert index.shape == x.shape == y.shape == (kept,)
        index, x, y = index[:len(finite)], x[:len(finite)], y[:len(finite)]
        # every finite point exactly once, with its own coordinates beside its index
        assert np.array_equal(np.sort(index), finite)
        assert np.array_equal(x, line[index, 0]) and np.array_equal(y, line[index, 1])
        # in the cell that the clamped floor gives, indices ascending inside a cell
        ix = np.clip(np.floor((x - x0) / cell), 0, nx - 1).astype(np.int64)
        iy = np.clip(np.floor((y - y0) / cell), 0, ny - 1).astype(np.int64)
        cell_of_entry = np.repeat(np.arange(cells), np.diff(start))
        assert np.array_equal(iy * nx + ix, cell_of_entry)
        same_cell = cell_of_entry[1:] == cell_of_entry[:-1]
        assert (np.diff(index)[same_cell] > 0).all()
        # block (t, c): the cell runs of the clipped 3 x 3 neighbourhood, row by row
        cy, cx = np.divmod(np.arange(cells), nx)
        rows = cy[:, None] + np.array([-1, 0, 1])[None, :]
        inside = (rows >= 0) & (rows < ny)
        rows = np.clip(rows, 0, ny - 1)
        first = start[rows * nx + np.maximum(cx - 1, 0)[:, None]].astype(np.int64)
        last = np.where(inside, start[rows * nx + np.minimum(cx + 1, nx - 1)[:, None] + 1], first).astype(np.int64)
        gather = concatenated_runs(first.ravel(), last.ravel())
        block_parts.append(((last - first).sum(axis=1), index[gather], x[gather], y[gather]))
    start, index, x, y = blocks
    lengths = np.concatenate([part[0] for part in block_parts])
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(lengths)]))
    total = int(lengths.sum())
    assert index.shape == x.shape == y.shape == (max(total, 1),)
    assert np.array_equal(index[:total], np.concatenate([part[1] for part in block_parts]))
    assert np.array_equal(x[:total], np.concatenate([part[2] for part in block_parts]))
    assert np.array_equal(y[:total], np.concatenate([part[3] for part in block_parts]))


def with_non_finite():
    track = {k: v.copy() for k, v in pf_scenes.tiny_map().items()}
    track["centre"][[0, 17, 149], 0] = np.nan
    track["centre"][60, 1] = np.inf
    track["left"][[5, 148]] = [[-np.inf, 1.0], [np.nan, np.nan]]
    track["right"][100, 1] = -np.inf
    return track


def one_point():
    point = np.array([[12.5, -3.25]])
    return dict(centre=np.repeat(point, 40, axis=0), left=np.repeat(point, 7, axis=0), right=np.repeat(point, 1, axis=0))


def shortest():
    return dict(centre=np.array([[0.0, 0.0], [9.0, 0.5], [17.5, -30.0]]), left=np.array([[-2.0, 100.0]]), right=np.array([[8.0, 8.0]]))


def all_nan():
    return dict(centre=np.full((5, 2), np.nan), left=np.full((2, 2), np.nan), right=np.full((1, 2), np.nan))


MAPS = {"tiny": pf_scenes.tiny_map, "long": pf_scenes.long_map, "non_finite": with_non_finite, "one_point": one_point,
        "shortest": shortest, "all_nan": all_nan}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_the_grid_is_the_one_defined(program, tmp_path, name):
    lines, geometry, per_line, blocks = build_grid(program, MAPS[name](), tmp_path)
    check_grid(lines, geometry, per_line, blocks)
    if name == "long":       # more than 2^20 cells of 8 m: one doubling (tests/test_gpu_pf_maps.py relies on it)
        assert geometry[2] == 16.0
    elif name == "one_point":
        assert geometry[3:] == (1, 1)
    elif name != "all_nan":
        assert geometry[2] == 8.0
