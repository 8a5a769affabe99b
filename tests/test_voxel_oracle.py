"""Known answers for the C restatement of the point->voxel scatter-mean
(oracle/voxelize_oracle.c), hand-derived from spconv's CPU point2voxel
semantics (first-appearance voxel order, first max_points points, zyx
coordinates, drop out-of-range) and HardSimpleVFE (mean of kept points)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "oracle", "_build", "libvoxel_oracle.so")


@pytest.fixture(scope="module")
def vox():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
    lib = ctypes.CDLL(LIB)
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int)

    def run(points, vsize, rng, grid, max_points, max_voxels, nmean=None):
        pts = np.ascontiguousarray(points, np.float32)
        N, F = pts.shape
        nmean = nmean or F
        v = np.zeros((max_voxels, max_points, F), np.float32)
        c = np.zeros((max_voxels, 3), np.int32)
        n = np.zeros((max_voxels,), np.int32)
        m = np.zeros((max_voxels, nmean), np.float32)
        M = lib.cmt_oracle_voxelize(pts.ctypes.data_as(fp), N, F, np.array(vsize, np.float32).ctypes.data_as(fp),
                                    np.array(rng, np.float32).ctypes.data_as(fp),
                                    np.array(grid, np.int32).ctypes.data_as(ip), max_points, max_voxels, nmean,
                                    v.ctypes.data_as(fp), c.ctypes.data_as(ip), n.ctypes.data_as(ip),
                                    m.ctypes.data_as(fp))
        return M, v[:M], c[:M], n[:M], m[:M]
    return run


def test_first_appearance_order_and_zyx(vox):
    pts = [[1.5, 0.5, 0.5, 10, 0], [0.5, 0.5, 0.5, 20, 0], [1.6, 0.6, 0.6, 30, 0], [0.5, 2.5, 1.5, 40, 1]]
    M, v, c, n, m = vox(pts, [1, 1, 1], [0, 0, 0, 4, 4, 4], [4, 4, 4], 10, 100)
    assert M == 3
    assert c.tolist() == [[0, 0, 1], [0, 0, 0], [1, 2, 0]]          # z, y, x in first-appearance order
    assert n.tolist() == [2, 1, 1]
    assert np.allclose(m[0], [1.55, 0.55, 0.55, 20.0, 0.0])
    assert v[0, 2:].sum() == 0                                          # zero padded


def test_max_points_keeps_first_in_input_order(vox):
    pts = [[0.5, 0.5, 0.5, float(i), 0] for i in range(15)]
    M, v, c, n, m = vox(pts, [1, 1, 1], [0, 0, 0, 4, 4, 4], [4, 4, 4], 10, 100)
    assert M == 1 and n[0] == 10
    assert v[0, :, 3].tolist() == [float(i) for i in range(10)]
    assert m[0, 3] == np.float32(45.0) / np.float32(10.0)


def test_out_of_range_dropped_and_voxel_budget(vox):
    pts = [[-0.1, 0.5, 0.5, 1, 0], [4.0, 0.5, 0.5, 1, 0], [0.5, 0.5, 0.5, 1, 0], [1.5, 0.5, 0.5, 1, 0],
           [2.5, 0.5, 0.5, 1, 0], [1.5, 0.5, 0.5, 2, 0]]
    M, v, c, n, m = vox(pts, [1, 1, 1], [0, 0, 0, 4, 4, 4], [4, 4, 4], 10, 2)
    assert M == 2                                                       # third voxel dropped by the budget
    assert c.tolist() == [[0, 0, 0], [0, 0, 1]]
    assert n.tolist() == [1, 2]


G753 = dict(vsize=[1, 1, 1], rng=[0, 0, 0, 7, 5, 3], grid=[7, 5, 3])


def _pt(axis, value, feat=1.0):
    """One row, mid-voxel (0.5) on the two other axes."""
    p = [0.5, 0.5, 0.5, feat, 0.0]
    p[axis] = value
    return p


def test_non_finite_and_huge_coordinates_dropped(vox):
    # kept iff 0 <= v < grid holds for the fp32 quotient itself: NaN, +-inf and |v| >= 2^31 never reach an int
    bad = [_pt(0, np.nan), _pt(1, np.nan), _pt(2, np.nan), _pt(0, np.inf), _pt(1, -np.inf), _pt(2, 3e9),
           _pt(0, -3e9), _pt(1, 1e30)]
    pts = bad[:4] + [[3.5, 2.5, 1.5, 7.0, 0.0]] + bad[4:]
    M, v, c, n, m = vox(pts, max_points=10, max_voxels=20, **G753)
    assert M == 1
    assert c.tolist() == [[1, 2, 3]] and n.tolist() == [1]
    assert v[0, 0].tolist() == [3.5, 2.5, 1.5, 7.0, 0.0] and m[0].tolist() == [3.5, 2.5, 1.5, 7.0, 0.0]


def test_points_on_voxel_planes(vox):
    f32 = np.float32
    pts = []
    for axis, g in enumerate(G753["grid"]):
        g = f32(g)
        pts += [_pt(axis, v) for v in (
            0.0, -0.0,                                  # both in cell 0 (-0.0 >= 0)
            np.nextafter(f32(0), f32(-1)),              # the largest negative fp32: dropped
            g,                                          # the upper bound itself: dropped
            np.nextafter(g, f32(0)),                    # one ulp inside: cell g-1
            np.nextafter(f32(1), f32(0)), f32(1), np.nextafter(f32(1), f32(2)))]   # cells 0, 1, 1
    M, v, c, n, m = vox(pts, max_points=10, max_voxels=50, **G753)
    assert M == 7
    #                   x axis                        y axis                 z axis
    assert c.tolist() == [[0, 0, 0], [0, 0, 6], [0, 0, 1], [0, 4, 0], [0, 1, 0], [2, 0, 0], [1, 0, 0]]
    assert n.tolist() == [9, 1, 2, 1, 2, 1, 2]            # cell (0,0,0): 0.0, -0.0 and 1-ulp of each axis
    assert np.signbit(v[0, 1, 0]) and v[0, 1, 0] == 0     # the -0.0 row is kept as it came


def test_non_square_grid_corners_zyx(vox):
    corners = [(z, y, x) for z in (0, 2) for y in (0, 4) for x in (0, 6)]
    pts = [[x + 0.5, y + 0.5, z + 0.5, 1.0, 0.0] for z, y, x in corners]
    M, v, c, n, m = vox(pts, max_points=10, max_voxels=20, **G753)
    assert M == 8
    assert c.tolist() == [list(zyx) for zyx in corners]
    assert n.tolist() == [1] * 8


def test_keys_above_2_pow_31(vox):
    # (599 * 2048 + 2047) * 2048 + 2047 = 2 516 582 399 >= 2^31
    pts = [[2047.5, 2047.5, 599.5, 1.0, 0.0], [0.5, 0.5, 599.5, 2.0, 0.0]]
    M, v, c, n, m = vox(pts, [1, 1, 1], [0, 0, 0, 2048, 2048, 600], [2048, 2048, 600], 10, 10)
    assert M == 2
    assert c.tolist() == [[599, 2047, 2047], [599, 0, 0]]
    assert n.tolist() == [1, 1]


def test_nfeat_mean_smaller_than_f(vox):
    pts = [[0.25, 0.5, 0.5, 10, 20, 30], [1.5, 0.5, 0.5, 1, 2, 3], [0.75, 0.5, 0.5, 30, 40, 50]]
    M, v, c, n, m = vox(pts, max_points=10, max_voxels=20, nmean=3, **G753)
    assert M == 2 and n.tolist() == [2, 1]
    assert m.shape == (2, 3)
    assert m.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]            # x, y, z only
    assert v.shape == (2, 10, 6) and v[0, 1].tolist() == [0.75, 0.5, 0.5, 30, 40, 50]


def test_empty_input(vox):
    M, *_ = vox(np.zeros((0, 5), np.float32), [1, 1, 1], [0, 0, 0, 4, 4, 4], [4, 4, 4], 10, 10)
    assert M == 0
