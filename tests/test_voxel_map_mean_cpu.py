"""The voxel map of means without a GPU: the host restatement the GPU tests compare against (voxel_map_mean_restatement.py)
is itself held to the rule (voxel_mean_restatement.py), and the two new entries of the C ABI are checked as the other
*_abi_cpu.py files check theirs: exported, declared, mirrored, and every refusal that is decided on the host (a map
allocates nothing before its first point, so a made-up context does: nothing is dereferenced)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import voxel_mean_cases as cases
from align3d_amd import DeviceVoxelMap, _abi
from voxel_map_mean_restatement import MeanMapRestatement, continued_mean, retained_mean
from voxel_mean_restatement import error_bound, exact_mean, voxel_mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_CTX = 0x900000
SENTINEL = 0x7777
ORIGIN = (0.013, -0.4, 7.5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Two results of voxel_mean (or continued_mean), bit for bit."""
    for g, w, floats in zip(got, want, (True, True, False, False, False, False)):
        assert (g is None) == (w is None)
        if g is not None:
            assert np.array_equal(_bits(g), _bits(w)) if floats else np.array_equal(g, w)


def _cloud(seed=3):
    points, normals, colors = cases.scanline(83, 61, seed=seed, nan_every=11)
    return points + np.float32(ORIGIN), normals, colors


def test_pieces_give_the_mean_of_the_whole():
    points, normals, colors = _cloud()
    whole = voxel_mean(points, normals, colors, cases.VOXEL, ORIGIN)
    assert (whole[4] > 1).any() and (whole[4] == 1).any() and whole[5] > 0  # the case is meaningful
    for k in (1, 2, 3, 7):
        cuts = np.linspace(0, len(points), k + 1).astype(int)
        pieces = [(points[a:b], normals[a:b], colors[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        model = MeanMapRestatement(*(np.concatenate([p[i] for p in pieces]) for i in range(3)), cases.VOXEL, ORIGIN)
        _same((model.rows, model.normals, model.colors, model.seq, model.counts, model.dropped), whole)
    # and through a retain that removes nothing: the survivors of the first part, then the second part summed into them
    half = len(points) // 2
    first = MeanMapRestatement(points[:half], normals[:half], colors[:half], cases.VOXEL, ORIGIN)
    keep, removed, marks, k, continued = retained_mean(first, marks=(0, half, 1 << 40))
    assert keep.all() and removed == 0 and marks == [0, k, k] and k == len(first.rows)
    got = continued_mean(continued, k, points[half:], normals[half:], colors[half:], cases.VOXEL, ORIGIN)
    _same(got[:3], whole[:3])
    assert np.array_equal(got[4], whole[4]) and got[5] == whole[5] - first.dropped
    # the numbering: survivor j is j; a cell that the second part opened has k + its position there
    old = whole[3] < half
    assert np.array_equal(got[3][old], np.arange(k)) and np.array_equal(got[3][~old], whole[3][~old] - half + k)


def test_a_permutation_gives_the_same_rows():
    points, normals, colors = _cloud(5)
    perm = np.random.default_rng(9).permutation(len(points))

    def rows(p, n, c):
        out_p, out_n, out_c, _, counts, _ = voxel_mean(p, n, c, cases.VOXEL, ORIGIN)
        table = np.concatenate([_bits(out_p), _bits(out_n), out_c.astype(np.uint32), counts[:, None].astype(np.uint32)], axis=1)
        single = counts == 1  # (a lone row is a copy: the same under any order too)
        return table[np.lexsort(table.T[::-1])], int(single.sum())

    a, singles = rows(points, normals, colors)
    b, _ = rows(points[perm], normals[perm], colors[perm])
    assert singles > 0 and len(a) > 100 and np.array_equal(a, b)


def test_rows_are_within_the_bound_of_the_exact_mean():
    points, normals, colors = _cloud(7)
    model = MeanMapRestatement(points, normals, colors, cases.VOXEL, ORIGIN)
    err = np.abs(model.rows.astype(np.float64) - exact_mean(points, cases.VOXEL, ORIGIN)).max()
    assert err <= error_bound(points, cases.VOXEL, ORIGIN)
    # every stored row answers for the cell of its INPUT points, also where the mean rounds onto a face
    assert all(model.cells[int(key)][1] == row for row, key in enumerate(model.row_keys.tolist()))


def test_retained_mean_keeps_whole_cells():
    points, normals, colors = _cloud(11)
    model = MeanMapRestatement(points, normals, colors, cases.VOXEL, ORIGIN)
    lo, hi = np.float32(ORIGIN) + np.float32([-0.2, -0.1, -1.0]), np.float32(ORIGIN) + np.float32([0.3, 0.25, 1.0])
    keep, removed, marks, k, continued = retained_mean(model, min_seq=500, box=(lo, hi), marks=(0, 500, 3000))
    assert 0 < k < len(model.rows) and removed == len(model.rows) - k and marks[0] == marks[1] == 0 < marks[2] <= k
    got = continued_mean(continued, k, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8),
                         cases.VOXEL, ORIGIN)
    _same(got[:3], (model.rows[keep], model.normals[keep], model.colors[keep]))
    assert np.array_equal(got[3], np.arange(k)) and np.array_equal(got[4], model.counts[keep]) and got[5] == 0


# ---- the C ABI


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _new(lib, maker="a3d_voxel_map_new_mean", normals=1, colors=1):
    h = C.c_void_p()
    if maker == "a3d_voxel_map_new_mean":
        assert lib.a3d_voxel_map_new_mean(C.c_void_p(FAKE_CTX), 0.05, None, normals, colors, 0, C.byref(h)) == _abi.A3D_OK
    else:
        assert lib.a3d_voxel_map_new_rgb(C.c_void_p(FAKE_CTX), 0.05, None, normals, colors, 0, C.byref(h)) == _abi.A3D_OK
    return h


def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    want = {
        "a3d_voxel_map_new_mean": ["a3d_context* ctx", "float voxel_size", "const float origin[3]", "int with_normals",
                                   "int with_colors", "uint64_t reserve_cells", "a3d_voxel_map** out"],
        "a3d_voxel_map_extract_mean": ["a3d_voxel_map* map", "float* d_out_points", "float* d_out_normals",
                                       "uint8_t* d_out_colors", "uint32_t* d_out_index", "uint32_t* d_out_counts",
                                       "uint64_t capacity", "uint64_t* out_len"],
    }
    for name, params in want.items():
        assert hasattr(lib, name) and hasattr(diag, name)
        decl = re.search(r"a3d_status\s+" + name + r"\s*\((.*?)\);", section, re.S)
        assert decl and [" ".join(p.split()) for p in decl.group(1).split(",")] == params
        assert len(_abi.SIGNATURES[name][1]) == len(params)


def test_new_mean_refuses_what_new_refuses(lib):
    h = C.c_void_p(SENTINEL)
    bad_origin = (C.c_float * 3)(0.0, float("inf"), 0.0)
    assert lib.a3d_voxel_map_new_mean(None, 0.05, None, 1, 1, 0, C.byref(h)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_new_mean(C.c_void_p(FAKE_CTX), 0.05, None, 1, 1, 0, None) == _abi.A3D_INVALID_PARAMETER
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.a3d_voxel_map_new_mean(C.c_void_p(FAKE_CTX), v, None, 1, 1, 0, C.byref(h)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_new_mean(C.c_void_p(FAKE_CTX), 0.05, bad_origin, 1, 1, 0, C.byref(h)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_new_mean(C.c_void_p(FAKE_CTX), 0.05, None, 1, 1, 1 << 32, C.byref(h)) == _abi.A3D_INVALID_PARAMETER
    assert h.value == SENTINEL


def test_extract_mean_refusals_decided_on_the_host(lib):
    buf = (C.c_uint32 * 64)()
    at = lambda word: C.c_void_p(C.addressof(buf) + 4 * word)  # noqa: E731
    n = C.c_uint64(SENTINEL)
    mean, nearest, bare = _new(lib), _new(lib, "a3d_voxel_map_new_rgb"), _new(lib, normals=0, colors=0)
    call = lib.a3d_voxel_map_extract_mean
    assert call(None, at(0), None, None, None, None, 0, C.byref(n)) == _abi.A3D_INVALID_PARAMETER  # NULL map
    assert call(mean, None, None, None, None, None, 0, C.byref(n)) == _abi.A3D_INVALID_PARAMETER  # NULL points
    assert call(mean, at(0), None, None, None, None, 0, None) == _abi.A3D_INVALID_PARAMETER  # NULL out_len
    assert n.value == SENTINEL
    # counts of a nearest-point map: it keeps none
    assert call(nearest, at(0), None, None, None, at(32), 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER and n.value == SENTINEL
    # normals / colours of a map that keeps none
    assert call(bare, at(0), at(16), None, None, None, 1, C.byref(n)) == _abi.A3D_MISSING_FIELD
    assert call(bare, at(0), None, at(16), None, None, 1, C.byref(n)) == _abi.A3D_MISSING_FIELD
    # the counts take part in the overlap check: 4 rows of points are words 0 ... 11
    assert call(mean, at(0), None, None, None, at(11), 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER
    assert call(mean, at(0), None, None, at(12), at(15), 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER
    assert n.value == SENTINEL
    # an empty map of means extracts nothing, with or without counts; without counts the entry serves either kind
    assert call(mean, at(0), None, None, at(12), at(16), 4, C.byref(n)) == _abi.A3D_OK and n.value == 0
    n.value = SENTINEL
    assert call(nearest, at(0), None, None, at(12), None, 4, C.byref(n)) == _abi.A3D_OK and n.value == 0
    assert not any(buf)
    for h in (mean, nearest, bare):
        lib.a3d_voxel_map_free(h)


def test_python_wrapper_checks_its_arguments(lib):
    ctx = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX))
    for mode in ("median", "", None, "MEAN", 1):
        with pytest.raises(_abi.InvalidParameter):
            DeviceVoxelMap(ctx, 0.05, mode=mode)
    nearest, mean = DeviceVoxelMap(ctx, 0.05), DeviceVoxelMap(ctx, 0.05, colors=True, mode="mean")
    with pytest.raises(_abi.InvalidParameter):
        nearest.extract(return_counts=True)
    with pytest.raises(_abi.InvalidParameter):
        nearest.extract(return_index=True, return_counts=True)
    assert nearest.mode == "nearest" and nearest.stats() == dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)
    assert mean.stats() == dict(cells=0, slots=0, total=0, dropped_total=0, growths=0, mode="mean", bytes_per_slot=128)
    assert (nearest.bytes_per_slot(), DeviceVoxelMap(ctx, 0.05, normals=False, mode="mean").bytes_per_slot()) == (40, 64)
    assert DeviceVoxelMap(ctx, 0.05, mode="mean").bytes_per_slot() == 100
    assert mean.retain() == 0 and mean.compact() == 0  # a map that holds no table yet
    mean.clear()
    nearest.free(), mean.free()
