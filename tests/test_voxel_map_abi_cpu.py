"""The C ABI of the persistent voxel map (a3d_voxel_map_*) without a GPU: the exported symbols, the header, the ctypes
mirror, every refusal that is decided on the host before any HIP call (a map allocates nothing on the device before its
first point, so a made-up context and made-up device addresses do: nothing is dereferenced), and the contract itself as
a pure-numpy property: per-key minima of bits(dist) << 32 | global index kept incrementally over any partition of a
cloud equal voxel_restatement.voxel_downsample of the whole."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import voxel_restatement as V
from align3d_amd import DevicePointCloud, DeviceVoxelMap, PointCloud, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"a3d_voxel_map_new": 6, "a3d_voxel_map_insert": 6, "a3d_voxel_map_extract": 6, "a3d_voxel_map_get_stats": 2,
         "a3d_voxel_map_clear": 1, "a3d_voxel_map_free": 1}
SENTINEL = 0x7777
FAKE_CTX = 0x900000


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


def _new(lib, voxel=0.05, origin=None, normals=1, reserve=0, ctx=FAKE_CTX):
    h = C.c_void_p()
    st = lib.a3d_voxel_map_new(C.c_void_p(ctx) if ctx else None, voxel, origin, normals, reserve, C.byref(h))
    return st, h


def _stats(lib, h):
    s = _abi.VoxelMapStatsC()
    assert lib.a3d_voxel_map_get_stats(h, C.byref(s)) == _abi.A3D_OK
    return s.as_dict()


EMPTY_STATS = dict(cells=0, slots=0, total=0, dropped_total=0, growths=0)


class _Insert:
    """Two clouds of 4 points at made-up device addresses and sentinel-filled result words."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 2)()
        self.views[0].points, self.views[0].normals, self.views[0].len = 0x10000, 0x20000, 4
        self.views[1].points, self.views[1].normals, self.views[1].len = 0x30000, 0x40000, 4
        self.dropped = (C.c_uint64 * 2)(SENTINEL, SENTINEL)
        self.cells = C.c_uint64(SENTINEL)

    def call(self, lib, h, n=2, views="own", poses=None):
        return lib.a3d_voxel_map_insert(h, self.views if views == "own" else views, poses, n, self.dropped,
                                        C.byref(self.cells))

    def untouched(self):
        return list(self.dropped) == [SENTINEL] * 2 and self.cells.value == SENTINEL


def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    section = header[header.index("PointCloud resident on the device"):header.index("---- R3dTree")]
    for name, arity in NAMES.items():
        assert hasattr(lib, name) and hasattr(diag, name), name
        assert re.search(r"(a3d_status|void)\s+%s\s*\(" % name, section), name
        assert name in _abi.SIGNATURES and len(_abi.SIGNATURES[name][1]) == arity, name
    assert "typedef struct a3d_voxel_map a3d_voxel_map;" in section
    body = re.search(r"typedef struct a3d_voxel_map_stats \{(.*?)\} a3d_voxel_map_stats;", section, re.S).group(1)
    fields = re.findall(r"uint64_t\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _abi.VoxelMapStatsC._fields_] == ["cells", "slots", "total", "dropped_total", "growths"]
    assert C.sizeof(_abi.VoxelMapStatsC) == 40
    # the header states the contract, the sequence-number rule, the reservation rule and the limit
    text = " ".join(section.split())
    for needle in ("in insertion order", "seq = total + sum(len[0..j)) + i", "slots >= 2 * (cells + L)", "2^32 - 2^21",
                   "NOT built"):
        assert needle in text, needle
    assert lib.a3d_abi_version() == 1 and "#define A3D_ABI_VERSION 1" in header
    for method in ("insert", "insert_many", "extract", "cells", "total", "stats", "clear", "free", "__del__"):
        assert callable(getattr(DeviceVoxelMap, method))


def test_product_library_has_no_knob_for_the_feature():
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"A3D_VOXEL" not in blob


def test_new_refuses_bad_arguments_and_allocates_nothing(lib):
    st, h = _new(lib)
    assert st == _abi.A3D_OK and h.value
    assert _stats(lib, h) == EMPTY_STATS
    lib.a3d_voxel_map_free(h)
    lib.a3d_voxel_map_free(None)
    assert _new(lib, ctx=None)[0] == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_new(C.c_void_p(FAKE_CTX), 0.05, None, 1, 0, None) == _abi.A3D_INVALID_PARAMETER
    for voxel in (0.0, -0.0, -0.05, float("nan"), float("inf"), float("-inf")):
        st, h = _new(lib, voxel=voxel)
        assert st == _abi.A3D_INVALID_PARAMETER and not h.value, voxel
    for bad in (float("nan"), float("inf"), float("-inf")):
        for axis in range(3):
            origin = (C.c_float * 3)(0.0, 0.0, 0.0)
            origin[axis] = bad
            st, h = _new(lib, origin=origin)
            assert st == _abi.A3D_INVALID_PARAMETER and not h.value
    # a reservation of 2^32 cells or more is refused (no map can hold them: a sequence number has 32 bits)
    for reserve in (1 << 32, (1 << 32) + 1, (1 << 64) - 1):
        st, h = _new(lib, reserve=reserve)
        assert st == _abi.A3D_INVALID_PARAMETER and not h.value, reserve
    st, h = _new(lib, reserve=(1 << 32) - 1)
    assert st == _abi.A3D_OK and _stats(lib, h) == EMPTY_STATS  # (nothing is allocated before the first point)
    lib.a3d_voxel_map_free(h)
    st, h = _new(lib, origin=(C.c_float * 3)(0.5, -2.0, 1e30), normals=0, reserve=1000)
    assert st == _abi.A3D_OK and _stats(lib, h) == EMPTY_STATS
    lib.a3d_voxel_map_free(h)


def test_null_arguments_are_invalid_without_a_device(lib):
    _, h = _new(lib)
    a = _Insert()
    assert a.call(lib, None) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert a.call(lib, h, views=None) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    n = C.c_uint64(SENTINEL)
    pts, idx = C.c_void_p(0x50000), C.c_void_p(0x60000)
    assert lib.a3d_voxel_map_extract(None, pts, None, idx, 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_extract(h, None, None, idx, 4, C.byref(n)) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_extract(h, pts, None, idx, 4, None) == _abi.A3D_INVALID_PARAMETER
    assert n.value == SENTINEL
    assert lib.a3d_voxel_map_get_stats(None, C.byref(_abi.VoxelMapStatsC())) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_get_stats(h, None) == _abi.A3D_INVALID_PARAMETER
    assert lib.a3d_voxel_map_clear(None) == _abi.A3D_INVALID_PARAMETER
    assert _stats(lib, h) == EMPTY_STATS
    lib.a3d_voxel_map_free(h)


def test_empty_call_is_ok_and_touches_nothing(lib):
    _, h = _new(lib)
    a = _Insert()
    assert lib.a3d_voxel_map_insert(None, None, None, 0, None, None) == _abi.A3D_OK
    assert a.call(lib, h, n=0) == _abi.A3D_OK and a.untouched()
    assert _stats(lib, h) == EMPTY_STATS
    # clouds of no points offer nothing (their pointers may be null): still no device
    a.views[0].len = a.views[1].len = 0
    a.views[0].points = a.views[1].normals = None
    assert a.call(lib, h) == _abi.A3D_OK
    assert list(a.dropped) == [0, 0] and a.cells.value == 0 and _stats(lib, h) == EMPTY_STATS
    assert lib.a3d_voxel_map_clear(h) == _abi.A3D_OK and _stats(lib, h) == EMPTY_STATS
    lib.a3d_voxel_map_free(h)


def test_insert_refusals_are_decided_on_the_host_and_change_nothing(lib):
    _, h = _new(lib)
    for big in (1 << 32, (1 << 32) + 5, 1 << 40):
        a = _Insert()
        a.views[1].len = big
        assert a.call(lib, h) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    a = _Insert()
    a.views[0].points = None
    assert a.call(lib, h) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    # a map with normals refuses the whole call if one non-empty cloud has none, whichever it is
    for i in (0, 1):
        a = _Insert()
        a.views[i].normals = None
        assert a.call(lib, h) == _abi.A3D_MISSING_FIELD and a.untouched()
    # the limit: total + L stays below 2^32 - 2^21 (each cloud alone is below 2^32)
    a = _Insert()
    a.views[0].len = a.views[1].len = (1 << 31) - (1 << 20)
    assert a.call(lib, h) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    a = _Insert()
    a.views[0].len, a.views[1].len = (1 << 32) - (1 << 21) - 4, 4
    assert a.call(lib, h) == _abi.A3D_INVALID_PARAMETER and a.untouched()
    assert _stats(lib, h) == EMPTY_STATS
    lib.a3d_voxel_map_free(h)


def test_extract_refusals_are_decided_on_the_host(lib):
    _, with_n = _new(lib, normals=1)
    _, without_n = _new(lib, normals=0)
    n = C.c_uint64(SENTINEL)
    pts, nrm, idx = 0x50000, 0x60000, 0x70000
    assert lib.a3d_voxel_map_extract(without_n, C.c_void_p(pts), C.c_void_p(nrm), C.c_void_p(idx), 4,
                                     C.byref(n)) == _abi.A3D_MISSING_FIELD
    assert n.value == SENTINEL
    # outputs that overlap one another (4 rows: 48 bytes of points or normals, 16 of index)
    for p, q, i in ((pts, pts, idx), (pts, pts + 36, idx), (pts, pts - 44, idx), (pts, nrm, pts + 44), (pts, nrm, nrm - 12),
                    (pts, nrm, pts - 12), (pts, None, pts)):
        st = lib.a3d_voxel_map_extract(with_n, C.c_void_p(p), C.c_void_p(q) if q else None, C.c_void_p(i), 4, C.byref(n))
        assert st == _abi.A3D_INVALID_PARAMETER and n.value == SENTINEL, (hex(p), q and hex(q), hex(i))
    # an empty map extracts nothing into disjoint outputs, whatever the capacity, and needs no device
    for cap in (0, 4):
        n.value = SENTINEL
        assert lib.a3d_voxel_map_extract(with_n, C.c_void_p(pts), C.c_void_p(nrm), C.c_void_p(idx), cap,
                                         C.byref(n)) == _abi.A3D_OK and n.value == 0
    assert lib.a3d_voxel_map_extract(without_n, C.c_void_p(pts), None, None, 0, C.byref(n)) == _abi.A3D_OK and n.value == 0
    lib.a3d_voxel_map_free(with_n), lib.a3d_voxel_map_free(without_n)


def test_python_wrapper_refuses_host_clouds(lib):
    ctx = types.SimpleNamespace(lib=lib, handle=C.c_void_p(FAKE_CTX))
    m = DeviceVoxelMap(ctx, 0.05, origin=(0.1, 0.2, 0.3), normals=False, reserve_cells=16)
    assert m.insert_many([]) == []
    with pytest.raises(TypeError):
        m.insert(PointCloud([[1.0, 2.0, 3.0]]))
    with pytest.raises(TypeError):
        m.insert_many([PointCloud([[1.0, 2.0, 3.0]])], None)
    foreign = DevicePointCloud.__new__(DevicePointCloud)
    foreign.ctx, foreign.n, foreign.d_points, foreign.d_normals = object(), 0, None, None
    with pytest.raises(_abi.InvalidParameter):
        m.insert(foreign)
    with pytest.raises(_abi.InvalidParameter):
        DeviceVoxelMap(ctx, 0.05, origin=(0.0, 1.0))
    with pytest.raises(_abi.A3dError):
        DeviceVoxelMap(ctx, -1.0)
    assert m.stats() == EMPTY_STATS and m.cells() == 0 and m.total() == 0
    m.clear()
    m.free()
    m.free()


def _raw_cloud(seed, n):
    """[n, 3] f32 from raw bit patterns: a third of the rows any bits at all (NaN, infinities, huge magnitudes: dropped
    points), the rest with exponents forced into [2^-4, 2^4) so that many points share cells of a 0.25 grid."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32)
    tame = rng.random(n) >= 1 / 3
    exponent = rng.integers(123, 131, size=(n, 3), dtype=np.uint64).astype(np.uint32)
    bits[tame] = (bits[tame] & np.uint32(0x807FFFFF)) | (exponent[tame] << np.uint32(23))
    return bits.view(np.float32)


def _incremental(parts, voxel, origin):
    """Per key the minimum of bits(dist) << 32 | global index, kept part by part; a part's first point takes the number
    after the previous part's last, dropped points included.  Returns (ascending winner indices, dropped per part)."""
    best, total, dropped = {}, 0, []
    for part in parts:
        kept, key, dist = V.voxel_keys(part, voxel, origin)
        word = dist.view(np.uint32).astype(np.uint64) << np.uint64(32) | (np.arange(len(part), dtype=np.uint64) + np.uint64(total))
        for i in np.flatnonzero(kept):
            k, w = int(key[i]), int(word[i])
            if k not in best or w < best[k]:
                best[k] = w
        dropped.append(int((~kept).sum()))
        total += len(part)
    return np.sort(np.asarray([w & 0xFFFFFFFF for w in best.values()], np.uint64)).astype(np.uint32), dropped


@pytest.mark.parametrize("voxel,origin", [(0.25, None), (0.02, (0.013, -0.4, 7.5)), (1e3, None)])
def test_incremental_minima_over_any_partition_equal_the_downsample_of_the_whole(voxel, origin):
    cloud = _raw_cloud(7, 6000)
    kept, key, _ = V.voxel_keys(cloud, voxel, origin)
    assert 500 < (~kept).sum() < len(cloud) - 500  # points are dropped and points are kept
    whole, dropped = V.voxel_downsample(cloud, voxel, origin)
    assert len(whole) < kept.sum()  # cells are shared
    rng = np.random.default_rng(8)
    for k in (1, 2, 3, 7, 40):
        cuts = np.sort(rng.choice(np.arange(1, len(cloud)), size=k - 1, replace=False)) if k > 1 else []
        parts = np.split(cloud, cuts)
        assert len(parts) == k
        index, part_dropped = _incremental(parts, voxel, origin)
        assert np.array_equal(index, whole) and sum(part_dropped) == dropped
        assert part_dropped == [int((~kept[a:b]).sum()) for a, b in zip([0, *cuts], [*cuts, len(cloud)])]
    # numbering the kept points only (dropped ones consuming nothing) is another, wrong, convention
    first_dropped = int(np.flatnonzero(~kept)[0])
    assert (whole > first_dropped).any()


def test_generated_rust_bindings_hold_rust_types_only():
    """The map's `int with_normals` is the header's first plain C int: sys.rs declares it c_int, and the generator refuses
    a C scalar it has no Rust type for instead of passing its name through."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "scripts", "gen_rust_sys.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.rust_type("int") == "c_int" and gen.rust_type("const a3d_pose*") == "*const a3d_pose"
    for unknown in ("long", "unsigned", "int64_t*"):
        with pytest.raises(ValueError):
            gen.rust_type(unknown)
    text = gen.generate()
    assert text == open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    new = re.search(r"pub fn a3d_voxel_map_new\((.*?)\)", text).group(1)
    assert "with_normals: c_int" in new
    rust = {"u8", "u16", "u32", "u64", "i32", "usize", "f32", "f64", "c_char", "c_int", "c_void", "a3d_status"}
    declared = set(re.findall(r"pub (?:struct|type) (\w+)", text))
    extern = text[text.index('extern "C" {'):]
    for t in set(re.findall(r"(?::|->|\*const|\*mut) (\w+)", extern)) - {"const", "mut"}:
        assert t in rust or t in declared, t
