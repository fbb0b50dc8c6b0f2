"""The TSDF surface rule without a device: the committed marching-tetrahedra table against a derivation from the rule's
paragraph, what that table gives for every sign pattern of one cell and for a closed random field (through the numpy
restatement, tsdf_surface_restatement.py), hand-computed vertices, and the ABI of a3d_tsdf_volume_extract_surface /
a3d_tsdf_volume_upload."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tsdf_surface_restatement as S
from align3d_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a3d_tsdf_volume_extract_surface", "a3d_tsdf_volume_upload")
F = np.float32
INVALID = _abi.A3D_INVALID_PARAMETER
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


# ---- the table -------------------------------------------------------------------------------------------------------

def test_the_committed_table_is_the_one_the_rule_gives():
    derived = S.encode(S.derive_table())
    assert np.array_equal(S.committed_table(), derived)
    # what the count pass assumes: 0, 1 or 2 triangles by the number of inside vertices
    for t in range(6):
        for s in range(16):
            n = bin(s).count("1")
            assert int(derived[t, s]) & 3 == min(n, 4 - n) == len(S.TABLE[t][s])
    # the six tetrahedra tile the cell: each has volume 1 / 6, and all share the body diagonal
    for permutation in S.PERMUTATIONS:
        v = np.asarray(S.tetrahedron(permutation), np.float64)
        assert abs(abs(np.linalg.det(v[1:] - v[0])) - 1.0) < 1e-12
        assert tuple(v[0]) == (0, 0, 0) and tuple(v[3]) == (1, 1, 1)
    assert [S.tetrahedron(p)[1:3] for p in S.PERMUTATIONS] == [
        ((1, 0, 0), (1, 1, 0)), ((1, 0, 0), (1, 0, 1)), ((0, 1, 0), (1, 1, 0)), ((0, 1, 0), (0, 1, 1)), ((0, 0, 1), (1, 0, 1)),
        ((0, 0, 1), (0, 1, 1))]


def _cell_triangles(pattern):
    """The triangles of one unit cell whose corner c is inside iff bit c of `pattern`: corners as (owner, class)."""
    out = []
    for t, permutation in enumerate(S.PERMUTATIONS):
        s = 0
        for n, (x, y, z) in enumerate(S.tetrahedron(permutation)):
            s |= (pattern >> (x | y << 1 | z << 2) & 1) << n
        out += list(S.TABLE[t][s])
    return out


def _midpoint(corner):
    owner, c = corner
    return np.asarray(S.class_offset(owner), np.float64) + 0.5 * np.asarray(S.class_offset(c), np.float64)


@pytest.mark.parametrize("pattern", range(256))
def test_every_interior_triangle_edge_of_a_cell_is_used_twice_in_opposite_directions(pattern):
    triangles = _cell_triangles(pattern)
    uses = {}
    for tri in triangles:
        # every corner lies on an edge whose ends are on different sides
        for owner, c in tri:
            assert (pattern >> owner & 1) != (pattern >> (owner + c) & 1)
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            uses[a, b] = uses.get((a, b), 0) + 1
    for (a, b), count in uses.items():
        pa, pb = _midpoint(a), _midpoint(b)
        on_boundary = any((pa[axis] == side and pb[axis] == side) for axis in range(3) for side in (0.0, 1.0))
        if on_boundary:
            assert count == 1 and (b, a) not in uses  # the neighbouring cell has the other direction
        else:
            assert count == 1 and uses.get((b, a), 0) == 1, (pattern, a, b)
    if pattern in (0, 255):
        assert not triangles
    # outward: every triangle's normal points from the inside corners towards the outside ones
    for tri in triangles:
        p0, p1, p2 = (_midpoint(c) for c in tri)
        normal = np.cross(p1 - p0, p2 - p0)
        owner, c = tri[0]
        a = np.asarray(S.class_offset(owner), np.float64)
        step = np.asarray(S.class_offset(c), np.float64)
        outward = step if pattern >> owner & 1 else -step  # along the first corner's edge, from inside to outside
        assert np.dot(normal, outward) > 0


# ---- the restatement -------------------------------------------------------------------------------------------------

def _closed_field(seed):
    rng = np.random.default_rng(seed)
    D = rng.normal(size=(4, 5, 6)).astype(F)  # 6 x 5 x 4 voxels
    D[0] = D[-1] = 1
    D[:, 0] = D[:, -1] = 1
    D[:, :, 0] = D[:, :, -1] = 1
    return S.volume_of(D, np.ones_like(D), None, 0.1, (0.3, -0.2, 0.1))


def _euler_of_the_inside(vol):
    """V - E + F - T of the Kuhn triangulation's full subcomplex on the inside voxels, counted without any table: the
    surface bounds a neighbourhood of that complex, and the boundary of a compact 3-manifold has twice its Euler
    characteristic."""
    inside = S.valid_inside(vol, 1)[1]
    nz, ny, nx = inside.shape
    simplices = [set(), set(), set(), set()]
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                for permutation in S.PERMUTATIONS:
                    corners = [(i + x, j + y, k + z) for x, y, z in S.tetrahedron(permutation)]
                    kept = [c for c in corners if inside[c[2], c[1], c[0]]]
                    for size in range(1, len(kept) + 1):
                        for first in range(1 << len(kept)):
                            if bin(first).count("1") == size:
                                simplices[size - 1].add(tuple(c for n, c in enumerate(kept) if first >> n & 1))
    return len(simplices[0]) - len(simplices[1]) + len(simplices[2]) - len(simplices[3])


@pytest.mark.parametrize("seed", (0, 5))
def test_a_fully_valid_field_with_an_outside_boundary_gives_a_closed_outward_surface(seed):
    """Seed 0: the inside voxels form blobs without a tunnel, and V - E + F is 2 for every component.  Seed 5 has a tunnel
    (a legitimate closed surface of genus 1): there the sum over the components is checked against the inside voxels' own
    Euler characteristic, as it is for seed 0."""
    vol = _closed_field(seed)
    out = S.extract(vol)
    faces, n = out["faces"], len(out["points"])
    assert len(faces) > 50 and faces.max() < n
    assert S.closed_and_oriented(faces)
    assert len(np.unique(faces)) == n  # every vertex is used
    components = S.euler_by_component(faces, n)
    assert components and sum(components) == 2 * _euler_of_the_inside(vol), components
    if seed == 0:
        assert all(chi == 2 for chi in components), components
    assert S.signed_volume(out["points"], faces) > 0
    # the cloud form is the mesh's vertices of classes 1, 2 and 4, in the same order
    cloud = S.extract(vol, want_faces=False)
    keep = np.isin(out["cls"], S.CLOUD_CLASSES)
    assert cloud["faces"] is None and np.array_equal(cloud["points"].view(np.uint32), out["points"][keep].view(np.uint32))
    assert np.array_equal(cloud["normals"].view(np.uint32), out["normals"][keep].view(np.uint32))


def test_vertices_by_hand():
    """2 x 2 x 2, v = 0.5, origin (1, 2, 3): voxel 0 inside at D = -1, every other voxel outside at D = 3: seven crossing
    edges owned by voxel 0, each at t = 1 / 4; no normals (no sample at +-1 voxel fits into two voxels)."""
    D = np.full((2, 2, 2), 3, F)
    D[0, 0, 0] = -1
    C_ = np.arange(24, dtype=np.uint8).reshape(2, 2, 2, 3)
    out = S.extract(S.volume_of(D, np.ones_like(D), C_, 0.5, (1.0, 2.0, 3.0)))
    assert out["cls"].tolist() == [1, 2, 3, 4, 5, 6, 7] and not out["voxel"].any()
    want = [[1 + 0.125 * (c & 1), 2 + 0.125 * (c >> 1 & 1), 3 + 0.125 * (c >> 2 & 1)] for c in range(1, 8)]
    assert np.array_equal(out["points"], np.asarray(want, F))
    assert not out["normals"].view(np.uint32).any() and np.array_equal(out["colors"], np.tile(C_[0, 0, 0], (7, 1)))
    # one corner inside: one triangle per tetrahedron, six in all, on a closed fan round the corner
    assert len(out["faces"]) == 6 and S.signed_volume(out["points"] - F([1, 2, 3]), out["faces"]) > 0
    # min_weight 2 with W = 1 everywhere: nothing is valid
    assert len(S.extract(S.volume_of(D, np.ones_like(D), None, 0.5, (0, 0, 0)), min_weight=2)["points"]) == 0
    # -0 is inside, +0 too; an infinite D is not valid; a NaN neither
    D2 = np.full((2, 2, 2), 1, F)
    D2[0, 0, 0], D2[0, 0, 1], D2[0, 1, 0], D2[1, 0, 0] = -0.0, 0.0, np.inf, np.nan
    out = S.extract(S.volume_of(D2, np.ones_like(D2), None, 1.0, (0, 0, 0)))
    pairs = list(zip(out["voxel"].tolist(), out["cls"].tolist()))
    # voxel 0 (inside) against 3 (x+y), 5, 6, 7; voxel 1 (inside) against 3 (class 2), 5 (class 4), 7 (class 6)
    assert pairs == [(0, 3), (0, 5), (0, 6), (0, 7), (1, 2), (1, 4), (1, 6)]
    assert out["faces"].shape == (0, 3)  # the only cell has invalid corners


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_symbols_are_exported_declared_and_mirrored(lib):
    header = open(os.path.join(ROOT, "include", "align3d_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "align3d-hip", "src", "sys.rs")).read()
    diag = _abi.load_library(_abi.DIAG_LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert hasattr(diag, name), name
        assert re.search(r"a3d_status\s+%s\s*\(" % name, header), name
        assert name in _abi.SIGNATURES, name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert len(_abi.SIGNATURES["a3d_tsdf_volume_extract_surface"][1]) == 11
    assert len(_abi.SIGNATURES["a3d_tsdf_volume_upload"][1]) == 3
    assert lib.a3d_abi_version() == 1
    assert "mesh extraction, along-ray" not in header
    makefile = open(os.path.join(ROOT, "align3d_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btsdf_surface\.hip\b", makefile, re.M)
    import align3d_amd

    for method in ("extract_point_cloud", "extract_triangle_mesh", "upload"):
        assert callable(getattr(align3d_amd.DeviceTsdfVolume, method))
    for attribute in ("download", "free", "len_vertices"):
        assert hasattr(align3d_amd.DeviceTriangleMesh, attribute)


def _extract(lib, vol=0x30000, min_weight=1, want_faces=1, points=0x40000, normals=None, colors=None, vcap=10, faces=0x50000,
             fcap=10, counts=(True, True)):
    """On a made-up volume: every check under test fails before anything is dereferenced."""
    nv, nf = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    st = lib.a3d_tsdf_volume_extract_surface(C.c_void_p(vol) if vol else None, min_weight, want_faces, points, normals, colors,
                                             vcap, faces, fcap, C.byref(nv) if counts[0] else None,
                                             C.byref(nf) if counts[1] else None)
    return st, nv.value, nf.value


BAD = [dict(vol=0), dict(counts=(False, True)), dict(counts=(True, False)), dict(min_weight=0), dict(min_weight=(1 << 24) + 1),
       dict(min_weight=(1 << 64) - 1), dict(points=None), dict(points=None, vcap=0, normals=0x60000),
       dict(points=None, vcap=0, colors=0x60000), dict(faces=None), dict(points=None, vcap=0, faces=None, fcap=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_extracts_are_invalid_without_a_device(lib, bad):
    st, nv, nf = _extract(lib, **bad)
    assert st == INVALID
    assert nv == SENTINEL and nf == SENTINEL  # (the counts are untouched)


def test_upload_refuses_nulls_without_a_device(lib):
    assert lib.a3d_tsdf_volume_upload(None, C.c_void_p(0x40000), None) == INVALID
    assert lib.a3d_tsdf_volume_upload(C.c_void_p(0x30000), None, None) == INVALID
