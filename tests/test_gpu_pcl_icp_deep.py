"""GPU parity of point-cloud ICP (src/icp/pcl_icp.rs) on a target tree deeper than the LDS split table, and through
every descent shape of pcl_point_loop by the diagnostics build's launch knobs (A3D_PCL_*, fixed at Icp::new)."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib as O
from align3d_amd import DevicePointCloud, Icp, IcpParams, PointCloud, Transform
from align3d_amd._abi import PoseC
from data_util import uniform01
from gpu_util import gn_rel_err, oracle_frame, small_pose, to_range_image, transform_diff

pytestmark = pytest.mark.gpu


def _oracle_accumulate(prm, tree, tgt, src, T):
    g = O.GnStateC()
    tv, sv = O.pcl_view(tgt.points, tgt.normals), O.pcl_view(src.points, src.normals)
    p, t = prm.to_c(), T.to_c()
    assert O.load().orc_pcl_icp_accumulate(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(t), 1, C.byref(g)) == 0
    return g.as_dict()


def _check_accumulate(icp, prm, tree, tgt, src, T, what):
    ref = _oracle_accumulate(prm, tree, tgt, src, T)
    gpu = icp.accumulate(src, T)
    assert gpu["count"] == ref["count"] and ref["count"] > 1000, (what, gpu["count"], ref["count"])
    eh, eg, es = gn_rel_err(gpu, ref)
    assert eh < 1e-6 and eg < 1e-6 and es < 1e-6, (what, eh, eg, es)


def _height_field(n, seed):
    """z = 0.2 sin(2x) cos(3y) + 0.05 x y at random (x, y) in [-1, 1]^2, with its analytic unit normals."""
    xy = (uniform01(seed, 2 * n).reshape(n, 2).astype(np.float64) * 2.0 - 1.0)
    x, y = xy[:, 0], xy[:, 1]
    z = 0.2 * np.sin(2 * x) * np.cos(3 * y) + 0.05 * x * y
    zx = 0.4 * np.cos(2 * x) * np.cos(3 * y) + 0.05 * y
    zy = -0.6 * np.sin(2 * x) * np.sin(3 * y) + 0.05 * x
    nrm = np.stack([-zx, -zy, np.ones_like(x)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], axis=1).astype(np.float32), nrm.astype(np.float32)


@pytest.fixture(scope="module")
def deep_clouds():
    n = 1_100_000  # depth 17: 78 % of the nodes at depth 16 are inner
    pts, nrm = _height_field(n, 31)
    tgt = PointCloud(pts, nrm)
    pick = np.sort(np.random.default_rng(32).choice(n, 300_001, replace=False))
    move = small_pose(5, rot=0.01, trans=0.01).to_c()
    src = PointCloud(O.transform_points(move, pts[pick]), _transform_normals(move, nrm[pick]))
    tree = O.KdTree(pts)
    assert tree.stats()[2] == 17
    return tgt, src, tree


def _transform_normals(p, n):
    out = np.empty_like(n)
    O.load().orc_transform_normals(C.byref(p), O.ptr(n), n.size // 3, O.ptr(out))
    return out


def test_pcl_icp_deep_target_accumulate_and_align(ctx, deep_clouds):
    t0 = time.perf_counter()
    tgt, src, tree = deep_clouds
    prm = IcpParams(max_iterations=10)
    icp = Icp.new(ctx, prm, tgt)
    for T in (Transform.eye(), small_pose(1), small_pose(2)):
        _check_accumulate(icp, prm, tree, tgt, src, T, "host arrays")
    out = PoseC()
    tv, sv = O.pcl_view(tgt.points, tgt.normals), O.pcl_view(src.points, src.normals)
    p = prm.to_c()
    assert O.load().orc_pcl_icp_align(C.byref(p), tree.h, C.byref(tv), C.byref(sv), C.byref(out), None) == 0
    T_host = icp.align(src)
    ang, tr = transform_diff(T_host, out)
    print(f"[pcl icp deep target, {tgt.len()} <- {src.len()}] d_angle={ang:.3e} d_trans={tr:.3e}")
    assert ang <= 1e-4 and tr <= 1e-4
    # the same clouds resident in HBM: the same pose, bit for bit
    d_tgt, d_src = DevicePointCloud(ctx, tgt), DevicePointCloud(ctx, src)
    try:
        T_dev = Icp.new(ctx, prm, d_tgt).align(d_src)
    finally:
        d_tgt.free()
        d_src.free()
    a, b = T_host.to_c(), T_dev.to_c()
    assert list(a.t) + list(a.q) == list(b.t) + list(b.q), (list(a.t) + list(a.q), list(b.t) + list(b.q))
    print(f"[pcl icp deep target] {time.perf_counter() - t0:.1f} s")


_PCL_KNOBS = ("A3D_PCL_LDS_LEVELS", "A3D_PCL_BLOCK", "A3D_PCL_BLOCKS_PER_CU")


@pytest.fixture(scope="module")
def sample1_clouds():
    tgt = PointCloud.from_range_image(to_range_image(oracle_frame("sample1", 0, True)))
    src = PointCloud.from_range_image(to_range_image(oracle_frame("sample1", 1, True)))
    return tgt, src, O.KdTree(tgt.points)


@pytest.mark.parametrize("levels", [0, 1, 2, 7, 13])
@pytest.mark.parametrize("block", [256, 512])
def test_pcl_icp_every_descent_shape(diag_ctx, monkeypatch, sample1_clouds, levels, block):
    tgt, src, tree = sample1_clouds
    prm = IcpParams(max_iterations=5)
    for per_cu in (1, 4):  # (changes the number of partials: the sums are checked against the bound, not for equal bits)
        env = {"A3D_PCL_LDS_LEVELS": str(levels), "A3D_PCL_BLOCK": str(block), "A3D_PCL_BLOCKS_PER_CU": str(per_cu)}
        for k in _PCL_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            icp = Icp.new(diag_ctx, prm, tgt)  # the launch geometry is fixed here
        finally:
            for k in env:
                monkeypatch.delenv(k, raising=False)
        for T in (Transform.eye(), small_pose(2)):
            _check_accumulate(icp, prm, tree, tgt, src, T, env)
        icp.free()
