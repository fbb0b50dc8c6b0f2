"""The launch geometry of voxel_map_icp.hip at the sizes the product runs: sources longer than one trip of the
grid-stride loops, num_cus partials per iteration, both halves of the partial double buffer at their real offsets.

B = ctx.num_cus().  The ICP's kernel, solo_icp_head_kernel over MapTarget (csrc/pcl_icp.hpp, voxel_map_icp.hip),
launches min(ceil(m / 1024), B) blocks of 1024 threads, so one trip serves S_icp = 1024 B points; voxel_map_nearest_kernel launches min(ceil(m / 256), 8 B) blocks of 256, S_near = 2048 B.  Both
are derived from the device here, and every test that means to take a second trip asserts m > S.  The map is the scene
of test_gpu_voxel_map_icp.py; the source is its 5 000-point source repeated with period P, S % P != 0, so that an index
wrong by one stride lands on another query and changes the answer.  Expected values: the association and the per-point
terms of ONE period by voxel_map_icp_restatement.py, indexed (PeriodicSource; test_voxel_map_sparse_restatement_cpu.py
holds it to the plain computation).  Bounds: `nearest` bit for bit; count exact; H and ssq within the project's 1e-6 of
the f64 sums of the restated f32 terms; g in the form of test_gpu_full_size.py for the same engine at 500 k points
(against the size of its terms, since g cancels near convergence; under eye also against max |g|); poses within the
project's 1e-4 rad / 1e-4 m of the restatement's run, whose orc_gn_steps sums in f32 as the reference does."""
import numpy as np
import pytest

import oracle_lib as O
import voxel_map_icp_restatement as R
from align3d_amd import IcpParams, Transform, _abi
from gpu_util import gn_rel_err, small_pose, transform_diff
from test_gpu_voxel_map_icp import NONE, _Scene, _assert_nearest, _assert_pose, _bits, _dev

pytestmark = pytest.mark.gpu

TRIPS = ("S - 1", "S", "S + 1", "2 S + ragged")
FAR = np.float32([50.0, -40.0, 30.0])  # metres away from the scene: no row within 27 cells


class _Geometry:
    """The strides of the device, the period, and the repeated source on the host and on the device."""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene
        self.blocks = ctx.num_cus()
        assert self.blocks >= 1
        self.s_icp, self.s_near = 1024 * self.blocks, 2048 * self.blocks
        self.period = 5000 if self.s_icp % 5000 and self.s_near % 5000 else 4999
        assert self.s_icp % self.period != 0 and self.s_near % self.period != 0
        self.p, self.n = scene.src_p[:self.period], scene.src_n[:self.period]
        self._clouds = {}

    def sizes(self, stride, ragged):
        return dict(zip(TRIPS, (stride - 1, stride, stride + 1, 2 * stride + ragged)))

    def host(self, m):
        reps = -(-m // self.period)
        return np.tile(self.p, (reps, 1))[:m], np.tile(self.n, (reps, 1))[:m]

    def cloud(self, m):
        if m not in self._clouds:
            self._clouds[m] = _dev(self.ctx, *self.host(m))
        return self._clouds[m]

    def view(self, model, m):
        return R.PeriodicSource(model, m)

    def free(self):
        for c in self._clouds.values():
            c.free()
        self._clouds = {}


@pytest.fixture(scope="module")
def scene():
    return _Scene()


@pytest.fixture(scope="module")
def vmap(ctx, scene):
    m = scene.new_map(ctx)
    assert m.cells() == len(scene.model.rows) > 1000
    yield m
    m.free()


@pytest.fixture(scope="module")
def geo(ctx, scene):
    g = _Geometry(ctx, scene)
    yield g
    g.free()


def _shifted_differs(a, stride):
    """An answer read one stride too early or too late is another answer: the array is not its own shift by `stride`."""
    return len(a) > stride and not np.array_equal(a[stride:], a[:len(a) - stride])


@pytest.mark.parametrize("trip", TRIPS)
def test_nearest_over_full_grids_and_further_trips(scene, vmap, geo, trip):
    m = geo.sizes(geo.s_near, 257)[trip]
    if trip in TRIPS[2:]:
        assert m > geo.s_near  # the second trip is really taken (and the third, ragged one, by the last size)
    if trip == TRIPS[3]:
        assert m > 2 * geo.s_near and (m - 2 * geo.s_near) % 256 != 0
    cloud = geo.cloud(m)
    for name, pose in (("no pose", None), ("under a pose", O.exp_se3([0.02, -0.03, 0.01, 0.01, 0.02, -0.015]))):
        want = geo.view(scene.model, m).nearest(geo.p, pose)
        assert (want[2] >= 0).sum() > 0.9 * m
        if m > geo.s_near:
            assert _shifted_differs(want[0], geo.s_near) and _shifted_differs(_bits(want[1]), geo.s_near)
        _assert_nearest(vmap.nearest(cloud, None if pose is None else Transform.from_c(pose)), want, (trip, name))


def _assert_sums(gpu, ref, what, from_eye):
    eh, eg, es = gn_rel_err(gpu, ref)
    # g against the size of what it sums, |g_i| <= sqrt(H_ii * sum r^2): the form of test_gpu_full_size.py
    hd = np.sqrt(np.diag(np.asarray(ref["H"], np.float64).reshape(6, 6)) * float(ref["ssq"]))
    eg_terms = float(np.max(np.abs(np.asarray(gpu["g"], np.float64) - np.asarray(ref["g"], np.float64)) / hd))
    print(f"accumulate {what}: count {gpu['count']} / {ref['count']}, rel err H {eh:.3g} g {eg:.3g} ssq {es:.3g}, "
          f"g against its terms {eg_terms:.3g}")
    assert gpu["count"] == ref["count"], (what, gpu["count"], ref["count"])
    assert eh < 1e-6 and es < 1e-6 and eg_terms < 1e-6 and (eg < 1e-6 or not from_eye), (what, eh, eg, es, eg_terms)


@pytest.mark.parametrize("trip", TRIPS)
def test_accumulate_over_num_cus_partials_and_further_trips(scene, vmap, geo, trip):
    m = geo.sizes(geo.s_icp, 1025)[trip]
    if trip in TRIPS[2:]:
        assert m > geo.s_icp
    if trip == TRIPS[3]:
        assert m > 2 * geo.s_icp and (m - 2 * geo.s_icp) % 1024 != 0
    prm = IcpParams(max_iterations=5)
    cloud = geo.cloud(m)
    for name, T in (("eye", Transform.eye()), ("small pose", small_pose(2))):
        ref = geo.view(scene.model, m).accumulate(geo.p, geo.n, T.to_c(), prm.to_c())
        assert ref["count"] > 0.5 * m
        _assert_sums(vmap.accumulate(cloud, prm, T), ref, f"m={m} ({trip}) {name}", name == "eye")


@pytest.mark.parametrize("run", ["default x5", "weight 0.7 x3"])
def test_align_over_both_halves_of_the_partial_buffer(scene, vmap, geo, run):
    m = geo.s_icp + 1
    assert m > geo.s_icp  # B blocks, B partials per half, a second trip
    prm = IcpParams(max_iterations=5) if run == "default x5" else IcpParams(max_iterations=3, weight=0.7)
    status, want = geo.view(scene.model, m).align(geo.p, geo.n, prm.to_c())
    assert status == _abi.A3D_OK
    got = vmap.align(geo.cloud(m), prm)
    _assert_pose(got, want, f"m={m} {run}")
    assert vmap.last_device_ms() > 0.0
    ang, tr = transform_diff(got, scene.offset)  # the alignment finds the pose the source was moved by
    assert ang < 2e-3 and tr < 2e-3, (ang, tr)


def test_rows_and_pose_do_not_depend_on_the_table_at_full_geometry(ctx, scene, vmap, geo):
    m_icp, m_near = geo.s_icp + 1, geo.s_near + 1
    assert m_icp > geo.s_icp and m_near > geo.s_near
    prm = IcpParams(max_iterations=5)
    src, q = geo.cloud(m_icp), geo.cloud(m_near)
    first_rows, first_pose = vmap.nearest(q), vmap.align(src, prm)
    want = geo.view(scene.model, m_near).nearest(geo.p)
    _assert_nearest(first_rows, want, "one call")
    renumbered = scene.model.renumbered()
    want_renumbered = geo.view(renumbered, m_near).nearest(geo.p)
    assert np.array_equal(want_renumbered[2], want[2]) and not np.array_equal(want_renumbered[0], want[0])
    for how, kw in (("frame by frame", {}), ("one call", {"reserve_cells": 1 << 16})):
        m = scene.new_map(ctx, how, **kw)
        assert m.stats()["slots"] != vmap.stats()["slots"] or how == "frame by frame"
        _assert_nearest(m.nearest(q), first_rows, how)
        assert bytes(m.align(src, prm).to_c()) == bytes(first_pose.to_c()), how
        assert m.compact() == 0 and m.total() == m.cells()
        _assert_nearest(m.nearest(q), want_renumbered, how + ", after compact")  # the same rows under their ranks
        assert bytes(m.align(src, prm).to_c()) == bytes(first_pose.to_c()), how + ", after compact"
        m.free()


def test_points_without_a_cell_contribute_nothing_in_any_trip(ctx, scene, vmap, geo):
    """Every point beyond the first stride lies metres away from the map (finite): its 27 probes find nothing, its lanes
    read slot 0 unconditionally, and neither the sums nor another query's answer may see that."""
    prm = IcpParams(max_iterations=5)
    # the ICP kernel: three trips, the second and the third without a single correspondence
    m = 2 * geo.s_icp + 1025
    assert m > 2 * geo.s_icp
    p, n = geo.host(m)
    p = p.copy()
    p[geo.s_icp:] += FAR
    assert np.isfinite(p).all()
    assert (scene.model.nearest(geo.p + FAR)[2] < 0).all()  # by the restatement: no moved point finds a row
    long_cloud, first_stride = _dev(ctx, p, n), geo.cloud(geo.s_icp)
    for name, T in (("eye", Transform.eye()), ("small pose", small_pose(2))):
        ref = geo.view(scene.model, geo.s_icp).accumulate(geo.p, geo.n, T.to_c(), prm.to_c())
        got, alone = vmap.accumulate(long_cloud, prm, T), vmap.accumulate(first_stride, prm, T)
        _assert_sums(got, ref, f"far tail, m={m} {name}", name == "eye")
        assert got["count"] == alone["count"] == ref["count"] > 0.5 * geo.s_icp
        for key in ("H", "g"):  # the same blocks and threads add the same terms in the same order
            assert np.array_equal(_bits(got[key]), _bits(alone[key])), (name, key)
        assert np.float32(got["ssq"]) == np.float32(alone["ssq"]), name
    long_cloud.free()
    # the nearest kernel: NONE / +inf for exactly the moved queries
    m = 2 * geo.s_near + 257
    assert m > 2 * geo.s_near
    q = geo.host(m)[0].copy()
    q[geo.s_near:] += FAR
    seq, d2, row = geo.view(scene.model, m).nearest(geo.p)
    seq, d2 = seq.copy(), d2.copy()
    seq[geo.s_near:], d2[geo.s_near:] = NONE, np.float32(np.inf)
    assert (row[:geo.s_near] >= 0).sum() > 0.9 * geo.s_near
    cloud = _dev(ctx, q)
    _assert_nearest(vmap.nearest(cloud), (seq, d2), "far tail")
    cloud.free()
