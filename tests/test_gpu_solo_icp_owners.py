"""The three single-job point-cloud ICPs on one context, interleaved: DeviceVoxelMap.align, DeviceTsdfVolume.align and
Icp.align run through one host driver over one kind of working state (csrc/solo_icp.hpp), a SoloIcp per handle.

What each of them computes is checked where it always was (test_gpu_voxel_map_icp.py, test_gpu_tsdf_icp.py,
test_gpu_pcl_icp.py).  Here: nothing of that state is shared between handles or depends on what ran before.  Every call
is first made on a handle that has done nothing else, then repeated between calls of the other owners, behind an
accumulate of its own owner, and behind an align of another source length (another number of blocks, so other rows of
the partial buffers); every repeat returns the first answer bit for bit, and the timer of a handle moves with its own
aligns only.  The scenes are those of the owners' own tests: the 3 000-point map and the 5 000-point source of
test_gpu_voxel_map_icp.py, the corner volume and its source of test_gpu_tsdf_icp.py, an Icp on the map's merged cloud."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import tsdf_icp_restatement as TR
import voxel_map_icp_restatement as VR
from align3d_amd import DevicePointCloud, DeviceTsdfVolume, DeviceVoxelMap, Icp, IcpParams, PointCloud, Transform, _abi
from gpu_util import small_pose

pytestmark = pytest.mark.gpu

VOXEL = 0.05
ORIGIN = (0.013, -0.4, 0.021)
FULL, SHORT = 5000, 1025  # five blocks of 1024 threads, and two
PRM = IcpParams(max_iterations=5)


def _inverse(pose):
    out = _abi.PoseC()
    O.load().orc_inverse(C.byref(pose), C.byref(out))
    return out


def _moved(pose, points, normals):
    return O.transform_points(pose, points), VR.transform_normals(pose, normals)


class _Owner:
    """One kind of handle with its sources: `make()` gives a fresh handle, the three calls take a handle and a length."""

    def __init__(self, make, align, accumulate):
        self.make, self._align, self._accumulate = make, align, accumulate
        self.handle = make()

    def align(self, m, handle=None):
        return bytes(self._align(self.handle if handle is None else handle, m).to_c())

    def accumulate(self, m=FULL):
        g = self._accumulate(self.handle, m)
        return g["H"].tobytes(), g["g"].tobytes(), g["ssq"].tobytes(), g["count"]

    def fresh_align(self, m):
        handle = self.make()
        try:
            return self.align(m, handle)
        finally:
            handle.free()

    def ms(self):
        return self.handle.last_device_ms()


@pytest.fixture(scope="module")
def owners(ctx):
    offset = small_pose(7, rot=0.01, trans=0.01).to_c()
    at = small_pose(3, rot=0.005, trans=0.005)  # where the accumulations are taken: not the identity
    clouds = []

    def resident(points, normals):
        clouds.append(DevicePointCloud(ctx, PointCloud(points, normals)))
        return clouds[-1]

    # the map of test_gpu_voxel_map_icp.py: three clouds under three poses, and the source a small pose away
    world_p, world_n = VR.surfaces(1, 3000)
    poses = [O.exp_se3(u) for u in ([0.5, -0.3, 0.2, 0.3, -0.2, 0.1], [-0.4, 0.1, 0.6, -0.1, 0.25, 0.3],
                                    [0.1, 0.7, -0.5, 0.2, 0.2, -0.3])]
    parts = [resident(*_moved(_inverse(T), world_p[k::3], world_n[k::3])) for k, T in enumerate(poses)]
    map_p, map_n = _moved(_inverse(offset), *VR.surfaces(5, FULL, noise=0.002))
    map_src = {m: resident(map_p[:m], map_n[:m]) for m in (FULL, SHORT)}

    def new_map():
        vmap = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN)
        assert vmap.insert_many(parts, [Transform.from_c(T) for T in poses]) == [0, 0, 0]
        return vmap

    # the volume of test_gpu_tsdf_icp.py
    restated = TR.corner_volume()
    vol_p, vol_n = _moved(_inverse(offset), *TR.corner_surfaces(5, FULL))
    vol_src = {m: resident(vol_p[:m], vol_n[:m]) for m in (FULL, SHORT)}

    def new_volume():
        vol = DeviceTsdfVolume(ctx, (restated.nx, restated.ny, restated.nz), float(restated.v), restated.origin,
                               truncation=float(restated.tau))
        vol.upload(restated.D, restated.W)
        return vol

    # Icp on the cloud the map was made of (its accumulate takes the source from host memory)
    target = PointCloud(world_p, world_n)

    made = {
        "map": _Owner(new_map, lambda h, m: h.align(map_src[m], PRM), lambda h, m: h.accumulate(map_src[m], PRM, at)),
        "volume": _Owner(new_volume, lambda h, m: h.align(vol_src[m], PRM), lambda h, m: h.accumulate(vol_src[m], PRM, at)),
        "icp": _Owner(lambda: Icp(ctx, PRM, target), lambda h, m: h.align(map_src[m]),
                      lambda h, m: h.accumulate(PointCloud(map_p[:m], map_n[:m]), at)),
    }
    yield made
    for owner in made.values():
        owner.handle.free()
    for c in clouds:
        c.free()


def test_interleaved_owners_repeat_their_own_answers_bit_for_bit(owners):
    vmap, volume, icp = owners["map"], owners["volume"], owners["icp"]
    eye = bytes(Transform.eye().to_c())
    first, first_sums, ms = {}, {}, {}
    for name, owner in owners.items():  # the baselines, and: a timer moves with its own handle's aligns only
        assert owner.ms() == 0.0
        first[name] = owner.align(FULL)
        assert first[name] != eye and owner.ms() > 0.0
        ms[name] = owner.ms()
        first_sums[name] = owner.accumulate()
        assert first_sums[name][3] > 0 and owner.ms() == ms[name]
        for other in set(ms) - {name}:
            assert owners[other].ms() == ms[other], (name, other)
    short = {name: owner.fresh_align(SHORT) for name, owner in owners.items()}
    assert all(short[name] not in (eye, first[name]) for name in owners)
    for name in owners:  # (the fresh handles were other handles)
        assert owners[name].ms() == ms[name]

    assert vmap.align(FULL) == first["map"]
    assert volume.align(FULL) == first["volume"]
    assert icp.align(FULL) == first["icp"]
    assert volume.accumulate() == first_sums["volume"]  # between two aligns of the volume
    assert volume.align(SHORT) == short["volume"]       # two blocks behind five
    assert vmap.align(SHORT) == short["map"]
    assert vmap.accumulate() == first_sums["map"]
    assert vmap.align(FULL) == first["map"]             # five behind two, behind an accumulate
    assert icp.align(SHORT) == short["icp"]
    assert icp.accumulate() == first_sums["icp"]
    assert icp.align(FULL) == first["icp"]
    assert volume.align(FULL) == first["volume"]
    assert vmap.accumulate(SHORT) != first_sums["map"] and vmap.accumulate() == first_sums["map"]
    assert all(owner.ms() > 0.0 for owner in owners.values())
