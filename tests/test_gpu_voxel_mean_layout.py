"""voxel_mean.hip at the edges of its runs, waves, trips and tiles, on the GPU: the recipes of voxel_mean_cases.py, whose
layout in the kernels is known on the host (tests/test_voxel_mean_cases_cpu.py states what each of them reaches).

As in test_gpu_voxel_mean.py, whose helpers are used unchanged: every expected value is the numpy restatement
(voxel_mean_restatement.voxel_mean), never the library; every comparison is bit for bit on uint32 / uint8 views; every
call goes through the raw ABI into canary-guarded buffers, and whatever the call did not have to write must still hold the
canary.  No tolerance appears.  Every test prints its wall time."""
import time

import numpy as np
import pytest

import voxel_mean_cases as K
import voxel_mean_restatement as M
from align3d_amd import _abi
from test_gpu_voxel_mean import FIELDS, _assert_matches, _call, _device_cloud

pytestmark = pytest.mark.gpu

ORIGIN = (0.013, -0.4, 7.5)


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"[wall time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


def _full_and_bare(ctx, points, normals, colors, voxel, origin=None, label=""):
    """One cloud, once with all five outputs and once bare (points only: no normals, colours, index or counts), against
    the restatement."""
    expected = M.voxel_mean(points, normals, colors, voxel, origin)
    full, bare = _device_cloud(ctx, points, normals, colors), _device_cloud(ctx, points)
    st, lens, dropped, outs = _call(ctx, [full], voxel, origin)
    assert st == _abi.A3D_OK, label
    assert all(outs[0][f] is not None for f in FIELDS), label
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    st, lens, dropped, outs = _call(ctx, [bare], voxel, origin, index=False, counts=False)
    assert st == _abi.A3D_OK and all(outs[0][f] is None for f in FIELDS[1:]), label
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    full.free(), bare.free()
    return expected


def _same_bits(a, b, label):
    for name in FIELDS:
        assert (a[name] is None and b[name] is None) or np.array_equal(a[name], b[name]), (label, name)


@pytest.mark.parametrize("drop_every", [0, K.DROP_EVERY], ids=["every row kept", "rows dropped"])
def test_uniform_runs_over_the_whole_table(ctx, drop_every):
    """K runs of L in the sorted records: run j starts at j * L, so every start lane, every run that ends on lane 63,
    starts on lane 63, covers a whole wave, crosses a block trip or a tile is met; with dropped rows kept < len, the last
    wave of pass 5 is ragged and the last tile lies behind kept."""
    for L, k in K.RUN_TABLE:
        points, normals, colors = K.uniform_runs(L, k, 1, drop_every)
        expected = _full_and_bare(ctx, points, normals, colors, K.VOXEL, label=(L, k))
        assert (expected[4] == L).all() and len(expected[4]) == k and expected[5] == len(points) - L * k
    # under an origin the cells differ and the counts are no longer equal: the same code, another layout
    points, normals, colors = K.uniform_runs(129, 67, 1, drop_every)
    _full_and_bare(ctx, points, normals, colors, K.VOXEL, ORIGIN, label="origin")


def test_scanline_and_sorted_inputs(ctx):
    """Runs of equal keys in INPUT order (passes 1 and 4): a row-major plane wider than a wave and one narrower, the same
    with NaN points inside the runs, and an input sorted by cell with runs of 1 to 130."""
    for w, h in K.SCANLINE_SHAPES:
        for nan_every in (0, 11):
            points, normals, colors = K.scanline(w, h, nan_every=nan_every)
            expected = _full_and_bare(ctx, points, normals, colors, K.VOXEL, label=(w, h, nan_every))
            assert (expected[5] > 0) == (nan_every > 0) and expected[4].max() > 10
    points, normals, colors = K.sorted_runs()
    expected = _full_and_bare(ctx, points, normals, colors, K.VOXEL, label="sorted")
    assert expected[4][:len(K.RUN_CYCLE)].tolist() == list(K.RUN_CYCLE)


def test_edges_of_the_arithmetic(ctx):
    """rintf ties, colour halves and thirds, normals that cancel to L == 0, the first and the last cell of the key range,
    points on a cell face: what test_voxel_mean_cpu.py asks of the restatement, asked of the device."""
    for case in K.edge_arithmetic():
        _full_and_bare(ctx, case["points"], case["normals"], case["colors"], case["voxel"], case["origin"], label=case["name"])


def test_table_as_one_batch_equals_single_calls_and_runs_are_identical(ctx):
    hosts = [K.uniform_runs(L, k, 2, K.DROP_EVERY if i % 2 else 0) for i, (L, k) in enumerate(K.RUN_TABLE)]
    clouds = [_device_cloud(ctx, *h) for h in hosts]
    runs = [_call(ctx, clouds, K.VOXEL, None) for _ in range(2)]
    for st, lens, dropped, outs in runs:
        assert st == _abi.A3D_OK
        for out, got_len, got_dropped, h in zip(outs, lens, dropped, hosts):
            _assert_matches(out, got_len, got_dropped, M.voxel_mean(*h, K.VOXEL))
    assert runs[0][1:3] == runs[1][1:3]
    for i, (a, b) in enumerate(zip(runs[0][3], runs[1][3])):
        _same_bits(a, b, f"two runs, cloud {i}")
    for i, cloud in enumerate(clouds):
        st, lens, dropped, outs = _call(ctx, [cloud], K.VOXEL, None)
        assert st == _abi.A3D_OK and (lens[0], dropped[0]) == (runs[0][1][i], runs[0][2][i])
        _same_bits(outs[0], runs[0][3][i], f"cloud {i} alone")
    for c in clouds:
        c.free()


def test_capacity_one_short_of_a_uniform_runs_cloud(ctx):
    points, normals, colors = K.uniform_runs(65, 67, 3, K.DROP_EVERY)
    cloud = _device_cloud(ctx, points, normals, colors)
    expected = M.voxel_mean(points, normals, colors, K.VOXEL)
    rows = len(expected[3])
    assert rows == 67
    st, lens, dropped, outs = _call(ctx, [cloud], K.VOXEL, None, capacities=[rows - 1])
    assert st == _abi.A3D_INVALID_PARAMETER
    assert lens == [rows] and dropped == [expected[5]] and expected[5] > 0
    for name in FIELDS:
        assert (outs[0][name] == outs[0][name + "_canary"]).all(), name
    st, lens, dropped, outs = _call(ctx, [cloud], K.VOXEL, None, capacities=[rows])  # exactly enough is enough
    assert st == _abi.A3D_OK
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    cloud.free()


def test_pass_3_slot_shares(ctx):
    """4097 points in 3 cells: 5 tiles share 16384 slots of which 3 are occupied, so most shares are empty and a share is
    no multiple of 256 slots; 1025 points each alone in its cell: as many cells as points."""
    expected = _full_and_bare(ctx, *K.few_cells(4097, 3), K.VOXEL, label="3 cells")
    assert len(expected[4]) == 3 and expected[4].sum() == 4097
    expected = _full_and_bare(ctx, *K.all_alone(1025), K.VOXEL, label="alone")
    assert (expected[4] == 1).all() and np.array_equal(expected[3], np.arange(1025, dtype=np.uint32))


def test_stale_scratch_between_a_large_and_a_small_call(ctx):
    """The scratch region is reused from call to call and only the hash tables and the spill accumulators are zeroed: a
    small call that follows a large one, and the large one again, find the other's records, flags and row numbers."""
    large = K.uniform_runs(1025, 5, 4, K.DROP_EVERY)
    small = (K.uniform_runs(33, 2, 4)[0][:65], None, None)  # 65 points in 2 cells
    exp_large, exp_small = M.voxel_mean(*large, K.VOXEL), M.voxel_mean(*small, K.VOXEL)
    assert sorted(exp_small[4].tolist()) == [32, 33] and exp_large[4].tolist() == [1025] * 5
    d_large, d_small = _device_cloud(ctx, *large), _device_cloud(ctx, *small)
    for cloud, expected in ((d_large, exp_large), (d_small, exp_small), (d_large, exp_large), (d_small, exp_small)):
        st, lens, dropped, outs = _call(ctx, [cloud], K.VOXEL, None)
        assert st == _abi.A3D_OK
        _assert_matches(outs[0], lens[0], dropped[0], expected)
    d_large.free(), d_small.free()
