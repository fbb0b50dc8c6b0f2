"""Every entry that keeps its working set in an open-addressing hash table, on clouds whose cells collide by construction.

The clouds are those of hash_collision_cases.py (test_hash_collision_cases_cpu.py proves what each is): one chain of half the
table that wraps, a wrapping chain of cells with content and satellites, two chains that merge, and a chain that survives
every growth of the map.  Every comparison is on bits against the numpy restatements (voxel_restatement,
voxel_mean_restatement, normals_restatement, outlier_restatement, cluster_restatement, voxel_map_icp_restatement,
voxel_map_mean_restatement), which know nothing of slots; the one tolerance is the 1e-4 rad / 1e-4 m that the suite holds
DeviceVoxelMap.align to against the restatement (its sums are not in the restatement's order), and later runs of an
alignment are compared with the first bit for bit.

Batch entries run alone, again, again after a3d_selftest_fill_scratch(0xFF), on a row permutation of the cloud (against the
restatement of the permuted cloud, and mapped back to the original rows where the result is documented as independent of the
row order), and as the middle job of three between two ordinary clouds, every job as if alone.  Both libraries.  A call
that reports a fault raises."""
import functools

import numpy as np
import pytest

import cluster_restatement as CR
import hash_collision_cases as H
import normals_restatement as NR
import oracle_lib as O
import outlier_restatement as OR
import scratch_cases as SC
import voxel_map_icp_restatement as R
import voxel_mean_restatement as VM
import voxel_restatement as V
from align3d_amd import DevicePointCloud, DeviceVoxelMap, IcpParams, PointCloud
from align3d_amd._abi import A3D_OK
from voxel_map_mean_restatement import MeanMapRestatement, retained_mean

pytestmark = pytest.mark.gpu

PITCH = H.PITCH
KS = (1, 8, 17)
MIN_NEIGHBORS, STAT_K, STD_RATIO = 3, 2, 1.0
MIN_POINTS = (1, 3)
MIN_SIZE = 4
ORDINARY = ((310, 600), (311, 1300))  # (seed, rows) of scratch_cases.scene: the jobs before and after the case
CASES = {c["name"]: c for c in H.batch_cases()}


@pytest.fixture(params=["product", "diagnostics"])
def lib_ctx(request):
    return request.getfixturevalue("ctx" if request.param == "product" else "diag_ctx")


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points, normals, colors) by name: a case, 'perm:' + a case, or 'ordinary0' / 'ordinary1'."""
    if name.startswith("ordinary"):
        seed, n = ORDINARY[int(name[-1])]
        p, nrm, col = SC.scene(seed, n)
        return (p * np.float32(0.5)).astype(np.float32), nrm, col  # a few rows per cell of the pitch
    if name.startswith("perm:"):
        return H.permuted(CASES[name[5:]])[1]
    return H.parts(CASES[name])


def _device(ctx, names, normals=True, colors=True):
    return [DevicePointCloud(ctx, PointCloud(p, n if normals else None, c if colors else None)) for p, n, c in map(cloud, names)]


def _words(ctx, d, n):
    return ctx.to_host(d, np.empty(n, np.uint32))


# ---- the groups: run(ctx, names) -> one dict per job; ref(name) -> the dict of that cloud alone ---------------------------------
def run_voxel(ctx, names):
    src = _device(ctx, names)
    thin, index = DevicePointCloud._voxel_downsample(src, PITCH, None, True)
    mean, mean_index, counts = DevicePointCloud._voxel_downsample(src, PITCH, None, True, "mean", True)
    outs = []
    for i in range(len(src)):
        out = {}
        SC._cloud_arrays(out, "nearest", thin[i], index[i])
        SC._cloud_arrays(out, "mean", mean[i], mean_index[i], counts[i])
        outs.append(out)
    SC._free(src, thin, mean)
    return outs


def ref_voxel(name):
    p, n, c = cloud(name)
    wp, wn, wi, _ = V.voxel_downsample_cloud(p, n, PITCH)
    out = {"nearest.points": SC._bits(wp), "nearest.normals": SC._bits(wn), "nearest.colors": c[wi],
           "nearest.index": wi.astype(np.uint32)}
    mp, mn, mc, mi, mk, _ = VM.voxel_mean(p, n, c, PITCH)
    out.update({"mean.points": SC._bits(mp), "mean.normals": SC._bits(mn), "mean.colors": mc, "mean.index": mi.astype(np.uint32),
                "mean.counts": mk.astype(np.uint32)})
    return out


def run_normals(ctx, names):
    src = _device(ctx, names, normals=False, colors=False)
    valid, curv, counts, dropped = DevicePointCloud.estimate_normals_many(src, PITCH, [H.EYE] * len(src), curvature=True,
                                                                          counts=True, dropped=True)
    outs = [{"valid": np.uint64(valid[i]), "dropped": np.uint64(dropped[i]), "normals": SC._bits(c.download()[1]),
             "curvature": SC._bits(curv[i]), "counts": counts[i]} for i, c in enumerate(src)]
    SC._free(src)
    return outs


def ref_normals(name):
    wn, wc, wk, wv = NR.estimate_normals(cloud(name)[0], PITCH, viewpoint=H.EYE)
    return {"valid": np.uint64(wv.sum()), "dropped": np.uint64((wk == 0).sum()), "normals": SC._bits(wn),
            "curvature": SC._bits(wc), "counts": wk.astype(np.uint32)}


def _stats_words(stats):
    return np.asarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in stats], np.uint64)


def run_knn(ctx, names):
    src = _device(ctx, names)
    outs = [{} for _ in src]
    for k in KS:
        d_counts, d_qsum, stats = DevicePointCloud.neighbor_distances_many(src, PITCH, k)
        for i, c in enumerate(src):
            outs[i][f"k{k}.counts"], outs[i][f"k{k}.qsum"] = _words(ctx, d_counts[i], c.len()), _words(ctx, d_qsum[i], c.len())
            outs[i][f"k{k}.stats"] = _stats_words(stats[i])
        for d in d_counts + d_qsum:
            ctx.free(d)
    SC._free(src)
    return outs


def ref_knn(name):
    out = {}
    for k in KS:
        counts, qsum, st = OR.knn_distance(cloud(name)[0], PITCH, k)
        out[f"k{k}.counts"], out[f"k{k}.qsum"] = counts.astype(np.uint32), qsum.astype(np.uint32)
        out[f"k{k}.stats"] = _stats_words((st[0], st[1], st[2] + (st[3] << 32)))
    return out


def run_outliers(ctx, names):
    src = _device(ctx, names)
    by_radius, ri = DevicePointCloud.remove_radius_outliers_many(src, PITCH, MIN_NEIGHBORS, return_index=True)
    by_stats, si = DevicePointCloud.remove_statistical_outliers_many(src, PITCH, STAT_K, STD_RATIO, return_index=True)
    outs = []
    for i in range(len(src)):
        out = {}
        SC._cloud_arrays(out, "radius", by_radius[i], ri[i])
        SC._cloud_arrays(out, "statistical", by_stats[i], si[i])
        outs.append(out)
    SC._free(src, by_radius, by_stats)
    return outs


def ref_outliers(name):
    parts, out = cloud(name), {}
    SC._rows(out, "radius", parts, OR.remove_radius_outliers(parts[0], PITCH, MIN_NEIGHBORS))
    SC._rows(out, "statistical", parts, OR.remove_statistical_outliers(parts[0], PITCH, STAT_K, STD_RATIO)[0])
    return out


def run_cluster(ctx, names):
    src = _device(ctx, names)
    outs = [{} for _ in src]
    for m in MIN_POINTS:
        d_labels, sizes, roots = DevicePointCloud.cluster_many(src, PITCH, m)
        for i, c in enumerate(src):
            outs[i][f"m{m}.labels"] = _words(ctx, d_labels[i], c.len())
            outs[i][f"m{m}.sizes"], outs[i][f"m{m}.roots"] = np.asarray(sizes[i], np.uint32), np.asarray(roots[i], np.uint32)
            ctx.free(d_labels[i])
    big, index = DevicePointCloud.remove_small_clusters_many(src, PITCH, MIN_POINTS[-1], MIN_SIZE, return_index=True)
    for i in range(len(src)):
        SC._cloud_arrays(outs[i], "big", big[i], index[i])
    SC._free(src, big)
    return outs


def ref_cluster(name):
    parts, out = cloud(name), {}
    for m in MIN_POINTS:
        c = CR.cluster(parts[0], PITCH, m)
        out[f"m{m}.labels"], out[f"m{m}.sizes"], out[f"m{m}.roots"] = c.labels, c.sizes, c.roots
    SC._rows(out, "big", parts, CR.remove_small_clusters(parts[0], PITCH, MIN_POINTS[-1], MIN_SIZE))
    return out


def _rows_sorted(out, tag):
    """The rows of a downsampled cloud as one sorted table: what does not depend on the order of the input rows."""
    table = np.concatenate([out[f"{tag}.points"].reshape(-1, 3), out[f"{tag}.normals"].reshape(-1, 3),
                            out[f"{tag}.colors"].reshape(-1, 3).astype(np.uint32), out[f"{tag}.counts"].reshape(-1, 1)], axis=1)
    return table[np.lexsort(table.T[::-1])]


def back_voxel(got, want, perm):
    assert np.array_equal(_rows_sorted(got, "mean"), _rows_sorted(want, "mean"))  # integer sums: the same means
    assert len(got["nearest.index"]) == len(want["nearest.index"])


def back_normals(got, want, perm):
    for name in ("normals", "curvature", "counts"):  # integer moments: the same bits per row
        assert np.array_equal(got[name], want[name][perm]), name
    assert got["valid"] == want["valid"]


def back_knn(got, want, perm):
    for k in KS:  # "the same for every order of the rows"
        assert np.array_equal(got[f"k{k}.counts"], want[f"k{k}.counts"][perm]), k
        assert np.array_equal(got[f"k{k}.qsum"], want[f"k{k}.qsum"][perm]), k
        assert np.array_equal(got[f"k{k}.stats"], want[f"k{k}.stats"]), k


def back_outliers(got, want, perm):
    for tag in ("radius", "statistical"):  # the same rows survive
        assert np.array_equal(np.sort(perm[got[f"{tag}.index"]]), want[f"{tag}.index"]), tag


def back_cluster(got, want, perm):
    a, b = got["m1.labels"], want["m1.labels"][perm]  # min_points = 1: connected components, numbered by their lowest row
    pairs = set(zip(a.tolist(), b.tolist()))
    assert len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
    assert np.array_equal(np.sort(got["m1.sizes"]), np.sort(want["m1.sizes"]))
    assert np.array_equal(np.sort(got["m3.sizes"]), np.sort(want["m3.sizes"]))
    assert np.array_equal(got["m3.labels"] == CR.NONE, (want["m3.labels"] == CR.NONE)[perm])


GROUPS = {"voxel": (run_voxel, ref_voxel, back_voxel), "normals": (run_normals, ref_normals, back_normals),
          "knn": (run_knn, ref_knn, back_knn), "outliers": (run_outliers, ref_outliers, back_outliers),
          "cluster": (run_cluster, ref_cluster, back_cluster)}


@functools.lru_cache(maxsize=None)
def reference(group, name):
    return GROUPS[group][1](name)


def _same(got, want, what):
    bad = SC.mismatches(got, want)
    assert not bad, (what, bad)


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", list(CASES))
def test_batch_entry_on_constructed_collisions(lib_ctx, name, group):
    run, _, back = GROUPS[group]
    want = reference(group, name)
    first = run(lib_ctx, [name])[0]
    _same(first, want, (name, group, "alone"))
    _same(run(lib_ctx, [name])[0], first, (name, group, "second run"))
    assert sum(lib_ctx.selftest_fill_scratch(0xFF)) > 0
    _same(run(lib_ctx, [name])[0], first, (name, group, "over 0xFF"))
    perm = H.permuted(CASES[name])[0]
    moved = run(lib_ctx, ["perm:" + name])[0]
    _same(moved, reference(group, "perm:" + name), (name, group, "permuted"))
    back(moved, want, perm)
    jobs = ["ordinary0", name, "ordinary1"]
    for job, got in zip(jobs, run(lib_ctx, jobs)):
        _same(got, reference(group, job), (name, group, "middle of three", job))


# ---- the map ------------------------------------------------------------------------------------------------------------------
def _extract_arrays(out, tag, m):
    if m.mode == "mean":
        c, index, counts = m.extract(return_index=True, return_counts=True)
        SC._cloud_arrays(out, tag, c, index, counts)
    else:
        c, index = m.extract(return_index=True)
        SC._cloud_arrays(out, tag, c, index)
    c.free()


def _downsample_ref(out, tag, parts, mode):
    """voxel_downsample(merge) of the rows that went in, in the map's mode."""
    p, n, c = parts
    if mode == "mean":
        mp, mn, mc, mi, mk, _ = VM.voxel_mean(p, n, c, PITCH)
        out[f"{tag}.points"], out[f"{tag}.normals"], out[f"{tag}.colors"] = SC._bits(mp), SC._bits(mn), mc
        out[f"{tag}.index"], out[f"{tag}.counts"] = mi.astype(np.uint32), mk.astype(np.uint32)
    else:
        wp, wn, wi, _ = V.voxel_downsample_cloud(p, n, PITCH)
        out[f"{tag}.points"], out[f"{tag}.normals"], out[f"{tag}.colors"] = SC._bits(wp), SC._bits(wn), c[wi]
        out[f"{tag}.index"] = wi.astype(np.uint32)


@pytest.mark.parametrize("mode", ["nearest", "mean"])
@pytest.mark.parametrize("last", [False, True])
def test_map_takes_one_chain_of_half_its_smallest_table(lib_ctx, mode, last):
    case = H.one_chain_half_full(6, last)
    want = {}
    _downsample_ref(want, "extract", H.parts(case), mode)
    runs = []
    for turn in range(3):
        if turn == 2:
            assert sum(lib_ctx.selftest_fill_scratch(0xFF)) > 0
        src = DevicePointCloud(lib_ctx, PointCloud(*H.parts(case)))
        m = DeviceVoxelMap(lib_ctx, PITCH, normals=True, colors=True, mode=mode)
        assert m.insert(src) == 0
        s = m.stats()
        assert (s["slots"], s["growths"], s["cells"], s["total"]) == (64, 0, 32, 32)
        got = {}
        _extract_arrays(got, "extract", m)
        _same(got, want, (case["name"], mode, turn))
        q = case["points"] + np.float32(0.01)
        seq, d2 = m.nearest(q)
        got["nearest.seq"], got["nearest.d2"] = seq, SC._bits(d2)
        runs.append(got)
        SC._free([src, m])
    model = (MeanMapRestatement(*H.parts(case), PITCH) if mode == "mean" else R.MapRestatement(*H.parts(case)[:2], PITCH))
    seq, d2, _ = model.nearest(case["points"] + np.float32(0.01))
    assert np.array_equal(runs[0]["nearest.seq"], seq) and np.array_equal(runs[0]["nearest.d2"], SC._bits(d2))
    assert not SC.mismatches(runs[1], runs[0]) and not SC.mismatches(runs[2], runs[0])


GROWTH = H.survives_growth()
ALIGN_TWIST = [0.002, -0.0015, 0.001, 0.004, -0.003, 0.002]


def _align_params():
    return IcpParams(max_iterations=1, max_normal_angle=4.0)  # (above pi: the normals are random)


def _queries(rows):
    """Queries around the stored rows, most of them around the colliding cells' neighbourhood; one far away."""
    rng = np.random.default_rng(29)
    chain = np.concatenate([GROWTH["frames"][0]["points"], GROWTH["frames"][6]["points"]])
    base = np.concatenate([chain[rng.integers(0, len(chain), 400)], rows[rng.integers(0, len(rows), 400)]])
    q = (base + rng.uniform(-0.06, 0.06, size=base.shape)).astype(np.float32)
    q[7] = (50.0, 50.0, 50.0)
    return q


def _align_source(rows, normals):
    """Every second stored row, a little off its place."""
    off = O.exp_se3(ALIGN_TWIST)
    return O.transform_points(off, rows[::2]), R.transform_normals(off, normals[::2])


def _mean_survivors(model, keep):
    """The readers' view of a map of means after a retain: the kept rows numbered 0 ... k-1, found under the keys of their
    cells (a mean may lie on a face of its cell: the key of the row itself would name the neighbour)."""
    s = R.MapRestatement.__new__(R.MapRestatement)
    s.voxel, s.origin = model.voxel, model.origin
    s.rows, s.normals = model.rows[keep], model.normals[keep]
    s.seq = np.arange(int(keep.sum()), dtype=model.seq.dtype)
    s.cells = {int(k): (i, i) for i, k in enumerate(model.row_keys[keep].tolist())}
    return s


@functools.lru_cache(maxsize=None)
def growth_reference(mode):
    """Everything growth_run returns, from the restatements; 'pose' is held within SC.POSE_BOUND."""
    out = {"slots": np.asarray(GROWTH["slots"], np.uint64)}
    for i in range(len(GROWTH["frames"])):
        _downsample_ref(out, f"frame{i}", H.merged_frames(GROWTH, i + 1), mode)
    p, n, c = H.merged_frames(GROWTH, len(GROWTH["frames"]))
    chain = set(H.cell_keys(GROWTH["chain_cells"]).tolist())
    if mode == "mean":
        model = MeanMapRestatement(p, n, c, PITCH)
        keep, removed, _, k, _ = retained_mean(model, box=GROWTH["box"])
        survivors = _mean_survivors(model, keep)
        out["retained.colors"], out["retained.counts"] = model.colors[keep], model.counts[keep].astype(np.uint32)
        assert (model.counts[keep] > 1).sum() == 16
    else:
        model = R.MapRestatement(p, n, PITCH)
        survivors, removed, _, k = R.retained(model, box=GROWTH["box"])
        keep = ((model.rows >= GROWTH["box"][0]) & (model.rows <= GROWTH["box"][1])).all(axis=1)
        out["retained.colors"] = c[model.seq][keep]
    assert len(chain & set(model.cells)) == 31 and len(chain & set(survivors.cells)) == 16 and int(keep.sum()) == k
    out["retained.points"], out["retained.normals"] = SC._bits(survivors.rows), SC._bits(survivors.normals)
    out["retained.index"] = np.arange(k, dtype=np.uint32)
    out["removed"] = np.asarray([removed, k, max(64, H.table_slots(k))], np.uint64)  # the table shrinks to fit
    seq, d2, row = survivors.nearest(_queries(survivors.rows))
    assert 200 < (row >= 0).sum() < len(row)
    out["nearest.seq"], out["nearest.d2"] = seq, SC._bits(d2)
    status, pose = survivors.align(*_align_source(survivors.rows, survivors.normals), _align_params().to_c())
    assert status == A3D_OK
    out["pose"] = np.frombuffer(bytes(pose), np.uint8).copy()
    return out


def growth_run(ctx, mode):
    m = DeviceVoxelMap(ctx, PITCH, normals=True, colors=True, mode=mode)
    out, slots = {}, []
    for i, frame in enumerate(GROWTH["frames"]):
        src = DevicePointCloud(ctx, PointCloud(*H.parts(frame)))
        assert m.insert(src) == 0
        src.free()
        slots.append(m.stats()["slots"])
        _extract_arrays(out, f"frame{i}", m)
    out["slots"] = np.asarray(slots, np.uint64)
    assert m.stats()["growths"] == 5
    removed = m.retain(box=GROWTH["box"])
    s = m.stats()
    assert s["cells"] == s["total"]
    out["removed"] = np.asarray([removed, s["cells"], s["slots"]], np.uint64)
    _extract_arrays(out, "retained", m)
    rows = out["retained.points"].view(np.float32).reshape(-1, 3)
    seq, d2 = m.nearest(_queries(rows))
    out["nearest.seq"], out["nearest.d2"] = np.asarray(seq, np.uint32), SC._bits(d2)
    sp, sn = _align_source(rows, out["retained.normals"].view(np.float32).reshape(-1, 3))
    moved = DevicePointCloud(ctx, PointCloud(sp, sn))
    out["pose"] = np.frombuffer(bytes(m.align(moved, _align_params()).to_c()), np.uint8).copy()
    SC._free([moved, m])
    return out


@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_map_chain_survives_growth_retain_and_is_read(lib_ctx, mode):
    want = growth_reference(mode)
    first = growth_run(lib_ctx, mode)
    bad = SC.mismatches(first, want, poses=("pose",))
    assert not bad, (mode, bad)
    assert not SC.mismatches(growth_run(lib_ctx, mode), first), (mode, "second run")
    assert sum(lib_ctx.selftest_fill_scratch(0xFF)) > 0
    assert not SC.mismatches(growth_run(lib_ctx, mode), first), (mode, "over 0xFF")


@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_map_stored_slot_form_gives_the_same_bits(diag_ctx, monkeypatch, mode):
    want = growth_reference(mode)
    got = {}
    for form in ("1", "0"):
        monkeypatch.setenv("A3D_VOXEL_MAP_STORED_SLOT", form)
        got[form] = growth_run(diag_ctx, mode)
        bad = SC.mismatches(got[form], want, poses=("pose",))
        assert not bad, (mode, form, bad)
    assert not SC.mismatches(got["1"], got["0"]), mode
