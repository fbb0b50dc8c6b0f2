"""The case table of the scratch-independence tests (test_gpu_scratch_independence.py, test_scratch_cases_cpu.py).

One entry per operation that works in the context's grow-only scratch regions or takes pooled memory: the regions it uses
(and, as 6 / 7, the pooled image arenas / spare blocks it takes), run(ctx, which) -> {name: host array} through the public
wrappers with EVERY output downloaded, and reference(which) -> the same names from the numpy restatement the suite
already has for that operation (never the code under test).  DESIGN.md section 5 has the audit these cases go with.

Every case has two seeded inputs.  "S" is the smallest at which the kernels take every path (a cloud of two chunks, one
of one row, rows that are dropped, duplicates); "L" is about eight to ten times larger, lies over the same coordinate
range (its cell keys, hash slots, rows and pixels collide with S's) and has another batch size, so that every part of
the region's layout starts somewhere else and what L leaves behind lies under every part S uses."""
import functools
from collections import namedtuple

import numpy as np

F = np.float32
LENGTHS = {"S": (1500, 548, 1), "L": (9000, 6000, 3000, 2010, 1)}  # 2049 rows in 3 clouds, 20011 in 5
IMAGES = {"S": ((37, 101), (64, 48)), "L": ((160, 120),)}             # (width, height)
VOXEL, ORIGIN = 0.25, (0.1, -0.05, 0.02)
RADIUS, K, MIN_NEIGHBORS, STD_RATIO = 0.15, 8, 6, 1.0
CLUSTER_RADIUS, CLUSTER_MIN_POINTS, CLUSTER_MIN_SIZE = 0.1, 4, 20
PLANE_T, PLANE_H, PLANE_SEED, PLANE_REFINE = 0.02, 64, 3, 2
RENDER_RADIUS = 0.05
BOX = (F([-0.8, -2.0, -0.5]), F([0.9, 0.6, 2.0]))
CHUNK = 1024  # rows per chunk of every tiled cloud kernel (VX_CHUNK, CO_CHUNK, VM_CHUNK, CLOUD_CHUNK)
CLUMPS = F([[0.6, 0.6, 0.7], [-0.6, 0.5, -0.6], [0.5, -0.6, -0.7], [-0.55, -0.6, 0.75]])

Case = namedtuple("Case", "regions run reference reference_name")


def scene(seed, n):
    """(points [n, 3] f32, normals, colors [n, 3] u8) in [-1, 1]^3: half the rows on a thin slab (a plane with inliers and
    outliers), four tenths in four clumps (clusters), the rest scattered (noise); from 16 rows on, two rows that every
    grid drops and four rows that are copies of others (ties)."""
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * 2 - 1).astype(F)
    kind = rng.random(n)
    slab = kind < 0.5
    pts[slab, 2] = (F(0.1) * pts[slab, 0] + F(0.25) + (rng.random(int(slab.sum())) * 0.02 - 0.01)).astype(F)
    clump = (kind >= 0.5) & (kind < 0.9)
    which = rng.integers(0, len(CLUMPS), int(clump.sum()))
    pts[clump] = (CLUMPS[which] + (rng.random((int(clump.sum()), 3)) * 0.25 - 0.125)).astype(F)
    if n >= 16:
        at = rng.permutation(n)[:10]
        pts[at[:4]] = pts[at[4:8]]
        pts[at[8]], pts[at[9]] = (np.nan, 0.0, 1.0), (np.inf, 0.5, -1.0)
    nrm = (rng.random((n, 3)) * 2 - 1).astype(F)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), F(1e-3)).astype(F)
    return pts, nrm.astype(F), rng.integers(0, 256, (n, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def clouds(which):
    """The batch of `which`: [(points, normals, colors)], one entry per cloud of LENGTHS[which]."""
    base = 100 if which == "S" else 200
    return [scene(base + i, n) for i, n in enumerate(LENGTHS[which])]


def merged(which):
    """The clouds of the batch back to back: what a voxel map holds after they went in."""
    parts = clouds(which)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def layout(which):
    """An APPROXIMATION of the sizes of region 3's parts for this batch, restated by hand from the library's rules (slots =
    the power of two at or above 2 n, every part padded to 256 bytes): it is not read from the library and would not follow
    a change of its sizing.  `jobs` and `rows` stand for the parts that scale with them (job-table bytes, the 64-bit words
    per job, spill accumulators per 64 rows).  A sanity check that L is the larger input in every respect, no more."""
    lens = LENGTHS[which]
    slots = [max(2, 1 << int(np.ceil(np.log2(2 * n)))) for n in lens]
    pad = lambda b: (b + 255) // 256 * 256  # noqa: E731
    return {"jobs": len(lens), "tiles": sum((n + CHUNK - 1) // CHUNK for n in lens),
            "ballot_bytes": sum(pad((n + 63) // 64 * 8) for n in lens), "table_bytes": 16 * sum(slots),
            "record_bytes": sum(pad(16 * n) for n in lens), "row_bytes": sum(pad(4 * n) for n in lens),
            "rows": sum(lens), "pixels": sum(w * h for w, h in IMAGES[which])}


def poses(which):
    import oracle_lib as O

    return [O.exp_se3([0.3 - 0.1 * i, -0.2, 0.1 * i, 0.4, 0.5 - 0.2 * i, 0.3]) for i in range(len(LENGTHS[which]))]


def cameras(which):
    from align3d_amd import CameraIntrinsics

    return [CameraIntrinsics(1.1 * w + 0.37, 1.0 * h, w / 2 - 0.5, h / 2 + 0.25, w, h) for w, h in IMAGES[which]]


TIE_ROWS = (5, 700)  # two rows of the render cloud at one place in front of everything else: an equal-depth tie in view


def render_cloud(which):
    """The first cloud of the batch, pushed in front of the camera, with TIE_ROWS both on the optical axis nearer than
    any other row: they compete for the same pixels at the same depth, and the lower row must win them."""
    p, n, c = clouds(which)[0]
    p = (p + F([0.0, 0.0, 2.5])).astype(F)
    p[list(TIE_ROWS)] = F([0.0, 0.0, 1.25])
    return p, n, c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _device(ctx, which, normals=True, colors=True):
    from align3d_amd import DevicePointCloud, PointCloud

    return [DevicePointCloud(ctx, PointCloud(p, n if normals else None, c if colors else None)) for p, n, c in clouds(which)]


def _free(*groups):
    for g in groups:
        for c in g:
            c.free()


def _cloud_arrays(out, tag, cloud, index=None, counts=None):
    p, n = cloud.download()
    out[f"{tag}.points"] = _bits(p)
    if n is not None:
        out[f"{tag}.normals"] = _bits(n)
    if cloud.has_colors():
        c = cloud.download_colors()
        out[f"{tag}.colors"] = c if c is not None else np.zeros((0, 3), np.uint8)
    if index is not None:
        out[f"{tag}.index"] = np.asarray(index, np.uint32)
    if counts is not None:
        out[f"{tag}.counts"] = np.asarray(counts, np.uint32)


def _rows(out, tag, parts, rows):
    """The reference of a compaction that keeps `rows` of a cloud, bit for bit."""
    p, n, c = parts
    out[f"{tag}.points"], out[f"{tag}.normals"], out[f"{tag}.colors"] = _bits(p[rows]), _bits(n[rows]), c[rows]
    out[f"{tag}.index"] = np.asarray(rows, np.uint32)


# ---- transform_many, merge ---------------------------------------------------------------------------------------------
def run_transform(ctx, which):
    from align3d_amd import DevicePointCloud, Transform

    src = _device(ctx, which)
    ts = [Transform.from_c(p) for p in poses(which)]
    moved = DevicePointCloud.transform_many(src, ts)
    one = DevicePointCloud.merge(src, ts)
    out = {}
    for i, m in enumerate(moved):
        _cloud_arrays(out, f"moved{i}", m)
    _cloud_arrays(out, "merged", one)
    _free(src, moved, [one])
    return out


def ref_transform(which):
    import oracle_lib as O
    from voxel_map_icp_restatement import transform_normals

    out, parts = {}, []
    for i, ((p, n, c), pose) in enumerate(zip(clouds(which), poses(which))):
        tp, tn = O.transform_points(pose, p), transform_normals(pose, n)
        out[f"moved{i}.points"], out[f"moved{i}.normals"], out[f"moved{i}.colors"] = _bits(tp), _bits(tn), c
        parts.append((tp, tn, c))
    for k, name in enumerate(("points", "normals", "colors")):
        out[f"merged.{name}"] = _bits(np.concatenate([x[k] for x in parts]))
    return out


# ---- voxel_downsample_many, both modes -------------------------------------------------------------------------------------
def run_voxel_nearest(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which)
    thin, index = DevicePointCloud._voxel_downsample(src, VOXEL, ORIGIN, True)
    out = {}
    for i, (t, ix) in enumerate(zip(thin, index)):
        _cloud_arrays(out, f"thin{i}", t, ix)
    _free(src, thin)
    return out


def ref_voxel_nearest(which):
    import voxel_restatement as V

    out = {}
    for i, (p, n, c) in enumerate(clouds(which)):
        wp, wn, wi, _ = V.voxel_downsample_cloud(p, n, VOXEL, ORIGIN)
        out[f"thin{i}.points"], out[f"thin{i}.normals"], out[f"thin{i}.index"] = _bits(wp), _bits(wn), wi.astype(np.uint32)
        out[f"thin{i}.colors"] = c[wi]
    return out


def run_voxel_mean(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which)
    thin, index, counts = DevicePointCloud._voxel_downsample(src, VOXEL, ORIGIN, True, "mean", True)
    out = {}
    for i, (t, ix, k) in enumerate(zip(thin, index, counts)):
        _cloud_arrays(out, f"mean{i}", t, ix, k)
    _free(src, thin)
    return out


def ref_voxel_mean(which):
    import voxel_mean_restatement as VM

    out = {}
    for i, (p, n, c) in enumerate(clouds(which)):
        wp, wn, wc, wi, wk, _ = VM.voxel_mean(p, n, c, VOXEL, ORIGIN)
        out[f"mean{i}.points"], out[f"mean{i}.normals"], out[f"mean{i}.colors"] = _bits(wp), _bits(wn), wc
        out[f"mean{i}.index"], out[f"mean{i}.counts"] = wi.astype(np.uint32), wk.astype(np.uint32)
    return out


# ---- estimate_normals_many -------------------------------------------------------------------------------------------------
def run_normals(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which, normals=False, colors=False)
    eyes = [(0.5, -1.0, 4.0)] * len(src)
    valid, curv, counts, dropped = DevicePointCloud.estimate_normals_many(src, RADIUS, eyes, curvature=True, counts=True,
                                                                          dropped=True)
    out = {"valid": np.asarray(valid, np.uint64), "dropped": np.asarray(dropped, np.uint64)}
    for i, c in enumerate(src):
        out[f"normals{i}"], out[f"curvature{i}"], out[f"counts{i}"] = _bits(c.download()[1]), _bits(curv[i]), counts[i]
    _free(src)
    return out


def ref_normals(which):
    import normals_restatement as NR

    out, valid, dropped = {}, [], []
    for i, (p, _, _) in enumerate(clouds(which)):
        wn, wc, wk, wv = NR.estimate_normals(p, RADIUS, viewpoint=(0.5, -1.0, 4.0))
        out[f"normals{i}"], out[f"curvature{i}"], out[f"counts{i}"] = _bits(wn), _bits(wc), wk.astype(np.uint32)
        valid.append(int(wv.sum())), dropped.append(int((wk == 0).sum()))
    out["valid"], out["dropped"] = np.asarray(valid, np.uint64), np.asarray(dropped, np.uint64)
    return out


# ---- neighbor_distances_many, the two outlier filters ------------------------------------------------------------------------
def run_outliers(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which)
    d_counts, d_qsum, stats = DevicePointCloud.neighbor_distances_many(src, RADIUS, K)
    out = {"stats": np.asarray([[int(v) & 0xFFFFFFFFFFFFFFFF for v in s] for s in stats], np.uint64)}
    for i, c in enumerate(src):
        out[f"counts{i}"] = ctx.to_host(d_counts[i], np.empty(c.len(), np.uint32))
        out[f"qsum{i}"] = ctx.to_host(d_qsum[i], np.empty(c.len(), np.uint32))
    for d in d_counts + d_qsum:
        ctx.free(d)
    by_radius, ri = DevicePointCloud.remove_radius_outliers_many(src, RADIUS, MIN_NEIGHBORS, return_index=True)
    by_stats, si = DevicePointCloud.remove_statistical_outliers_many(src, RADIUS, K, STD_RATIO, return_index=True)
    for i in range(len(src)):
        _cloud_arrays(out, f"radius{i}", by_radius[i], ri[i])
        _cloud_arrays(out, f"statistical{i}", by_stats[i], si[i])
    _free(src, by_radius, by_stats)
    return out


def ref_outliers(which):
    import outlier_restatement as R

    out, stats = {}, []
    for i, parts in enumerate(clouds(which)):
        counts, qsum, st = R.knn_distance(parts[0], RADIUS, K)
        out[f"counts{i}"], out[f"qsum{i}"] = counts.astype(np.uint32), qsum.astype(np.uint32)
        stats.append([int(v) & 0xFFFFFFFFFFFFFFFF for v in (st[0], st[1], st[2] + (st[3] << 32))])
        _rows(out, f"radius{i}", parts, R.remove_radius_outliers(parts[0], RADIUS, MIN_NEIGHBORS))
        _rows(out, f"statistical{i}", parts, R.remove_statistical_outliers(parts[0], RADIUS, K, STD_RATIO)[0])
    out["stats"] = np.asarray(stats, np.uint64)
    return out


# ---- cluster_many, remove_small_clusters_many ---------------------------------------------------------------------------------
def run_cluster(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which)
    d_labels, sizes, roots = DevicePointCloud.cluster_many(src, CLUSTER_RADIUS, CLUSTER_MIN_POINTS)
    out = {}
    for i, c in enumerate(src):
        out[f"labels{i}"] = ctx.to_host(d_labels[i], np.empty(c.len(), np.uint32))
        out[f"sizes{i}"], out[f"roots{i}"] = np.asarray(sizes[i], np.uint32), np.asarray(roots[i], np.uint32)
        ctx.free(d_labels[i])
    big, index = DevicePointCloud.remove_small_clusters_many(src, CLUSTER_RADIUS, CLUSTER_MIN_POINTS, CLUSTER_MIN_SIZE,
                                                             return_index=True)
    for i in range(len(src)):
        _cloud_arrays(out, f"big{i}", big[i], index[i])
    _free(src, big)
    return out


def ref_cluster(which):
    import cluster_restatement as R

    out = {}
    for i, parts in enumerate(clouds(which)):
        c = R.cluster(parts[0], CLUSTER_RADIUS, CLUSTER_MIN_POINTS)
        out[f"labels{i}"], out[f"sizes{i}"], out[f"roots{i}"] = c.labels, c.sizes, c.roots
        _rows(out, f"big{i}", parts, R.remove_small_clusters(parts[0], CLUSTER_RADIUS, CLUSTER_MIN_POINTS, CLUSTER_MIN_SIZE))
    return out


# ---- segment_plane_many with refine, split_plane_many ---------------------------------------------------------------------------
def run_plane(ctx, which):
    from align3d_amd import DevicePointCloud

    src = _device(ctx, which)
    planes, d_flags, inliers = DevicePointCloud.segment_plane_many(src, PLANE_T, PLANE_H, PLANE_SEED, PLANE_REFINE)
    out = {"planes": _bits(np.asarray(planes, np.float64)), "inliers": np.asarray(inliers, np.uint64)}
    for i, c in enumerate(src):
        out[f"flags{i}"] = ctx.to_host(d_flags[i], np.empty(c.len(), np.uint32))
        ctx.free(d_flags[i])
    planes2, on, rest, on_rows, rest_rows = DevicePointCloud.split_plane_many(src, PLANE_T, PLANE_H, PLANE_SEED, PLANE_REFINE,
                                                                              return_index=True)
    out["split.planes"] = _bits(np.asarray(planes2, np.float64))
    for i in range(len(src)):
        _cloud_arrays(out, f"on{i}", on[i], on_rows[i])
        _cloud_arrays(out, f"rest{i}", rest[i], rest_rows[i])
    _free(src, on, rest)
    return out


def ref_plane(which):
    import plane_restatement as PR

    out, planes, inliers = {}, [], []
    for i, parts in enumerate(clouds(which)):
        seg = PR.segment(parts[0], PR.hypotheses(PLANE_SEED, len(parts[0]), PLANE_H), PLANE_T, PLANE_REFINE)
        planes.append(np.asarray(seg.plane, np.float64)), inliers.append(int(seg.inliers))
        out[f"flags{i}"] = np.asarray(seg.flags, np.uint32)
        _rows(out, f"on{i}", parts, np.flatnonzero(seg.flags == 1))
        _rows(out, f"rest{i}", parts, np.flatnonzero(seg.flags == 0))
    out["planes"] = out["split.planes"] = _bits(np.asarray(planes, np.float64))
    out["inliers"] = np.asarray(inliers, np.uint64)
    return out


# ---- DeviceVoxelMap, both modes: insert_many, extract, nearest, retain, compact --------------------------------------------------
def queries(which):
    p = merged(which)[0]
    rng = np.random.default_rng(7 if which == "S" else 8)
    q = (p[::3] + (rng.random((len(p[::3]), 3)) * 0.4 - 0.2)).astype(F)
    q[3] = (50.0, 50.0, 50.0)
    return q


def run_map_nearest(ctx, which):
    from align3d_amd import DeviceVoxelMap

    src = _device(ctx, which)
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, normals=True, colors=True)
    out = {"dropped": np.asarray(m.insert_many(src), np.uint64)}
    cloud, index = m.extract(return_index=True)
    _cloud_arrays(out, "extract", cloud, index)
    seq, d2 = m.nearest(queries(which))
    out["nearest.seq"], out["nearest.d2"] = np.asarray(seq, np.uint32), _bits(d2)
    removed = m.retain(box=BOX, min_seq=LENGTHS[which][0] // 2)
    kept, kept_index = m.extract(return_index=True)
    _cloud_arrays(out, "retained", kept, kept_index)
    removed2 = m.compact()
    again, again_index = m.extract(return_index=True)
    _cloud_arrays(out, "compacted", again, again_index)
    out["removed"] = np.asarray([removed, removed2, m.total()], np.uint64)
    _free(src, [cloud, kept, again, m])
    return out


def ref_map_nearest(which):
    import voxel_map_icp_restatement as R
    import voxel_restatement as V

    p, n, c = merged(which)
    model = R.MapRestatement(p, n, VOXEL, ORIGIN)
    out = {"dropped": np.asarray([int((~V.voxel_keys(x[0], VOXEL, ORIGIN)[0]).sum()) for x in clouds(which)], np.uint64)}
    out["extract.points"], out["extract.normals"] = _bits(model.rows), _bits(model.normals)
    out["extract.index"], out["extract.colors"] = model.seq.astype(np.uint32), c[model.seq]
    seq, d2, _ = model.nearest(queries(which))
    out["nearest.seq"], out["nearest.d2"] = seq, _bits(d2)
    keep = ((model.rows >= BOX[0]) & (model.rows <= BOX[1])).all(axis=1) & (model.seq >= LENGTHS[which][0] // 2)
    k = int(keep.sum())
    for tag in ("retained", "compacted"):
        out[f"{tag}.points"], out[f"{tag}.normals"] = _bits(model.rows[keep]), _bits(model.normals[keep])
        out[f"{tag}.colors"], out[f"{tag}.index"] = c[model.seq][keep], np.arange(k, dtype=np.uint32)
    out["removed"] = np.asarray([len(model.rows) - k, 0, k], np.uint64)
    return out


def run_map_mean(ctx, which):
    from align3d_amd import DeviceVoxelMap

    src = _device(ctx, which)
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, normals=True, colors=True, mode="mean")
    out = {"dropped": np.asarray(m.insert_many(src), np.uint64)}
    cloud, index, counts = m.extract(return_index=True, return_counts=True)
    _cloud_arrays(out, "extract", cloud, index, counts)
    m.compact()
    again, again_index, again_counts = m.extract(return_index=True, return_counts=True)
    _cloud_arrays(out, "compacted", again, again_index, again_counts)
    _free(src, [cloud, again, m])
    return out


def ref_map_mean(which):
    import voxel_mean_restatement as VM
    import voxel_restatement as V

    p, n, c = merged(which)
    wp, wn, wc, wi, wk, _ = VM.voxel_mean(p, n, c, VOXEL, ORIGIN)
    out = {"dropped": np.asarray([int((~V.voxel_keys(x[0], VOXEL, ORIGIN)[0]).sum()) for x in clouds(which)], np.uint64)}
    for tag, index in (("extract", wi.astype(np.uint32)), ("compacted", np.arange(len(wi), dtype=np.uint32))):
        out[f"{tag}.points"], out[f"{tag}.normals"], out[f"{tag}.colors"] = _bits(wp), _bits(wn), wc
        out[f"{tag}.index"], out[f"{tag}.counts"] = index, wk.astype(np.uint32)
    return out


# ---- DevicePointCloud.render, DeviceVoxelMap.render ------------------------------------------------------------------------------
def _image_arrays(out, tag, image, index, cam):
    host = image.download(normals=image.has_normals(), intensity=False, colors=image.has_colors())
    out[f"{tag}.points"], out[f"{tag}.mask"], out[f"{tag}.index"] = _bits(host.points), host.mask, index
    if host.normals is not None:
        out[f"{tag}.normals"] = _bits(host.normals)
    if host.colors is not None:  # the image's own 3 * w * h bytes: the slack behind them is nobody's
        out[f"{tag}.colors"] = np.ascontiguousarray(host.colors).reshape(cam.height, cam.width, 3)
    image.free()


def run_render(ctx, which):
    from align3d_amd import DevicePointCloud, PointCloud

    p, n, c = render_cloud(which)
    cloud = DevicePointCloud(ctx, PointCloud(p, n, c))
    out = {}
    for i, cam in enumerate(cameras(which)):
        image, index = cloud.render(cam, None, RENDER_RADIUS, return_index=True)
        _image_arrays(out, f"image{i}", image, index, cam)
    cloud.free()
    return out


def _ref_render(out, tag, p, n, c, cam):
    import render_restatement as RR

    want = RR.render(p, n, c, None, F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy), cam.width, cam.height, RENDER_RADIUS)
    out[f"{tag}.points"], out[f"{tag}.mask"], out[f"{tag}.index"] = _bits(want["points"]), want["mask"], want["index"]
    out[f"{tag}.normals"], out[f"{tag}.colors"] = _bits(want["normals"]), want["colors"]


def ref_render(which):
    out = {}
    for i, cam in enumerate(cameras(which)):
        _ref_render(out, f"image{i}", *render_cloud(which), cam)
    return out


def run_map_render(ctx, which):
    from align3d_amd import DevicePointCloud, DeviceVoxelMap, PointCloud

    p, n, c = render_cloud(which)
    cloud = DevicePointCloud(ctx, PointCloud(p, n, c))
    m = DeviceVoxelMap(ctx, VOXEL / 4, origin=ORIGIN, normals=True, colors=True)
    m.insert(cloud)
    out = {}
    for i, cam in enumerate(cameras(which)):
        image, index = m.render(cam, None, RENDER_RADIUS, return_index=True)
        _image_arrays(out, f"image{i}", image, index, cam)
    _free([cloud, m])
    return out


def ref_map_render(which):
    import voxel_restatement as V

    p, n, c = render_cloud(which)
    wp, wn, wi, _ = V.voxel_downsample_cloud(p, n, VOXEL / 4, ORIGIN)
    out = {}
    for i, cam in enumerate(cameras(which)):
        _ref_render(out, f"image{i}", wp, wn, c[wi], cam)
    return out


# ---- DevicePointCloud.from_range_images with colours -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def images(which):
    """[(points [h, w, 3], normals, mask [h, w] u8 with about six pixels in ten set, colors [h, w, 3] u8)] per IMAGES[which]."""
    out = []
    for i, (w, h) in enumerate(IMAGES[which]):
        rng = np.random.default_rng((300 if which == "S" else 400) + i)
        pts, nrm = ((rng.random((h, w, 3)) * 2 - 1).astype(F) for _ in range(2))
        mask = (rng.random((h, w)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
        mask[-1, -1], mask[0, 0] = 2, 0
        out.append((pts, nrm, mask, rng.integers(0, 256, (h, w, 3)).astype(np.uint8)))
    return out


def run_from_images(ctx, which):
    from align3d_amd import CameraIntrinsics, DevicePointCloud, DeviceRangeImage, RangeImage

    resident = []
    for pts, nrm, mask, rgb in images(which):
        h, w = mask.shape
        host = RangeImage(pts, mask, CameraIntrinsics(500.0, 500.0, w / 2, h / 2, w, h), normals=nrm)
        resident.append(DeviceRangeImage(ctx, host).set_colors(rgb))
    made = DevicePointCloud.from_range_images(resident, colors=True)
    out = {}
    for i, c in enumerate(made):
        _cloud_arrays(out, f"cloud{i}", c)
    _free(made, resident)
    return out


def ref_from_images(which):
    out = {}
    for i, (pts, nrm, mask, rgb) in enumerate(images(which)):
        keep = mask.reshape(-1) != 0  # row-major, the kept pixels in order
        out[f"cloud{i}.points"], out[f"cloud{i}.normals"] = _bits(pts.reshape(-1, 3)[keep]), _bits(nrm.reshape(-1, 3)[keep])
        out[f"cloud{i}.colors"] = rgb.reshape(-1, 3)[keep]
    return out


# ---- DeviceVoxelMap.align ---------------------------------------------------------------------------------------------------
ALIGN_ITERATIONS = 4


def align_source(which):
    """The first cloud of the batch, moved a little off the map it is part of."""
    import oracle_lib as O
    from voxel_map_icp_restatement import transform_normals

    p, n, _ = clouds(which)[0]
    off = O.exp_se3([0.01, -0.008, 0.006, 0.01, -0.012, 0.008])
    return O.transform_points(off, p), transform_normals(off, n)


def _align_params():
    from align3d_amd import IcpParams

    return IcpParams(max_iterations=ALIGN_ITERATIONS, max_normal_angle=4.0)  # (above pi: the scene's normals are random)


def run_map_align(ctx, which):
    from align3d_amd import DevicePointCloud, DeviceVoxelMap, PointCloud

    src = _device(ctx, which, colors=False)
    m = DeviceVoxelMap(ctx, VOXEL, origin=ORIGIN, normals=True)
    m.insert_many(src)
    sp, sn = align_source(which)
    moved = DevicePointCloud(ctx, PointCloud(sp, sn))
    pose = m.align(moved, _align_params())
    out = {"pose": np.frombuffer(bytes(pose.to_c()), np.uint8).copy()}
    _free(src, [moved, m])
    return out


def ref_map_align(which):
    import voxel_map_icp_restatement as R
    from align3d_amd._abi import A3D_OK

    p, n, _ = merged(which)
    status, pose = R.MapRestatement(p, n, VOXEL, ORIGIN).align(*align_source(which), _align_params().to_c())
    assert status == A3D_OK
    return {"pose": np.frombuffer(bytes(pose), np.uint8).copy()}


# The reference of an alignment is the restatement's pose within the bound the suite already holds DeviceVoxelMap.align
# to (test_gpu_voxel_map_icp.py: 1e-4 rad and 1e-4 m; the sums are not in the restatement's order).  Later runs are compared
# with the GPU's own pose over zeros bit for bit.
POSE_BOUND = 1e-4
POSES = {"map_align": ("pose",), "icp_host": ("pose",), "ms_render": ("pose",),
         "icp_batch": tuple(f"pose{i}" for i in range(8))}


def pose_errors(got, want):
    """(angle, translation) between two 28-byte poses."""
    import oracle_lib as O
    from align3d_amd._abi import PoseC

    return O.transform_metrics(PoseC.from_buffer_copy(bytes(got)), PoseC.from_buffer_copy(bytes(want)))


# ---- BilateralFilter, host and device forms ---------------------------------------------------------------------------------
DEPTH_BATCH = {"S": 3, "L": 5}  # images of one size per call of the device form


def depth_image(seed, w, h):
    """[h, w] u16: a tilted surface with a step edge, noise, and about a tenth of the pixels invalid (0)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = 900.0 + 6.0 * x + 3.0 * y + np.where(x > w // 2, 700.0, 0.0) + rng.random((h, w)) * 25.0
    d[rng.random((h, w)) < 0.1] = 0.0
    return d.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def depth_images(which):
    """(the images of IMAGES[which], one per size; a batch of DEPTH_BATCH[which] images of the first size)."""
    base = 500 if which == "S" else 600
    w0, h0 = IMAGES[which][0]
    return ([depth_image(base + i, w, h) for i, (w, h) in enumerate(IMAGES[which])],
            np.stack([depth_image(base + 50 + i, w0, h0) for i in range(DEPTH_BATCH[which])]))


def run_bilateral_host(ctx, which):
    from align3d_amd import BilateralFilter

    f = BilateralFilter.default()
    return {f"host{i}": f.filter(ctx, img) for i, img in enumerate(depth_images(which)[0])}


def run_bilateral_device(ctx, which):
    from align3d_amd import BilateralFilter

    batch = depth_images(which)[1]
    d_in, d_out = ctx.to_device(batch), ctx.malloc(batch.nbytes)
    BilateralFilter.default().filter_device(ctx, d_in, len(batch), batch.shape[2], batch.shape[1], d_out)
    out = {"device": ctx.to_host(d_out, np.empty_like(batch))}
    ctx.free(d_in), ctx.free(d_out)
    return out


def _filtered(img):
    import oracle_lib as O

    status, want, _ = O.bilateral(img)
    assert status == 0
    return want


def ref_bilateral_host(which):
    return {f"host{i}": _filtered(img) for i, img in enumerate(depth_images(which)[0])}


def ref_bilateral_device(which):
    return {"device": np.stack([_filtered(img) for img in depth_images(which)[1]])}


# ---- pyramids with intensity over four levels, compute_intensity_batch --------------------------------------------------------
PYRAMID_LEVELS = 4
# (width, height, images per call): sides that are multiples of 4 take the fused level-0 kernel, the others the pick kernels
PYRAMID_BATCHES = {"S": ((64, 48, 2), (37, 101, 1)), "L": ((160, 120, 3),)}
INTENSITY_SIZES = {"S": ((37, 101), (64, 48), (5, 3)), "L": ((160, 120), (80, 60), (37, 101), (12, 8), (1, 1))}


def colour_image(seed, w, h):
    """A host RangeImage of finite points and normals, a mask with zeros, and colours."""
    from align3d_amd import CameraIntrinsics, RangeImage

    rng = np.random.default_rng(seed)
    pts, nrm = ((rng.standard_normal((h, w, 3)) * 10).astype(F) for _ in range(2))
    mask = rng.choice(np.asarray([0, 1, 1, 1, 2, 255], np.uint8), size=(h, w))
    return RangeImage(pts, mask, CameraIntrinsics(525.0, 523.5, w / 2 - 0.5, h / 2 + 0.25, w, h), normals=nrm,
                      colors=rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def pyramid_hosts(which):
    base = 700 if which == "S" else 800
    return [[colour_image(base + 10 * b + i, w, h) for i in range(n)] for b, (w, h, n) in enumerate(PYRAMID_BATCHES[which])]


@functools.lru_cache(maxsize=None)
def intensity_hosts(which):
    base = 900 if which == "S" else 950
    return [colour_image(base + i, w, h) for i, (w, h) in enumerate(INTENSITY_SIZES[which])]


def _upload(ctx, host):
    from align3d_amd import DeviceRangeImage

    return DeviceRangeImage(ctx, host).set_colors(host.colors)


def _level_arrays(out, tag, points, mask, normals, colors, intensities, imap):
    out[f"{tag}.points"], out[f"{tag}.mask"], out[f"{tag}.normals"] = _bits(points), np.asarray(mask), _bits(normals)
    out[f"{tag}.colors"] = np.ascontiguousarray(colors)  # the plane's own 3 * w * h bytes
    out[f"{tag}.intensities"], out[f"{tag}.imap"] = np.asarray(intensities).reshape(-1), _bits(imap)


def run_pyramid(ctx, which):
    from align3d_amd import pyramids

    out = {}
    for b, hosts in enumerate(pyramid_hosts(which)):
        built = pyramids([_upload(ctx, h) for h in hosts], PYRAMID_LEVELS, 1.0, True)
        for i, levels in enumerate(built):
            for l, dev in enumerate(levels):
                g = dev.download()
                _level_arrays(out, f"batch{b}.image{i}.level{l}", g.points, g.mask, g.normals, g.colors, g.intensities,
                              g.intensity_map)
                dev.free()
    return out


def oracle_levels(host, levels, sigma):
    """RangeImage::pyramid(levels, sigma) with intensities and maps, put together from the oracle's own bricks
    (orc_resize_range_points / _normals, orc_rgb_pyr_down, orc_rgb_to_luma_u8, intensity_map): a list of dicts."""
    import oracle_lib as O
    from align3d_amd._abi import ptr

    lib = O.load()
    pyr = [dict(points=host.points, mask=host.mask, normals=host.normals, colors=host.colors)]
    for _ in range(levels - 1):
        p = pyr[-1]
        sh, sw = p["mask"].shape
        dh, dw = sh // 2, sw // 2
        pts, mask, nrm = np.empty((dh, dw, 3), F), np.empty((dh, dw), np.uint8), np.empty((dh, dw, 3), F)
        col = np.empty((dh, dw, 3), np.uint8)
        lib.orc_resize_range_points(ptr(p["points"]), ptr(p["mask"]), sw, sh, dw, dh, ptr(pts), ptr(mask))
        lib.orc_resize_range_normals(ptr(p["normals"]), ptr(p["mask"]), sw, sh, dw, dh, ptr(nrm))
        lib.orc_rgb_pyr_down(ptr(p["colors"]), sw, sh, sigma, ptr(col))
        pyr.append(dict(points=pts, mask=mask, normals=nrm, colors=col))
    for p in pyr:
        h, w = p["mask"].shape
        luma = np.empty((h, w), np.uint8)
        lib.orc_rgb_to_luma_u8(ptr(np.ascontiguousarray(p["colors"])), w * h, ptr(luma))
        p["intensities"], p["imap"] = luma.reshape(-1), O.intensity_map(luma)
    return pyr


def ref_pyramid(which):
    out = {}
    for b, hosts in enumerate(pyramid_hosts(which)):
        for i, host in enumerate(hosts):
            for l, r in enumerate(oracle_levels(host, PYRAMID_LEVELS, 1.0)):
                _level_arrays(out, f"batch{b}.image{i}.level{l}", r["points"], r["mask"], r["normals"], r["colors"],
                              r["intensities"], r["imap"])
    return out


def run_intensity(ctx, which):
    from align3d_amd import compute_intensity_batch

    devs = [_upload(ctx, h) for h in intensity_hosts(which)]
    compute_intensity_batch(devs)
    out = {}
    for i, dev in enumerate(devs):
        g = dev.download(normals=False, colors=False)
        out[f"image{i}.intensities"], out[f"image{i}.imap"] = np.asarray(g.intensities).reshape(-1), _bits(g.intensity_map)
        dev.free()
    return out


def ref_intensity(which):
    out = {}
    for i, host in enumerate(intensity_hosts(which)):
        r = oracle_levels(host, 1, 1.0)[0]
        out[f"image{i}.intensities"], out[f"image{i}.imap"] = np.asarray(r["intensities"]).reshape(-1), _bits(r["imap"])
    return out


# ---- R3dTree.new + nearest + download, Icp.align from a host source, IcpBatch.align ------------------------------------------
TREE_ROWS = {"S": 5003, "L": 40009}        # ranges above 2048 rows: the selection build's wide levels run
ICP_BATCH = {"S": (5003, 2600, 17), "L": (40009, 9001, 5003, 2049, 33)}  # target rows per pair of an IcpBatch
ICP_ITERATIONS = 5


def surface(seed, n):
    """(points, unit normals) of n rows scattered over a smooth, bumpy surface in [-1, 1]^2: every neighbourhood
    constrains all six degrees of freedom, so an alignment on it does not hang on rounding."""
    rng = np.random.default_rng(seed)
    x, y = rng.random(n) * 2 - 1, rng.random(n) * 2 - 1
    z = 0.3 * np.sin(2 * x) + 0.2 * np.cos(3 * y) + 0.1 * np.sin(5 * x * y)
    dzdx = 0.6 * np.cos(2 * x) + 0.5 * y * np.cos(5 * x * y)
    dzdy = -0.6 * np.sin(3 * y) + 0.5 * x * np.cos(5 * x * y)
    nrm = np.stack([-dzdx, -dzdy, np.ones(n)], -1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = np.stack([x, y, z], -1).astype(F)
    if n >= 64:  # equal rows and equal coordinates: ties at every level of the tree
        pts[5:9] = pts[1:5]
        pts[20:40, 0] = pts[20, 0]
        nrm[5:9] = nrm[1:5]
    return pts, nrm.astype(F)


def moved_source(points, normals, step):
    """Every step-th row, a little off its place."""
    import oracle_lib as O
    from voxel_map_icp_restatement import transform_normals

    off = O.exp_se3([0.004, -0.003, 0.002, 0.01, -0.008, 0.006])
    return O.transform_points(off, points[::step]), transform_normals(off, normals[::step])


def tree_queries(which):
    rng = np.random.default_rng(11 if which == "S" else 12)
    q = (rng.random((TREE_ROWS[which] // 2, 3)) * 2.2 - 1.1).astype(F)
    q[:64] = surface(40 if which == "S" else 41, TREE_ROWS[which])[0][:64]  # queries that are points of the tree: distance 0
    return q


def tree_restatement(points):
    """R3dTree::new (src/kdtree.rs:28-58) as the library lays it out (include/align3d_hip.h): per node a stable sort by the
    coordinate of axis depth % 3 (-0.0 == +0.0), the split value the coordinate at len / 2, leaves of at most 16 rows;
    split values in heap order (0 where the node is a leaf), leaf slot r of the leaf at `path`, `depth` at
    (path << (D - depth)) * 16 + r holding (x, y, z, row), the others (+inf, +inf, +inf, 0)."""
    pts = np.ascontiguousarray(points, F)
    n = len(pts)

    def depth_of(length, depth):
        return depth if length <= 16 else max(depth_of(length // 2, depth + 1), depth_of(length - length // 2, depth + 1))

    D = depth_of(n, 0)
    split = np.zeros((1 << D) - 1, F)
    leaves = np.zeros(((1 << D) * 16, 4), np.uint32)
    leaves[:, :3] = np.float32(np.inf).view(np.uint32)
    stack = [(np.arange(n), 0, 0, 0)]
    while stack:
        idx, node, path, depth = stack.pop()
        if len(idx) <= 16:
            base = (path << (D - depth)) * 16
            leaves[base:base + len(idx), :3] = pts[idx].view(np.uint32)
            leaves[base:base + len(idx), 3] = idx
            continue
        k = depth % 3
        idx = idx[np.argsort(pts[idx, k] + F(0.0), kind="stable")]
        mid = len(idx) // 2
        split[node] = pts[idx[mid], k]
        stack.append((idx[mid:], 2 * node + 2, 2 * path + 1, depth + 1))
        stack.append((idx[:mid], 2 * node + 1, 2 * path, depth + 1))
    return split.view(np.uint32), leaves


def run_tree(ctx, which):
    from align3d_amd import R3dTree

    tree = R3dTree.new(ctx, surface(40 if which == "S" else 41, TREE_ROWS[which])[0])
    idx, d2 = tree.nearest(tree_queries(which))
    split, leaves = tree.download()
    tree.free()
    return {"nearest.index": idx, "nearest.d2": _bits(d2), "split": np.ascontiguousarray(split),
            "leaves": np.ascontiguousarray(leaves)}


def ref_tree(which):
    import oracle_lib as O

    pts = surface(40 if which == "S" else 41, TREE_ROWS[which])[0]
    idx, d2 = O.KdTree(pts).nearest(tree_queries(which))
    split, leaves = tree_restatement(pts)
    return {"nearest.index": idx, "nearest.d2": _bits(d2), "split": split, "leaves": leaves}


def _icp_params():
    from align3d_amd import IcpParams

    return IcpParams(max_iterations=ICP_ITERATIONS)


def _pose_bytes(pose_c):
    return np.frombuffer(bytes(pose_c), np.uint8).copy()


def _oracle_align(target, source):
    import ctypes as C

    import oracle_lib as O
    from align3d_amd._abi import PoseC

    tree, out, prm = O.KdTree(target[0]), PoseC(), _icp_params().to_c()
    tv, sv = O.pcl_view(target[0], target[1]), O.pcl_view(source[0], source[1])
    status = O.load().orc_pcl_icp_align(C.byref(prm), tree.h, C.byref(tv), C.byref(sv), C.byref(out), None)
    return status, out


def run_icp_host(ctx, which):
    from align3d_amd import Icp, PointCloud

    target = surface(50 if which == "S" else 51, TREE_ROWS[which])
    icp = Icp.new(ctx, _icp_params(), PointCloud(*target))
    pose = icp.align(PointCloud(*moved_source(*target, 3)))  # host memory: staged in the kd-tree scratch region
    icp.free()
    return {"pose": _pose_bytes(pose.to_c())}


def ref_icp_host(which):
    target = surface(50 if which == "S" else 51, TREE_ROWS[which])
    status, pose = _oracle_align(target, moved_source(*target, 3))
    assert status == 0
    return {"pose": _pose_bytes(pose)}


def icp_batch_pairs(which):
    pairs = []
    for i, n in enumerate(ICP_BATCH[which]):
        target = surface((60 if which == "S" else 70) + i, n)
        pairs.append((target, moved_source(*target, 2 if n < 100 else 5)))
    return pairs


def run_icp_batch(ctx, which):
    from align3d_amd import DevicePointCloud, IcpBatch, PointCloud

    pairs = icp_batch_pairs(which)
    targets = [DevicePointCloud(ctx, PointCloud(*t)) for t, _ in pairs]
    sources = [DevicePointCloud(ctx, PointCloud(*s)) for _, s in pairs]
    batch = IcpBatch.new(ctx, _icp_params(), targets)
    poses, status = batch.align(sources)
    batch.free()
    _free(targets, sources)
    out = {"status": np.asarray(status, np.int32)}
    for i, pose in enumerate(poses):
        out[f"pose{i}"] = _pose_bytes(pose.to_c())
    return out


def ref_icp_batch(which):
    out, status = {}, []
    for i, (target, source) in enumerate(icp_batch_pairs(which)):
        st, pose = _oracle_align(target, source)
        status.append(st)
        out[f"pose{i}"] = _pose_bytes(pose)
    out["status"] = np.asarray(status, np.int32)
    return out


# ---- RangeImageBuilder.build at 1 and 3 levels, with and without the bilateral filter ---------------------------------------------
BUILDER_VARIANTS = ((1, False), (3, True), (3, False), (1, True))  # (pyramid levels, bilateral filter)
BUILDER_FRAMES = {"S": 1, "L": 3}                                    # frames per build call
DEPTH_SCALE = 5000.0


@functools.lru_cache(maxsize=None)
def builder_frames(which):
    """[(width, height, [(depth u16, rgb u8)] of BUILDER_FRAMES[which] frames)] per size of IMAGES[which]."""
    base = 1000 if which == "S" else 1100
    out = []
    for k, (w, h) in enumerate(IMAGES[which]):
        frames = []
        for i in range(BUILDER_FRAMES[which]):
            rng = np.random.default_rng(base + 10 * k + i)
            frames.append((depth_image(base + 10 * k + i, w, h), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
        out.append((w, h, frames))
    return out


def _builder_camera(w, h):
    return 525.0 * w / 640.0, 523.5 * w / 640.0, w / 2 - 0.5, h / 2 + 0.25


def run_builder(ctx, which):
    from align3d_amd import BilateralFilter, CameraIntrinsics, RangeImageBuilder

    out = {}
    for k, (w, h, frames) in enumerate(builder_frames(which)):
        for levels, bilateral in BUILDER_VARIANTS:
            builder = RangeImageBuilder(ctx).pyramid_levels(levels)
            if bilateral:
                builder = builder.with_bilateral_filter(BilateralFilter.default())
            built = builder.build_many(CameraIntrinsics(*_builder_camera(w, h), w, h), frames, DEPTH_SCALE)
            for i, pyramid in enumerate(built):
                for l, dev in enumerate(pyramid):
                    g = dev.download()
                    _level_arrays(out, f"size{k}.L{levels}.B{int(bilateral)}.frame{i}.level{l}", g.points, g.mask, g.normals,
                                  g.colors, g.intensities, g.intensity_map)
                    dev.free()
    return out


def ref_builder(which):
    import oracle_lib as O

    out = {}
    for k, (w, h, frames) in enumerate(builder_frames(which)):
        for levels, bilateral in BUILDER_VARIANTS:
            for i, (depth, rgb) in enumerate(frames):
                pyr = O.build_pyramid(depth, rgb, *_builder_camera(w, h), DEPTH_SCALE, levels=levels, use_bilateral=bilateral)
                for l, f in enumerate(pyr):
                    _level_arrays(out, f"size{k}.L{levels}.B{int(bilateral)}.frame{i}.level{l}", f.points, f.mask, f.normals,
                                  f.colors, f.intensities, f.intensity_map)
    return out


# ---- MultiscaleAlign.align on a rendered target ---------------------------------------------------------------------------------
MS_VIEW = {"S": (64, 48, 40.0, 12000), "L": (160, 120, 100.0, 60000)}  # width, height, focal length, rows of the model
MS_LEVELS, MS_ITERATIONS = 3, 3


@functools.lru_cache(maxsize=None)
def ms_clouds(which):
    """(the model in front of the camera, the same model moved a little): points, normals, colours of a textured surface."""
    import oracle_lib as O
    from voxel_map_icp_restatement import transform_normals

    n = MS_VIEW[which][3]
    pts, nrm = surface(80 if which == "S" else 81, n)
    tex = 128 + 100 * np.sin(4 * pts[:, 0]) * np.cos(3 * pts[:, 1])
    col = np.stack([tex, 0.8 * tex + 20, 255 - tex], -1).clip(0, 255).astype(np.uint8)
    pts = (pts + F([0.0, 0.0, 2.0])).astype(F)
    off = O.exp_se3([0.004, -0.003, 0.002, 0.006, -0.005, 0.004])
    return (pts, nrm, col), (O.transform_points(off, pts), transform_normals(off, nrm), col)


def _ms_camera(which):
    from align3d_amd import CameraIntrinsics

    w, h, f, _ = MS_VIEW[which]
    return CameraIntrinsics(f, f, w / 2 - 0.5, h / 2 - 0.5, w, h)


def _ms_params():
    from align3d_amd import MsIcpParams

    return MsIcpParams.default().customize(lambda i, p: setattr(p, "max_iterations", MS_ITERATIONS))


def run_ms_render(ctx, which):
    from align3d_amd import DevicePointCloud, MultiscaleAlign, PointCloud

    cam, pyramids_ = _ms_camera(which), []
    for pts, nrm, col in ms_clouds(which):
        cloud = DevicePointCloud(ctx, PointCloud(pts, nrm, col))
        pyramids_.append(cloud.render(cam, None, 0.0).pyramid(MS_LEVELS, 1.0, True))
        cloud.free()
    aligner = MultiscaleAlign.new(ctx, _ms_params(), pyramids_[0])
    pose = aligner.align(pyramids_[1])
    aligner.free()
    for levels in pyramids_:
        _free(levels)
    return {"pose": _pose_bytes(pose.to_c())}


def ref_ms_render(which):
    import types

    import oracle_lib as O
    import render_restatement as RR

    cam, frames = _ms_camera(which), []
    for pts, nrm, col in ms_clouds(which):
        image = RR.render(pts, nrm, col, None, F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy), cam.width, cam.height, 0.0)
        host = types.SimpleNamespace(points=image["points"], mask=image["mask"], normals=image["normals"], colors=image["colors"])
        frames.append([O.Frame(lv["points"], lv["mask"], cam.fx * 0.5 ** l, cam.fy * 0.5 ** l, cam.cx * 0.5 ** l, cam.cy * 0.5 ** l,
                               lv["normals"], lv["intensities"], lv["imap"]) for l, lv in enumerate(oracle_levels(host, MS_LEVELS, 1.0))])
    status, pose = O.multiscale_align(_ms_params().to_c_array(), MS_LEVELS, frames[0], frames[1], threads=4)
    assert status == 0
    return {"pose": _pose_bytes(pose)}


CASES = {
    "ms_render": Case((4, 5, 6), run_ms_render, ref_ms_render, "render_restatement, oracle_lib"),
    "builder": Case((0, 1, 6), run_builder, ref_builder, "oracle_lib"),
    "tree": Case((2, 7), run_tree, ref_tree, "oracle_lib, tree_restatement"),
    "icp_host": Case((2, 7), run_icp_host, ref_icp_host, "oracle_lib"),
    "icp_batch": Case((2, 7), run_icp_batch, ref_icp_batch, "oracle_lib"),
    "pyramid": Case((4, 6), run_pyramid, ref_pyramid, "oracle_lib"),
    "intensity": Case((4, 6), run_intensity, ref_intensity, "oracle_lib"),
    "bilateral_host": Case((0, 1), run_bilateral_host, ref_bilateral_host, "oracle_lib"),
    "bilateral_device": Case((1,), run_bilateral_device, ref_bilateral_device, "oracle_lib"),
    "map_align": Case((3, 7), run_map_align, ref_map_align, "voxel_map_icp_restatement"),
    "from_images": Case((3, 6), run_from_images, ref_from_images, "numpy (mask != 0, row-major)"),
    "transform_merge": Case((3,), run_transform, ref_transform, "oracle_lib"),
    "voxel_nearest": Case((3,), run_voxel_nearest, ref_voxel_nearest, "voxel_restatement"),
    "voxel_mean": Case((3,), run_voxel_mean, ref_voxel_mean, "voxel_mean_restatement"),
    "normals": Case((3,), run_normals, ref_normals, "normals_restatement"),
    "outliers": Case((3,), run_outliers, ref_outliers, "outlier_restatement"),
    "cluster": Case((3,), run_cluster, ref_cluster, "cluster_restatement"),
    "plane": Case((3,), run_plane, ref_plane, "plane_restatement"),
    "map_nearest": Case((3, 7), run_map_nearest, ref_map_nearest, "voxel_map_icp_restatement"),
    "map_mean": Case((3, 7), run_map_mean, ref_map_mean, "voxel_mean_restatement"),
    "render": Case((5, 6), run_render, ref_render, "render_restatement"),
    "map_render": Case((3, 5, 6, 7), run_map_render, ref_map_render, "render_restatement"),
}
POOLED = {name: tuple(r for r in case.regions if r >= 6) for name, case in CASES.items() if max(case.regions) >= 6}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The independent reference of the case's S input, computed once for every test that needs it."""
    return CASES[name].reference("S")


def sharing(name):
    """The other cases that use one of this case's scratch regions (pooled memory, 6 and 7, is not a layout)."""
    mine = {r for r in CASES[name].regions if r < 6}
    return [other for other, case in CASES.items() if other != name and mine & {r for r in case.regions if r < 6}]


# A NaN that the arithmetic produces (a pose applied to a NaN or infinite row) has another sign and payload on x86 than on
# the GPU (test_gpu_cloud_transform.py); the reference of these cases fixes WHERE the NaNs are and every other bit.  What
# the GPU itself gave over zeros, (a), is compared with later runs in full, NaN bits included.
COMPUTED_NANS = ("transform_merge",)


def mismatches(got, want, computed_nans=False, poses=()):
    """The names at which two results differ (shape, type or a bit).  computed_nans: in f32 planes (uint32 views named
    *.points / *.normals) a NaN matches any NaN.  poses: names compared as poses within POSE_BOUND."""
    bad = sorted(set(got) ^ set(want))
    for name in sorted(set(got) & set(want)):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if name in poses:
            ang, tr = pose_errors(a, b)
            if not (ang <= POSE_BOUND and tr <= POSE_BOUND):
                bad.append(f"{name} (d_angle {ang:.3g}, d_trans {tr:.3g})")
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(name)
            continue
        if computed_nans and a.dtype == np.uint32 and name.endswith((".points", ".normals")):
            nan_a, nan_b = (a & 0x7FFFFFFF) > 0x7F800000, (b & 0x7FFFFFFF) > 0x7F800000
            if not np.array_equal(nan_a, nan_b) or not np.array_equal(a[~nan_a], b[~nan_b]):
                bad.append(name)
        elif not np.array_equal(a, b):
            bad.append(name)
    return bad
