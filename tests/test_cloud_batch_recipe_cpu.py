"""The batch recipe of test_gpu_cloud_batch_many_jobs.py and the conditions it has to meet, checked without a GPU.

The job-table kernels (csrc/cloud_batch.hpp: point clouds from images, transform, merge, voxel downsample, voxel-map
insert) take one job per NON-EMPTY cloud, in cloud order; a job's tiles follow the previous job's.  `recipe` and
`image_recipe` are the seeded inputs of the GPU tests; `plan` restates the host's tile plan (plan_tiles and the loop
around it) in Python.  The tests below are conditions on those inputs: they say that a batch of 1000 reaches the paths
the GPU tests are there for (the second trip of the loops over jobs, a deep find_job search, job index != cloud index,
tiles exactly full and one point either side, per-job counts that an index mix-up cannot reproduce)."""
import numpy as np

import voxel_restatement as V

SEED = 20250
VOXEL = 0.05
LENGTHS = (1, 0, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
BIG_AT, BIG_LEN = (0, 70), 70001
# (h, w) of the image cycle: 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097 and 6145 pixels
IMAGE_SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (23, 89), (32, 64), (3, 683), (63, 65), (64, 64), (17, 241), (5, 1229))
BIG_IMAGE = (480, 640)
MASK_VALUES = (0, 1, 2, 255)
BATCHES = (65, 129, 1000)
# points per tile: transform and merge (XF_THREADS * XF_PPT), voxel downsample and voxel-map insert (VX_CHUNK, VM_CHUNK),
# pixels per tile of point clouds from images (CLOUD_CHUNK); and the most tiles a job of the last three may have
TILE_TRANSFORM, TILE_VOXEL, TILE_IMAGE, MAX_TILES = 512, 1024, 2048, 4096
EDGE_CLOUDS = (63, 64, 65, 127, 128, 129)  # and N - 1


def is_raw(i):
    """Whether cloud i holds raw random bits: two clouds of every 64 from index 64 on."""
    return i >= 64 and i % 64 < 2 and i not in BIG_AT


def cloud_length(i):
    return BIG_LEN if i in BIG_AT else LENGTHS[i % len(LENGTHS)]


def _raw_bits(rng, n):
    """[n, 3] raw random bits (the _raw_bits recipe of test_gpu_voxel_downsample.py): NaNs with payloads, infinities,
    -0.0, denormals and magnitudes far beyond the 2^20 cell range all occur."""
    a = rng.integers(0, 2**32, size=(n, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    special = np.asarray([np.nan, -0.0, np.inf, -np.inf, 0.0, 1e-45], np.float32)
    a.reshape(-1)[:min(6, a.size)] = special[:min(6, a.size)]
    return a


def _pose(rng):
    """(t [3], q [4] i, j, k, w) f32: a rotation of up to ~1 rad, a translation of up to 0.5 m per axis."""
    q = np.concatenate([rng.uniform(-0.5, 0.5, size=3), [1.0]]).astype(np.float32)
    q = q / np.float32(np.sqrt(np.float32(np.sum(q * q))))
    return rng.uniform(-0.5, 0.5, size=3).astype(np.float32), q.astype(np.float32)


def recipe(n_jobs, bare_third=True):
    """[(points [len, 3] f32, normals [len, 3] f32 or None, (t, q))] for clouds 0 .. n_jobs - 1.  Cloud i does not
    depend on n_jobs.  Its points fill a box of side 0.05 * cbrt(len / 4) somewhere inside [-2, 2 + side)^3, so a 0.05
    voxel holds about four of them; clouds with is_raw(i) hold raw random bits instead (their normals stay finite: the
    payload of a NaN that a transform COMPUTES is not defined, and a normal plays no part in any drop rule).
    bare_third: every third non-empty cloud has no normals (the values of the other clouds do not change)."""
    out, ordinal = [], 0
    for i in range(n_jobs):
        rng = np.random.default_rng([SEED, i])
        n = cloud_length(i)
        side = VOXEL * max(1.0, n / 4.0) ** (1.0 / 3.0)
        corner = rng.uniform(-2.0, 2.0, size=3)
        points = (corner + rng.uniform(0.0, side, size=(n, 3))).astype(np.float32)
        normals = rng.normal(size=(n, 3)).astype(np.float32)
        if is_raw(i):
            points = _raw_bits(rng, n)
        pose = _pose(rng)
        if n:
            ordinal += 1
        out.append((points, None if bare_third and n and ordinal % 3 == 0 else normals, pose))
    return out


def image_shape(i):
    return BIG_IMAGE if i in BIG_AT else IMAGE_SHAPES[i % len(IMAGE_SHAPES)]


def keeps_nothing(i):
    """Images whose mask is all zero (none of them is one of the images the GPU tests single out)."""
    return i % 17 == 3


def image_recipe(n_jobs):
    """[(points [h, w, 3] f32 raw random bits, mask [h, w] u8 drawn from MASK_VALUES, normals [h, w, 3] or None)] for
    images 0 .. n_jobs - 1; every third image has no normals, the images with keeps_nothing(i) an all-zero mask."""
    out = []
    for i in range(n_jobs):
        rng = np.random.default_rng([SEED + 1, i])
        h, w = image_shape(i)
        points = _raw_bits(rng, h * w).reshape(h, w, 3)
        normals = _raw_bits(rng, h * w).reshape(h, w, 3)
        mask = rng.choice(np.asarray(MASK_VALUES, np.uint8), size=(h, w))
        if keeps_nothing(i):
            mask[:] = 0
        out.append((points, mask, None if i % 3 == 2 else normals))
    return out


def plan(lengths, chunk, max_tiles=None):
    """The tile plan of a batch: [(cloud index, first_tile, tiles, chunks_per_tile)] per job, one job per non-empty
    element.  max_tiles=None: the transform's plan, a tile per chunk whatever the length."""
    jobs, tiles = [], 0
    for i, n in enumerate(lengths):
        if n == 0:
            continue
        chunks = (n + chunk - 1) // chunk
        per_tile = 1 if max_tiles is None else (chunks + max_tiles - 1) // max_tiles
        count = (chunks + per_tile - 1) // per_tile
        jobs.append((i, tiles, count, per_tile))
        tiles += count
    return jobs


def batch_lengths(n_jobs):
    return [cloud_length(i) for i in range(n_jobs)]


def image_pixels(n_jobs):
    return [image_shape(i)[0] * image_shape(i)[1] for i in range(n_jobs)]


def plans(n_jobs):
    """{operation: (lengths, tile size, plan)} of a batch of n_jobs."""
    clouds, pixels = batch_lengths(n_jobs), image_pixels(n_jobs)
    return {
        "transform / merge": (clouds, TILE_TRANSFORM, plan(clouds, TILE_TRANSFORM)),
        "voxel downsample / voxel-map insert": (clouds, TILE_VOXEL, plan(clouds, TILE_VOXEL, MAX_TILES)),
        "point clouds from images": (pixels, TILE_IMAGE, plan(pixels, TILE_IMAGE, MAX_TILES)),
    }


def test_lengths_follow_the_cycle_and_the_images_their_pixel_counts():
    clouds = recipe(200)
    assert [len(p) for p, _, _ in clouds] == batch_lengths(200)
    assert all(len(clouds[i][0]) == BIG_LEN for i in BIG_AT)
    assert [p.shape[0] * p.shape[1] for p, _, _ in image_recipe(33)[1:12]] == [63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097,
                                                                              6145, 1]
    assert image_pixels(71)[0] == image_pixels(71)[70] == 480 * 640
    # a cloud is the same in every batch size, with and without the bare third
    for (p, n, pose), (p2, n2, pose2) in zip(recipe(66), recipe(66, bare_third=False)[:66]):
        assert np.array_equal(p.view(np.uint32), p2.view(np.uint32)) and (n is None or np.array_equal(n, n2))
        assert np.array_equal(pose[0], pose2[0]) and np.array_equal(pose[1], pose2[1])
    bare = [n is None for p, n, _ in clouds if len(p)]
    assert bare == [k % 3 == 2 for k in range(len(bare))]
    images = image_recipe(130)
    assert sum(m.any() for _, m, _ in images) < len(images) and all(set(np.unique(m)) <= set(MASK_VALUES) for _, m, _ in images)
    assert [n is None for _, _, n in images] == [i % 3 == 2 for i in range(130)]
    for i in (0, 63, 64, 65, 70, 128, 129):
        assert not keeps_nothing(i) and images[i][1].any()
    assert not keeps_nothing(999)


def test_tile_plans_of_a_thousand_jobs_reach_every_edge():
    n = 1000
    for name, (lengths, tile, jobs) in plans(n).items():
        by_cloud = {i: (k, first, count, per_tile) for k, (i, first, count, per_tile) in enumerate(jobs)}
        assert all(per_tile == 1 for _, _, _, per_tile in jobs), name
        assert len(jobs) > 64 * 2, name  # the k += 64 loops over jobs make a second trip, and a third
        # exactly one full tile, one point more, one point less
        for want in (tile, tile + 1, tile - 1):
            assert any(lengths[i] == want for i, _, _, _ in jobs), (name, want)
        assert any(count == 1 and lengths[i] == tile for i, _, count, _ in jobs), name
        assert any(count == 2 and lengths[i] == tile + 1 for i, _, count, _ in jobs), name
        assert max(first for _, first, _, _ in jobs) > 1024, name
        k70, first70, count70, _ = by_cloud[70]
        assert count70 > 64 and first70 > 64, name  # the sum over a job's earlier tiles makes a second trip too
        print(f"[{name}] N = {n}: {len(jobs)} jobs, {jobs[-1][1] + jobs[-1][2]} tiles of {tile}, "
              f"largest first_tile {max(first for _, first, _, _ in jobs)}, job 70: {count70} tiles from {first70}")


def test_job_index_differs_from_cloud_index_behind_the_first_empty_cloud():
    for n in BATCHES:
        lengths = batch_lengths(n)
        first_empty = lengths.index(0)
        assert first_empty == 1
        for tile, limit in ((TILE_TRANSFORM, None), (TILE_VOXEL, MAX_TILES)):
            jobs = plan(lengths, tile, limit)
            assert len(jobs) == sum(1 for x in lengths if x) < n
            for k, (i, _, _, _) in enumerate(jobs):
                assert (k == i) == (i < first_empty) and k <= i
        # the clouds the GPU tests single out are jobs, not empty clouds
        assert all(lengths[i] > 0 for i in (*EDGE_CLOUDS, 0, 70, n - 1) if i < n)
    # an image cannot be empty: there the two indices agree
    assert [i for i, _, _, _ in plan(image_pixels(1000), TILE_IMAGE, MAX_TILES)] == list(range(1000))


def test_edge_clouds_have_distinct_counts_and_late_jobs_drop_and_keep():
    n = 1000
    clouds = recipe(n)
    triples = {}
    for i in (*EDGE_CLOUDS, n - 1):
        index, dropped = V.voxel_downsample(clouds[i][0], VOXEL)
        triples[i] = (len(clouds[i][0]), len(index), dropped)
    print(f"(length, kept, dropped) at v = {VOXEL}: {triples}")
    assert len(set(triples.values())) == len(triples)
    assert all(kept >= 2 for _, kept, _ in triples.values())  # (a capacity one short still leaves room for a point)
    both = []
    for i in range(64, n):
        if is_raw(i) and len(clouds[i][0]):
            index, dropped = V.voxel_downsample(clouds[i][0], VOXEL)
            if dropped and len(index):
                both.append((i, len(index), dropped))
    assert len(both) >= 3
    assert len({(kept, dropped) for _, kept, dropped in both}) >= 3  # and the counts differ from job to job
    # the tame clouds drop nothing and share cells: about four points per occupied voxel
    for i in (0, 5, 13, 70):
        p = clouds[i][0]
        index, dropped = V.voxel_downsample(p, VOXEL)
        assert dropped == 0 and np.isfinite(p).all() and np.abs(p).max() < 4.0
        assert len(p) / 8 < len(index) < len(p) / 1.5, (i, len(p), len(index))
