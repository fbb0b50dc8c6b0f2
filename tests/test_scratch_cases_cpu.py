"""The inputs of the scratch-independence cases (scratch_cases.py) do their job: every S reference is non-trivial, L lies
over S's cells, and every part of L's layout is strictly larger than S's.  No GPU."""
import numpy as np
import pytest

import scratch_cases as SC
import voxel_restatement as V


def test_lengths_are_the_sizes_the_table_promises():
    assert sum(SC.LENGTHS["S"]) == 2049 and sum(SC.LENGTHS["L"]) == 20011
    assert 1 in SC.LENGTHS["S"] and 1 in SC.LENGTHS["L"] and len(SC.LENGTHS["S"]) != len(SC.LENGTHS["L"])
    assert len(set(SC.LENGTHS["S"])) == len(SC.LENGTHS["S"])  # unequal lengths
    assert max(SC.LENGTHS["S"]) > SC.CHUNK  # a cloud of two chunks
    assert set(SC.IMAGES["S"]) == {(37, 101), (64, 48)} and SC.IMAGES["L"] == ((160, 120),)


def test_large_layout_is_strictly_larger_in_every_part():
    small, large = SC.layout("S"), SC.layout("L")
    assert set(small) == set(large)
    for part in small:
        assert large[part] > small[part], part


def test_small_and_large_share_cells_and_coordinate_range():
    (sp, _, _), (lp, _, _) = SC.merged("S"), SC.merged("L")
    for pitch, origin in ((SC.VOXEL, SC.ORIGIN), (SC.RADIUS, None), (SC.CLUSTER_RADIUS, None)):
        sk, s_keys, _ = V.voxel_keys(sp, pitch, origin)
        lk, l_keys, _ = V.voxel_keys(lp, pitch, origin)
        shared = np.intersect1d(s_keys[sk], l_keys[lk])
        # most cells of S are cells of L at every pitch (the scattered rows of S have cells of their own at the finer ones)
        assert len(shared) > 0.5 * len(np.unique(s_keys[sk])), pitch
    ok = np.isfinite(sp).all(axis=1)
    assert np.abs(sp[ok]).max() <= 1.0 and np.abs(lp[np.isfinite(lp).all(axis=1)]).max() <= 1.0


def test_every_case_names_a_reference_and_shares_a_region():
    for name, case in SC.CASES.items():
        assert case.reference_name and all(0 <= r < 8 for r in case.regions), name
        assert any(r < 6 for r in case.regions), name
        assert SC.sharing(name), name  # no case is alone in its region: the ordered pairs cover it


def test_voxel_references_have_cells_with_several_points_and_dropped_rows():
    for name, counted in (("voxel_nearest", False), ("voxel_mean", True)):
        ref = SC.reference(name)
        tag = "mean" if counted else "thin"
        kept = len(ref[f"{tag}0.index"])
        assert 1 < kept < SC.LENGTHS["S"][0] - 2, name  # cells hold several points; two rows are dropped
        assert len(ref[f"{tag}2.index"]) == 1, name      # the cloud of one row
        if counted:
            assert (ref["mean0.counts"] > 1).any() and int(ref["mean0.counts"].sum()) == SC.LENGTHS["S"][0] - 2


def test_normals_and_outlier_references_are_not_trivial():
    ref = SC.reference("normals")
    assert 0 < ref["valid"][0] < SC.LENGTHS["S"][0] and ref["dropped"][0] == 2 and ref["valid"][2] == 0
    assert len(np.unique(ref["counts0"])) > 5
    ref = SC.reference("outliers")
    for what in ("radius", "statistical"):
        assert 0 < len(ref[f"{what}0.index"]) < SC.LENGTHS["S"][0], what
    assert (ref["qsum0"] == 0xFFFFFFFF).any() and (ref["qsum0"] != 0xFFFFFFFF).any() and ref["stats"][0][0] > 0


def test_cluster_reference_has_several_clusters_noise_and_a_filtered_part():
    ref = SC.reference("cluster")
    assert len(ref["sizes0"]) > 1 and (ref["labels0"] == 0xFFFFFFFF).any()
    assert 0 < len(ref["big0.index"]) < SC.LENGTHS["S"][0]
    assert (ref["sizes0"] < SC.CLUSTER_MIN_SIZE).any() and (ref["sizes0"] >= SC.CLUSTER_MIN_SIZE).any()


def test_plane_reference_has_inliers_and_outliers():
    ref = SC.reference("plane")
    for i in (0, 1):
        assert 0 < ref["inliers"][i] < SC.LENGTHS["S"][i], i
        assert len(ref[f"on{i}.index"]) == ref["inliers"][i] and len(ref[f"rest{i}.index"]) > 0
    assert ref["planes"][0].any()


def test_map_references_keep_a_part_and_find_most_queries():
    ref = SC.reference("map_nearest")
    assert ref["dropped"].tolist() == [2, 2, 0]
    assert 0 < ref["removed"][0] < len(ref["extract.index"]) and ref["removed"][2] == len(ref["retained.index"]) > 0
    none = ref["nearest.seq"] == 0xFFFFFFFF
    assert none[3] and 0 < none.sum() < len(none) // 2
    ref = SC.reference("map_mean")
    assert (ref["extract.counts"] > 1).any() and not np.array_equal(ref["extract.index"], ref["compacted.index"])


def test_align_reference_moves_the_source_back():
    import oracle_lib as O

    ref = SC.reference("map_align")
    ang, tr = SC.pose_errors(ref["pose"], np.frombuffer(bytes(O.pose()), np.uint8))
    assert ang > 1e-3 and tr > 1e-3  # not the identity it started from: iterations ran and moved the pose


def test_bilateral_reference_smooths_and_keeps_invalid_pixels_apart():
    singles, batch = SC.depth_images("S")
    ref = SC.reference("bilateral_host")
    for i, img in enumerate(singles):
        assert (img == 0).any() and (ref[f"host{i}"] != img).any() and ref[f"host{i}"].shape == img.shape
    assert SC.reference("bilateral_device")["device"].shape == batch.shape and len(batch) != len(SC.depth_images("L")[1])


def test_pyramid_cases_take_both_kernels_and_four_levels():
    (w0, h0, _), (w1, h1, _) = SC.PYRAMID_BATCHES["S"]
    assert w0 % 4 == 0 and h0 % 4 == 0 and (w1 % 4 or h1 % 4) and SC.PYRAMID_LEVELS == 4
    ref = SC.reference("pyramid")
    assert ref["batch0.image0.level3.mask"].shape == (h0 >> 3, w0 >> 3) and ref["batch1.image0.level3.mask"].shape == (h1 >> 3, w1 >> 3)
    for tag in ("batch0.image1.level2", "batch1.image0.level1"):
        assert 0 < (ref[f"{tag}.mask"] != 0).sum() and len(np.unique(ref[f"{tag}.intensities"])) > 4
    assert len(SC.reference("intensity")) == 2 * len(SC.INTENSITY_SIZES["S"])
    # the level table of L (images x levels entries) is longer than either of S's
    assert min(n for _, _, n in SC.PYRAMID_BATCHES["L"]) > max(n for _, _, n in SC.PYRAMID_BATCHES["S"])
    assert len(SC.INTENSITY_SIZES["L"]) > len(SC.INTENSITY_SIZES["S"])


def test_tree_and_icp_references():
    assert SC.TREE_ROWS == {"S": 5003, "L": 40009} and len(SC.ICP_BATCH["S"]) != len(SC.ICP_BATCH["L"])
    ref = SC.reference("tree")
    assert (ref["nearest.d2"][:64] == 0).all() and (ref["nearest.d2"][64:] != 0).any()
    inf = np.float32(np.inf).view(np.uint32)
    used = ref["leaves"][:, 0] != inf
    assert used.sum() == 5003 and (~used).any() and sorted(ref["leaves"][used, 3].tolist()) == list(range(5003))
    import oracle_lib as O

    eye = np.frombuffer(bytes(O.pose()), np.uint8)
    for name, keys in (("icp_host", ["pose"]), ("ms_render", ["pose"]), ("icp_batch", [f"pose{i}" for i in range(len(SC.ICP_BATCH["S"]))])):
        ref = SC.reference(name)
        for k in keys:
            ang, tr = SC.pose_errors(ref[k], eye)
            assert ang > 1e-3 or tr > 1e-3, (name, k)  # the alignment moved the pose
    assert (SC.reference("icp_batch")["status"] == 0).all()


def test_builder_reference_covers_the_four_variants():
    assert set(SC.BUILDER_VARIANTS) == {(1, False), (1, True), (3, False), (3, True)}
    assert SC.BUILDER_FRAMES["S"] != SC.BUILDER_FRAMES["L"]
    ref = SC.reference("builder")
    plain, filtered = ref["size0.L3.B0.frame0.level0.points"], ref["size0.L3.B1.frame0.level0.points"]
    assert plain.shape == filtered.shape and (plain != filtered).any()  # the filter changes the depths
    mask = ref["size1.L3.B1.frame0.level2.mask"]
    assert mask.shape == (SC.IMAGES["S"][1][1] >> 2, SC.IMAGES["S"][1][0] >> 2) and 0 < (mask != 0).sum()
    assert (ref["size0.L1.B0.frame0.level0.mask"] == 0).any()  # invalid pixels


def test_image_reference_keeps_a_part_of_every_image():
    ref = SC.reference("from_images")
    for i, (w, h) in enumerate(SC.IMAGES["S"]):
        assert 0 < len(ref[f"cloud{i}.points"]) < w * h and len(ref[f"cloud{i}.colors"]) == len(ref[f"cloud{i}.points"])
    assert len(SC.images("L")) != len(SC.images("S"))


@pytest.mark.parametrize("name", ["render", "map_render"])
def test_render_references_have_pixels_with_ties_and_empty_pixels(name):
    ref = SC.reference(name)
    for i, (w, h) in enumerate(SC.IMAGES["S"]):
        mask, index = ref[f"image{i}.mask"], ref[f"image{i}.index"]
        assert mask.shape == (h, w) and 0 < mask.sum() < w * h, (name, i)
        winners = np.unique(index[mask != 0])
        assert len(winners) < mask.sum(), (name, i)  # a footprint covers several pixels


def test_rendered_view_has_equal_depth_ties_that_the_lower_row_wins():
    """Two rows at the same place compete for every pixel of their footprint at the same depth, and the rule gives it to
    the lower row: scene()'s four copied rows wherever they are seen, and TIE_ROWS, which every S camera sees."""
    points = SC.render_cloud("S")[0]
    rows, inverse, counts = np.unique(points, axis=0, return_inverse=True, return_counts=True)
    pairs = [np.flatnonzero(inverse.reshape(-1) == g) for g in np.flatnonzero(counts > 1) if np.isfinite(rows[g]).all()]
    assert len(pairs) == 5 and all(len(p) == 2 for p in pairs) and any(tuple(p) == SC.TIE_ROWS for p in pairs)
    ref = SC.reference("render")
    for i in range(len(SC.IMAGES["S"])):
        won = set(ref[f"image{i}.index"][ref[f"image{i}.mask"] != 0].tolist())
        assert SC.TIE_ROWS[0] in won, i
        assert not any(int(hi) in won for _, hi in pairs), i
