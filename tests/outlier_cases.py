"""Clouds that the outlier tests share (test_cloud_outliers_cpu.py, test_gpu_cloud_outliers.py)."""
import numpy as np

from test_cloud_normals_cpu import plane_and_sphere

RADIUS = 0.15  # about 70 plane points and 17 sphere points within it
N_OUTLIERS = 30


def effectiveness_cloud():
    """(points [1530, 3] f32, is_outlier [1530] bool): plane_and_sphere() plus 30 seeded points that are at least 3 RADIUS
    from every other point of the cloud, shuffled."""
    rng = np.random.default_rng(2024)
    inliers = plane_and_sphere().astype(np.float64)
    rows = [inliers]
    n = 0
    while n < N_OUTLIERS:
        c = rng.uniform([-1.5, -1.5, -1.0], [3.5, 1.5, 2.0])
        if np.linalg.norm(np.concatenate(rows) - c, axis=1).min() >= 3 * RADIUS + 1e-3:
            rows.append(c[None])
            n += 1
    points = np.concatenate(rows).astype(np.float32)
    outlier = np.r_[np.zeros(len(inliers), bool), np.ones(N_OUTLIERS, bool)]
    perm = rng.permutation(len(points))
    return points[perm], outlier[perm]


def sentinel_edge_cloud(k):
    """Three well separated clusters of k, k + 1 and k + 2 points, each within a ball of 0.01: at radius 0.05 every row of
    a cluster has exactly k - 1, k and k + 1 others."""
    rng = np.random.default_rng(500 + k)
    parts = []
    for c, size in enumerate((k, k + 1, k + 2)):
        parts.append(np.float64([c * 1.0 + 0.37, -0.21, 0.63]) + rng.uniform(-0.005, 0.005, size=(size, 3)))
    return np.concatenate(parts).astype(np.float32)
