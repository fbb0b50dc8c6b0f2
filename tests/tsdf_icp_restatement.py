"""The field query of the TSDF volume and the point-to-SDF ICP on top of it (include/align3d_hip.h, "Aligning against
the volume"), restated on the host from the header text.  It is the expected value of the TSDF ICP tests, never the code
under test.

The query is plain numpy float32 (each operation rounded on its own, IEEE divide and sqrt) on top of
tsdf_restatement.Volume.tri, the raycast rule's trilinear sample.  Poses are applied by the oracle (orc_transform_points /
orc_transform_normals).  The gates, the residual, the Jacobian, one Gauss-Newton iteration and the loop with its
best-pose rule are those of voxel_map_icp_restatement.MapRestatement (src/icp/pcl_icp.rs:59-106), which this class
borrows: only the association differs."""
import numpy as np

import oracle_lib as O
import tsdf_restatement as TS
from voxel_map_icp_restatement import MapRestatement, transform_normals

F = np.float32
INF = F(np.inf)
NAN_BITS = 0x7FC00000


class FieldRestatement:
    """A volume's field as an alignment target.  `volume`: a tsdf_restatement.Volume whose D and W are set."""

    def __init__(self, volume):
        self.volume = volume

    def sample(self, queries, pose=None):
        """Steps 1-5 for queries [m, 3]: (d [m] f32, n [m, 3] f32, value [m] bool, direction [m] bool).  `pose`: a PoseC
        applied first.  d is the NaN 0x7FC00000 without a value (and for any NaN), n is +0 without a direction."""
        vol = self.volume
        q = np.ascontiguousarray(queries, F).reshape(-1, 3)
        if pose is not None:
            q = O.transform_points(pose, q)
        m = len(q)
        with np.errstate(all="ignore"):
            g = ((q - vol.origin).astype(F) / vol.v).astype(F)  # step 1
            value, D = vol.tri(g)  # step 2
            d = (D * vol.tau).astype(F)  # step 5
            direction = value & (np.abs(D) < F(1))  # step 3 (a NaN fails)
            G = np.zeros((m, 3), F)
            for axis in range(3):  # step 4
                e = np.zeros(3, F)
                e[axis] = 1
                ok_p, plus = vol.tri((g + e).astype(F))
                ok_m, minus = vol.tri((g - e).astype(F))
                direction &= ok_p & ok_m
                G[:, axis] = (plus - minus).astype(F)
            length = np.sqrt((((G[:, 0] * G[:, 0]).astype(F) + (G[:, 1] * G[:, 1]).astype(F)).astype(F)
                              + (G[:, 2] * G[:, 2]).astype(F)).astype(F)).astype(F)
            direction &= (length > F(0)) & (length < INF)
            n = np.zeros((m, 3), F)
            n[direction] = (G[direction] / length[direction][:, None]).astype(F)
        d = np.where(value & ~np.isnan(d), d, np.uint32(NAN_BITS).view(F)).astype(F)
        return d, n, value, direction

    def point_terms_kept(self, src_points, src_normals, pose, params):
        """(residuals [k] f32, Jacobians [k, 6] f32, source indices [k]) of the points that have a correspondence and pass
        both gates under `pose` (a PoseC), in source order."""
        p = O.transform_points(pose, src_points)
        sn = transform_normals(pose, src_normals)
        d, n, _, direction = self.sample(p)
        with np.errstate(all="ignore"):
            d2 = (d * d).astype(F)
            max_d2 = F(params.max_distance) * F(params.max_distance)
            keep = direction & ~(d2 > max_d2)
            kept = np.flatnonzero(keep)
            p, sn, d, tn = p[keep], sn[keep], d[keep], n[keep]
            tp = (p - (d[:, None] * tn).astype(F)).astype(F)  # t = q - d * n per component
            dot = (sn[:, 0] * tn[:, 0] + sn[:, 1] * tn[:, 1]) + sn[:, 2] * tn[:, 2]
            keep = ~O.acos_gate_rejects(dot, params.max_normal_angle, strict=True) if len(dot) else np.zeros(0, bool)
            kept = kept[keep]
            p, tp, tn = p[keep], tp[keep], tn[keep]
            e = tp - p
            r = (e[:, 0] * tn[:, 0] + e[:, 1] * tn[:, 1]) + e[:, 2] * tn[:, 2]
            tw = np.stack([p[:, 1] * tn[:, 2] - p[:, 2] * tn[:, 1], p[:, 2] * tn[:, 0] - p[:, 0] * tn[:, 2],
                           p[:, 0] * tn[:, 1] - p[:, 1] * tn[:, 0]], axis=1)
        J = np.ascontiguousarray(np.concatenate([tn, tw], axis=1), F)
        assert r.dtype == F and J.shape == (len(r), 6)
        return np.ascontiguousarray(r), J, kept

    point_terms = MapRestatement.point_terms
    gn_state = MapRestatement.gn_state
    accumulate = MapRestatement.accumulate
    align = MapRestatement.align


# ---- the analytic scene of the tests ---------------------------------------------------------------------------------------

DIMS, VOXEL, ORIGIN = (32, 32, 32), 0.05, (0.013, -0.02, 0.021)
PLANES = (0.3, 0.25, 0.35)  # x = 0.3, y = 0.25, z = 0.35: a room corner, the room on their positive sides
CENTRE, RADIUS = (0.9, 0.8, 0.85), 0.25


def signed_distance(p):
    """The scene's signed distance at p [..., 3] in f64: the minimum of the three plane distances and the sphere's."""
    p = np.asarray(p, np.float64)
    planes = p - np.asarray(PLANES)
    sphere = np.linalg.norm(p - np.asarray(CENTRE), axis=-1) - RADIUS
    return np.minimum(planes.min(axis=-1), sphere)


def corner_volume():
    """The scene as a tsdf_restatement.Volume: D = clip(sd / tau, -1, 1) at the voxel centres, W = 1 where sd >= -tau."""
    vol = TS.Volume(DIMS, VOXEL, ORIGIN, float(F(4.0) * F(VOXEL)), 64, False)
    sd = signed_distance(vol.pw.astype(np.float64)).reshape(vol.D.shape)
    tau = float(vol.tau)
    vol.D[...] = np.clip(sd / tau, -1.0, 1.0).astype(F)
    vol.W[...] = (sd >= -tau).astype(F)
    return vol


def corner_surfaces(seed, n, noise=0.002):
    """([n, 3] points, [n, 3] outward unit normals) on the three walls and the sphere, a quarter each, shuffled; `noise`:
    standard deviation of the displacement along the normal.  The walls are sampled inside the room up to 1.3."""
    rng = np.random.default_rng(seed)
    a = n // 4
    points, normals = [], []
    for axis in range(3):
        p = np.stack([rng.uniform(PLANES[k], 1.3, size=a) for k in range(3)], axis=1)
        p[:, axis] = PLANES[axis]
        e = np.zeros(3)
        e[axis] = 1.0
        points.append(p), normals.append(np.tile(e, (a, 1)))
    radial = rng.normal(size=(n - 3 * a, 3))
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    points.append(np.asarray(CENTRE) + RADIUS * radial), normals.append(radial)
    points, normals = np.concatenate(points), np.concatenate(normals)
    points = points + normals * rng.normal(size=(n, 1)) * noise
    order = rng.permutation(n)
    return points[order].astype(F), normals[order].astype(F)
