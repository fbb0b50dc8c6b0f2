"""A numpy restatement of the TSDF rules (a3d_tsdf_volume_integrate / a3d_tsdf_volume_raycast), written from their
statement in include/align3d_hip.h and from the reference: CameraIntrinsics::project and the rounding of
PinholeCamera::project_to_image (src/camera.rs:64-70, :177-202) and Transform::transform_vector / transform_normal
(src/transform.rs:138-153), through render_restatement's camera_points, project and round_half_away.  Never from the
kernel.

All arithmetic is f32 with every operation rounded on its own (numpy float32 arrays do exactly that).  Voxels are held as
[nz, ny, nx] arrays, x fastest, as the library stores them.  A pose is (t_xyz, q_ijkw)."""
import numpy as np

from render_restatement import camera_normals, camera_points, project, round_half_away

F = np.float32
INF = F(np.inf)

# why a ray of the raycast ended
RAN_OUT, HIT, LEFT_FROM_BEHIND = 0, 1, 2


def conjugate_pose(pose):
    """The rotation of the inverse pose (the only part of world_to_camera the raycast uses: normals are rotated)."""
    q = np.asarray(pose[1], F)
    return np.zeros(3, F), np.asarray([-q[0], -q[1], -q[2], q[3]], F)


class Volume:
    def __init__(self, dims, voxel_size, origin, truncation, max_weight, colors):
        self.nx, self.ny, self.nz = (int(d) for d in dims)
        self.v, self.tau, self.max_weight = F(voxel_size), F(truncation), F(max_weight)
        self.origin = np.asarray(origin, F)
        shape = (self.nz, self.ny, self.nx)
        self.D, self.W = np.zeros(shape, F), np.zeros(shape, F)
        self.C = np.zeros(shape + (3,), np.uint8) if colors else None
        # for the tests' own checks, never read by a rule: the (voxel, row, col) of every update of the last frame, and the
        # least and greatest colour channel any frame produced BEFORE its cast to u8
        self.last_pixels, self.color_range = None, [np.inf, -np.inf]
        k, j, i = np.meshgrid(np.arange(self.nz), np.arange(self.ny), np.arange(self.nx), indexing="ij")
        # step 1: pw = origin + (float)index * v
        self.pw = np.stack([self.origin[0] + i.astype(F) * self.v, self.origin[1] + j.astype(F) * self.v,
                            self.origin[2] + k.astype(F) * self.v], -1).astype(F).reshape(-1, 3)

    def copy(self):
        other = Volume.__new__(Volume)
        other.__dict__.update(self.__dict__)
        other.D, other.W = self.D.copy(), self.W.copy()
        other.C = None if self.C is None else self.C.copy()
        other.color_range = list(self.color_range)
        return other

    # ---- integrate ---------------------------------------------------------------------------------------------------

    def integrate(self, points, mask, colors, intrinsics, world_to_camera):
        """One frame: points [h, w, 3] f32 in the camera's frame, mask [h, w] u8, colors [h, w, 3] u8 (needed iff the
        volume has colours), intrinsics (fx, fy, cx, cy).  Returns the number of voxels the frame touched."""
        points, mask = np.asarray(points, F), np.asarray(mask, np.uint8)
        h, w = mask.shape
        fx, fy, cx, cy = intrinsics
        pc = camera_points(self.pw, world_to_camera)  # step 2
        z = pc[:, 2]
        with np.errstate(all="ignore"):
            alive = (z > F(0)) & (z < INF)
            u, v_ = project(pc, fx, fy, cx, cy)  # step 3
            ui, vi = round_half_away(u), round_half_away(v_)
            alive &= (ui >= F(0)) & (ui < F(w)) & (vi >= F(0)) & (vi < F(h))
            idx = np.nonzero(alive)[0]
            col, row = ui[idx].astype(np.int64), vi[idx].astype(np.int64)
            dz = points[row, col, 2]  # step 4
            keep = (mask[row, col] != 0) & (dz > F(0)) & (dz < INF)
            sdf = (dz - z[idx]).astype(F)  # step 5
            keep &= ~(sdf < -self.tau)
        idx, col, row, sdf = idx[keep], col[keep], row[keep], sdf[keep]
        self.last_pixels = (idx, row, col)
        d = np.minimum(F(1), (sdf / self.tau).astype(F)).astype(F)
        D, W = self.D.reshape(-1), self.W.reshape(-1)  # (views)
        w_old = W[idx]
        w_new = (w_old + F(1)).astype(F)  # step 6
        if self.C is not None:  # step 7
            C = self.C.reshape(-1, 3)
            c_in = np.asarray(colors, np.uint8)[row, col].astype(F)
            mixed = ((C[idx].astype(F) * w_old[:, None]).astype(F) + c_in).astype(F) / w_new[:, None]
            whole = np.floor((mixed.astype(F) + F(0.5)).astype(F))
            if whole.size:
                self.color_range = [min(self.color_range[0], float(whole.min())), max(self.color_range[1], float(whole.max()))]
            C[idx] = whole.astype(np.uint8)
        with np.errstate(all="ignore"):  # (an uploaded D of 3e38 overflows D * W: the rule's result is the infinity)
            D[idx] = (((D[idx] * w_old).astype(F) + d).astype(F) / w_new).astype(F)
        W[idx] = np.minimum(w_new, self.max_weight)
        return len(idx)

    # ---- raycast -----------------------------------------------------------------------------------------------------

    def voxel_coordinate(self, pc, camera_to_world):
        pw = camera_points(pc, camera_to_world)
        return ((pw - self.origin).astype(F) / self.v).astype(F)

    def tri(self, g):
        """Step 3 for rows g [n, 3]: (valid [n] bool, value [n] f32; the value of an invalid row means nothing)."""
        g = np.asarray(g, F)
        with np.errstate(all="ignore"):
            f0 = np.floor(g).astype(F)
            inside = np.ones(len(g), bool)
            for axis, n in enumerate((self.nx, self.ny, self.nz)):
                inside &= (f0[:, axis] >= F(0)) & ((f0[:, axis] + F(1)).astype(F) <= F(n - 1))
            i0 = np.where(inside[:, None], f0, F(0)).astype(np.int64)
            t = (g - f0).astype(F)
        i, j, k = i0[:, 0], i0[:, 1], i0[:, 2]
        valid = inside.copy()
        corner = {}
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    valid &= self.W[k + dk, j + dj, i + di] > F(0)
                    corner[di, dj, dk] = self.D[k + dk, j + dj, i + di]

        def lerp(a, b, s):
            return (a + (s * (b - a).astype(F)).astype(F)).astype(F)

        with np.errstate(all="ignore"):
            tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
            c00, c10 = lerp(corner[0, 0, 0], corner[1, 0, 0], tx), lerp(corner[0, 1, 0], corner[1, 1, 0], tx)
            c01, c11 = lerp(corner[0, 0, 1], corner[1, 0, 1], tx), lerp(corner[0, 1, 1], corner[1, 1, 1], tx)
            value = lerp(lerp(c00, c10, ty), lerp(c01, c11, ty), tz)
        return valid, value

    def raycast(self, intrinsics, width, height, camera_to_world, z_near, z_far, step):
        """The whole rule.  Returns a dict: points [h, w, 3] f32, mask [h, w] u8, normals [h, w, 3] f32, colors [h, w, 3]
        u8 or None, and for the tests' own checks `reason` [h, w] (RAN_OUT, HIT, LEFT_FROM_BEHIND), `started_behind`
        [h, w] bool (a first valid sample, or the first after an invalid one, had D <= 0) and `samples` = K."""
        fx, fy, cx, cy = (F(x) for x in intrinsics)
        z_near, z_far, step = F(z_near), F(z_far), F(step)
        K = int(np.floor((float(z_far) - float(z_near)) / float(step))) + 1  # f64 from the f32 values
        row, col = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
        xn = ((col.reshape(-1).astype(F) - cx).astype(F) / fx).astype(F)  # step 1
        yn = ((row.reshape(-1).astype(F) - cy).astype(F) / fy).astype(F)
        n = width * height
        have_prev, done = np.zeros(n, bool), np.zeros(n, bool)
        reason, started_behind = np.zeros(n, np.int64), np.zeros(n, bool)
        D_prev, z_prev, D_hit, z_hit = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        for k in range(K):  # step 2
            z_k = F(z_near + F(F(k) * step))
            pc = np.stack([(xn * z_k).astype(F), (yn * z_k).astype(F), np.full(n, z_k, F)], -1)
            valid, D = self.tri(self.voxel_coordinate(pc, camera_to_world))
            active = ~done  # step 4
            have_prev[active & ~valid] = False
            live = active & valid
            started_behind |= live & ~have_prev & (D <= F(0))
            paired = live & have_prev
            hit = paired & (D_prev > F(0)) & (D <= F(0))
            left = paired & (D_prev <= F(0)) & (D > F(0))
            D_hit[hit], z_hit[hit] = D[hit], z_k
            reason[hit], reason[left] = HIT, LEFT_FROM_BEHIND
            done |= hit | left
            go_on = live & ~hit & ~left
            have_prev[go_on] = True
            D_prev[go_on], z_prev[go_on] = D[go_on], z_k
            if done.all():
                break
        won = reason == HIT
        points, normals = np.zeros((n, 3), F), np.zeros((n, 3), F)
        colors = None if self.C is None else np.zeros((n, 3), np.uint8)
        if won.any():  # step 5
            s = (D_prev[won] / (D_prev[won] - D_hit[won]).astype(F)).astype(F)
            zs = (z_prev[won] + ((z_hit[won] - z_prev[won]).astype(F) * s).astype(F)).astype(F)
            ps = np.stack([(xn[won] * zs).astype(F), (yn[won] * zs).astype(F), zs], -1)
            points[won] = ps
            gs = self.voxel_coordinate(ps, camera_to_world)  # step 6
            G, all_valid = np.zeros((len(gs), 3), F), np.ones(len(gs), bool)
            for axis in range(3):
                e = np.zeros(3, F)
                e[axis] = 1
                ok_p, plus = self.tri((gs + e).astype(F))
                ok_m, minus = self.tri((gs - e).astype(F))
                all_valid &= ok_p & ok_m
                with np.errstate(all="ignore"):
                    G[:, axis] = (plus - minus).astype(F)
            with np.errstate(all="ignore"):
                length = np.sqrt((((G[:, 0] * G[:, 0]).astype(F) + (G[:, 1] * G[:, 1]).astype(F)).astype(F)
                                  + (G[:, 2] * G[:, 2]).astype(F)).astype(F)).astype(F)
                good = all_valid & (length > F(0)) & (length < INF)
                unit = (G[good] / length[good][:, None]).astype(F)
            nrm = np.zeros((len(gs), 3), F)
            nrm[good] = camera_normals(unit, conjugate_pose(camera_to_world))
            normals[won] = nrm
            if colors is not None:  # step 7
                at = [np.clip(round_half_away(gs[:, axis]), F(0), F(m - 1)).astype(np.int64)
                      for axis, m in enumerate((self.nx, self.ny, self.nz))]
                colors[won] = self.C[at[2], at[1], at[0]]
        shape = (height, width)
        return {"points": points.reshape(shape + (3,)), "mask": won.astype(np.uint8).reshape(shape),
                "normals": normals.reshape(shape + (3,)), "colors": None if colors is None else colors.reshape(shape + (3,)),
                "reason": reason.reshape(shape), "started_behind": started_behind.reshape(shape), "samples": K}
