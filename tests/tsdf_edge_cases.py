"""Inputs that reach, by construction, the clauses of the TSDF integrate and raycast rules (a3d_tsdf_volume_integrate /
a3d_tsdf_volume_raycast in include/align3d_hip.h) that a few fused random frames never reach.  numpy only: no GPU and no
library import.

  A  layered_cases          fields whose D and W depend on the z layer alone, on exact numbers: hits with s == 1, -0, a ray
                            that leaves from behind, a NaN that swallows a crossing, a hole, a denormal pair, corners whose
                            difference overflows, infinities, and hits whose g* lies on k + 0.5 with k even
  B  one_cell_case,         the 2 x 2 x 2 volume, and 1024 x 2 x 2 in its three orientations
     stick_case
  C  weight_case            uploaded W up to 2^24 and around a small cap, D down to denormals and up to 3e38, colours at
                            0, 1, 127, 128, 254, 255
  D  mixed_frames,          one call of frames that differ in width, height and intrinsics; calls of 64, 65, 128 and 129
     chunk_call             frames
  E  scene_frames, MODEL_*, a model image fused back into a second volume, with voxels on its last pixel and last row
     SECOND_*
  F  k_cases, SHAPE_CAMERAS the sample count at 4096 and 4097 and just below an integer; 1 x 1, 257 x 1 and 1 x 300 images

Every builder returns plain dicts of numpy arrays and Python numbers.  A field is (D, W, C): [nz, ny, nx] f32, f32 and
[nz, ny, nx, 3] u8.  A frame is a dict points [h, w, 3] f32, mask [h, w] u8, colors [h, w, 3] u8, intrinsics (fx, fy, cx,
cy), width, height.  A pose is camera_to_world as (t_xyz, q_ijkw).  tests/test_tsdf_edge_cases_cpu.py proves with the
restatement that each case is what it claims and that it changes under the slip it targets;
tests/test_gpu_tsdf_edges.py runs them on the device.  The expected value of a GPU test is always the restatement's."""
import numpy as np

F = np.float32
EYE = (np.zeros(3, F), np.asarray([0, 0, 0, 1], F))
NAN, INF = float("nan"), float("inf")
ROOT_HALF = float(np.sqrt(F(0.5)))


def field_colors(dims):
    """A distinct colour per voxel, from its indices (every dimension at most 8 here)."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([30 * i + j, 30 * j + k, 30 * k + i], -1).astype(np.uint8)


# ---- the seeded frames and poses of test_gpu_tsdf.py, as plain arrays ------------------------------------------------------

CAMERAS = {"24x20": (21.3, 20.7, 11.5, 9.75, 24, 20), "65x3": (40.0, 41.0, 32.0, 1.0, 65, 3),
           "1x1": (1.5, 1.25, 0.0, 0.0, 1, 1), "300x1": (150.0, 2.0, 149.5, 0.0, 300, 1)}


def seeded_frame(seed, cam, depth=(0.15, 1.2)):
    """test_gpu_tsdf._frame: a smooth surface with a step in it, mask holes, and kept pixels whose z is NaN, +-inf, 0 or
    negative.  cam = (fx, fy, cx, cy, width, height)."""
    fx, fy, cx, cy, w, h = cam
    rng = np.random.default_rng(seed)
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lo, hi = depth
    z = lo + (hi - lo) * (0.5 + 0.5 * np.sin(cols * rng.uniform(0.1, 0.5) + rng.uniform(0, 6)) * np.cos(rows * rng.uniform(0.1, 0.7)))
    z = np.where(cols > w * rng.uniform(0.3, 0.7), z, z * 0.6 + 0.05).astype(F)
    mask = (rng.random((h, w)) < 0.85).astype(np.uint8)
    bad = rng.permutation(w * h)[:6]
    z.reshape(-1)[bad[:min(6, len(bad))]] = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0], F)[:len(bad)]
    mask.reshape(-1)[bad] = 1
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        pts = np.stack([(cols - cx) * z64 / fx, (rows - cy) * z64 / fy, z64], -1).astype(F)
    return {"points": pts, "mask": mask, "colors": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "intrinsics": (fx, fy, cx, cy), "width": w, "height": h}


def unit_pose(seed):
    """test_gpu_tsdf._unit_pose: a seeded rotation, normalised in f32, and a translation within half a metre."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q = (q / np.linalg.norm(q)).astype(F)
    q = (q / np.sqrt(np.sum(q.astype(np.float64) ** 2))).astype(F)
    return rng.uniform(-0.5, 0.5, 3).astype(F), q


# ---- A. layered fields -----------------------------------------------------------------------------------------------------

# Sample k of the centre ray sits exactly on layer k: g = (2, 2, k), t == 0 on every axis.  Sample 7 has g.z == nz - 1 and is
# invalid.  The outer columns meet g.x == 0 (valid) at z = 1 and g.x == nx - 1 == 5 (invalid) at z = 1.5.
LAYERED = {"dims": (6, 5, 8), "v": 0.25, "origin": (-0.5, -0.5, 0.5), "intrinsics": (4.0, 4.0, 2.0, 2.0), "width": 5, "height": 5,
           "z_near": 0.5, "z_far": 2.25, "step": 0.25, "centre": (2, 2)}
# With this origin the centre ray has g.x == g.y == 2.5 at every depth: a hit's colour pick is a tie on x and y, 2 is even.
TIE_ORIGIN = (-0.625, -0.625, 0.5)
DENORMAL = float(F(1e-45))  # 2^-149, the smallest f32

# name -> (D per layer, W per layer or None, step, origin or None); the profile's last value fills the layers left
PROFILES = {
    "exact zero": ([1, .5, 0.0, -.5, -1], None, 0.25, None),
    "minus zero": ([1, .5, -0.0, -.5, -1], None, 0.25, None),
    "zero first": ([0.0, 1, -1], None, 0.25, None),
    "nan swallows": ([1, NAN, -1, -1, 1], None, 0.25, None),
    "hole": ([1, 1, -1], [1, 0, 1], 0.125, None),
    "denormal pair": ([1, DENORMAL, -DENORMAL, -1], None, 0.25, None),
    "huge": ([3e38, -3e38, 3e38, -3e38, 1, -1], None, 0.125, None),
    "infinite": ([1, INF, -1, 1, -INF, 1, -1], None, 0.25, None),
    "infinite, half steps": ([1, INF, -1, 1, -INF, 1, -1], None, 0.125, None),
    "denormal tie": ([1, 1, DENORMAL, -DENORMAL, -1], None, 0.25, TIE_ORIGIN),
    "plain tie": ([1, 1, .5, -.5, -1], [3, 2, 1, 1, 7], 0.25, TIE_ORIGIN),
}


def layered_field(profile, weights=None, dims=LAYERED["dims"]):
    nx, ny, nz = dims
    d = list(profile) + [profile[-1]] * (nz - len(profile))
    w = [1] * nz if weights is None else list(weights) + [weights[-1]] * (nz - len(weights))
    D = np.broadcast_to(np.asarray(d, F)[:, None, None], (nz, ny, nx)).copy()
    W = np.broadcast_to(np.asarray(w, F)[:, None, None], (nz, ny, nx)).copy()
    return D, W, field_colors(dims)


def layered_cases():
    cases = []
    for name, (profile, weights, step, origin) in PROFILES.items():
        case = dict(LAYERED, name=name, step=step, profile=profile)
        if origin is not None:
            case["origin"] = origin
        case["D"], case["W"], case["C"] = layered_field(profile, weights)
        cases.append(case)
    return cases


# F: other image shapes over the layered field: one pixel, a row that crosses a block of 256 threads, one column
SHAPE_CAMERAS = {"1x1": (4.0, 4.0, 0.0, 0.0, 1, 1), "257x1": (256.0, 256.0, 128.0, 0.0, 257, 1),
                 "1x300": (300.0, 300.0, 0.0, 149.5, 1, 300)}


# ---- F. the K rule ---------------------------------------------------------------------------------------------------------

def samples(z_near, z_far, step):
    """K of the rule: f64 arithmetic on the f32 values."""
    return int(np.floor((float(F(z_far)) - float(F(z_near))) / float(F(step)))) + 1


K_STEP = 2.0 ** -12
K_CAMERA = (4.0, 4.0, 1.0, 0.5, 3, 2)
K_PROFILE = [1, 1, 1, 1, 1, 1, -1, -1]  # the crossing lies between z = 1.75 and 2: past sample 3072 of 4096


def k_cases():
    """(name, z_near, z_far, step, K or None for refused), every value an exact f32."""
    below_two = float(np.nextafter(F(2.0), F(0)))
    return [
        ("4096, the last sample is z_far", 1.0, 1.0 + 4095 * K_STEP, K_STEP, 4096),
        ("4096, a quotient just below 4096", 1.0, below_two, K_STEP, 4096),
        ("4097", 1.0, 2.0, K_STEP, None),
        ("8, the last sample is z_far", 0.25, 2.0, 0.25, 8),  # (sample 7 is layer 6, the first behind the surface)
        ("7, a quotient just below 7", 0.25, below_two, 0.25, 7),
        ("a tenth", 0.3, 1.3, 0.1, samples(0.3, 1.3, 0.1)),
    ]


# ---- B. the smallest volume and the longest ones -----------------------------------------------------------------------------

def one_cell_case():
    """2 x 2 x 2 with v = 1 and its origin at (0, 0, 1): the one cell is [0, 1)^2 x [1, 2).  Layer 0 is in front of the
    surface, layer 1 behind it.  The camera looks down z; column 2 reaches x == 1.0 at z == 2, and the sample at z == 2 has
    g.z == 1.0 on every ray: invalid."""
    D = np.asarray([[[0.5, 0.75], [0.625, 1.0]], [[-1.0, -0.5], [-0.75, -0.25]]], F)
    C = np.arange(24, dtype=np.uint8).reshape(2, 2, 2, 3) * 10 + 1
    return {"dims": (2, 2, 2), "v": 1.0, "origin": (0.0, 0.0, 1.0), "D": D, "W": np.full((2, 2, 2), 2, F), "C": C,
            "intrinsics": (4.0, 4.0, 0.0, 0.0), "width": 3, "height": 3,
            # (name, z_near, z_far, step): the second has its samples at g.z == 0.125, where D > 0 still, 1.0 and 1.875:
            # only a valid sample at g.z == 1.0 could make it a hit
            "rays": (("through the cell", 1.0, 2.25, 0.25), ("the far face", 1.125, 3.0, 0.875))}


STICK_V = 0.01
STICK_CAMERA = (4000.0, 4000.0, 1.0, 0.5, 3, 2)  # six rays that stay inside one cell over ten metres
ACROSS_CAMERA = (21.3, 20.7, 12.0, 10.0, 24, 20)  # column 12 and row 10 look straight ahead, through the cell
# camera_to_world rotations that turn the camera's +z into the world's +x, -x, +y, -y
TURN = {(0, 1): (0.0, ROOT_HALF, 0.0, ROOT_HALF), (0, -1): (0.0, -ROOT_HALF, 0.0, ROOT_HALF),
        (1, 1): (-ROOT_HALF, 0.0, 0.0, ROOT_HALF), (1, -1): (ROOT_HALF, 0.0, 0.0, ROOT_HALF),
        (2, 1): (0.0, 0.0, 0.0, 1.0), (2, -1): (0.0, 1.0, 0.0, 0.0)}


def stick_case(axis):
    """1024 voxels along `axis` (0: x, 1: y, 2: z), 2 x 2 across, v = 1 cm.  An uploaded field with a crossing about every
    63 voxels along the stick and one across it; raycasts along the stick from either end and across it at the far end;
    two seeded frames to fuse, one that sees the stick's middle and one that sees its far end."""
    dims = [2, 2, 2]
    dims[axis] = 1024
    nx, ny, nz = dims
    origin = np.asarray([-0.3, 0.2, 0.9], F)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    along = (i, j, k)[axis]
    across = i + j + k - along
    D = (0.5 * np.cos(0.05 * along) + 0.9 * (1 - across)).astype(F)
    rng = np.random.default_rng(40 + axis)
    W = rng.integers(1, 4, D.shape).astype(F)
    W.reshape(-1)[rng.permutation(D.size)[:5]] = 0
    C = rng.integers(0, 256, D.shape + (3,), dtype=np.uint8)
    unit = np.zeros(3)
    unit[axis] = 1.0
    mid = origin.astype(np.float64) + 0.5 * STICK_V  # the middle of the cross-section, at index 0
    far = mid + unit * (1023 * STICK_V)
    rays = [("along, upwards", STICK_CAMERA, ((mid - 0.2 * unit).astype(F), np.asarray(TURN[axis, 1], F)), 0.15, 10.5, 0.004),
            ("along, downwards", STICK_CAMERA, ((far + 0.2 * unit).astype(F), np.asarray(TURN[axis, -1], F)), 0.15, 10.5, 0.004)]
    # across: look at the last 60 cm of the stick from a metre away, along another axis
    view = (axis + 1) % 3 if axis == 2 else 2
    off = np.zeros(3)
    off[view] = 1.0
    eye = far - 0.3 * unit - off
    rays.append(("across", ACROSS_CAMERA, (eye.astype(F), np.asarray(TURN[view, 1], F)), 0.99, 1.012, 0.0005))
    # frames: the seeded wall a metre away, seen from a metre in front of the stick's middle and of its far end
    frames, poses = [], []
    for f, at in enumerate((mid + unit * (500 * STICK_V), far - 0.1 * unit)):
        frames.append(seeded_frame(60 + 10 * axis + f, CAMERAS["24x20"], depth=(0.9, 1.15)))
        poses.append(((at - off).astype(F), np.asarray(TURN[view, 1], F)))
    return {"name": "x".join(str(d) for d in dims), "axis": axis, "dims": tuple(dims), "v": STICK_V, "origin": origin,
            "tau": 0.5, "D": D, "W": W, "C": C, "rays": rays, "frames": frames, "poses": poses}


# ---- C. integrate on uploaded fields -----------------------------------------------------------------------------------------

SMALL_CAP = 5
TOP = 1 << 24
WEIGHTS = (0, 1, TOP - 2, TOP - 1, TOP, SMALL_CAP - 1, SMALL_CAP, SMALL_CAP + 1, 1000000)
DISTANCES = (0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-39, -1e-39, 0.99999994, -0.99999994, 3e38, -3e38)
CHANNELS = (0, 1, 127, 128, 254, 255)


def weight_case():
    """12 x 9 x 5 voxels of pitch 1 / 4 from (0, 0, 1): D runs over DISTANCES along x, W over WEIGHTS along y.  The camera
    (fx = fy = 4, cx = cy = 0, no pose) sees voxel (i, j, 0) at pixel (i, j) exactly and voxel (i, j, 4), at z == 2, at
    (i / 2, j / 2): a tie for every odd index.  With tau == 1 every voxel is within the truncation of both frames, and
    pixel (col, row) of the first frame has depth 1 + ((col + row) % 5) / 8: where that is 1, layer 0 gets d == 0 and a
    denormal D stays one."""
    nx, ny, nz = len(DISTANCES), len(WEIGHTS), 5
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    D = np.asarray(DISTANCES, F)[i]
    W = np.asarray(WEIGHTS, F)[j]
    ch = np.asarray(CHANNELS, np.uint8)
    C = np.stack([ch[(i + k) % 6], ch[(j + 2 * k) % 6], ch[(i + j + k) % 6]], -1)
    frames = []
    rows, cols = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    for f in range(2):
        z = (1.0 + ((cols + rows + 2 * f) % 5) / 8.0 + 0.5 * f).astype(F)
        pts = np.stack([cols * z / 4.0, rows * z / 4.0, z], -1).astype(F)
        colors = np.stack([ch[(cols + f) % 6], ch[(rows + 3 * f) % 6], ch[(cols + rows) % 6]], -1)
        frames.append({"points": pts, "mask": np.ones((ny, nx), np.uint8), "colors": colors,
                       "intrinsics": (4.0, 4.0, 0.0, 0.0), "width": nx, "height": ny})
    return {"dims": (nx, ny, nz), "v": 0.25, "origin": (0.0, 0.0, 1.0), "tau": 1.0, "D": D, "W": W, "C": C,
            "frames": frames, "poses": [EYE, EYE], "caps": (TOP, SMALL_CAP)}


# ---- D. the frame table --------------------------------------------------------------------------------------------------------

TABLE_VOLUME = ((16, 12, 10), 0.1, (-0.8, -0.6, -0.5))


def mixed_frames():
    """Ten frames of four sizes through four cameras, each from its own pose."""
    order = ("24x20", "65x3", "1x1", "24x20", "300x1", "65x3", "24x20", "65x3", "300x1", "1x1")
    frames = [seeded_frame(700 + f, CAMERAS[name], depth=(0.15, 0.9)) for f, name in enumerate(order)]
    for frame in frames:  # (one pixel: no room for the six bad depths)
        if frame["width"] * frame["height"] == 1:
            frame["points"][0, 0] = (0.0, 0.0, 0.5)
            frame["mask"][0, 0] = 1
    return frames, [unit_pose(850 + f) for f in range(len(order))]


CHUNK_SIZES = (64, 65, 128, 129)
CHUNK_POOL = 12


def chunk_pool():
    """Twelve seeded frames of the two existing cameras: the calls below reuse them."""
    return [seeded_frame(900 + f, CAMERAS["24x20" if f % 3 else "65x3"]) for f in range(CHUNK_POOL)]


def chunk_call(n):
    """(pool index, pose) of the n frames of a call: images repeat, twice in a row at the chunk's cut, every pose is new."""
    picks = [(5 * f) % CHUNK_POOL for f in range(n)]
    if n > 64:
        picks[64] = picks[63]
    return picks, [unit_pose(1000 + f) for f in range(n)]


# ---- E. an image made on the device ----------------------------------------------------------------------------------------------

SCENE = ((16, 12, 10), 0.1, (-0.8, -0.6, 0.5), 0.3)  # test_gpu_tsdf.SCENE
SCENE_POSES = (EYE, (np.asarray((0.1, -0.05, 0.0), F), np.asarray((0.0, 0.08715574, 0.0, 0.9961947), F)),
               (np.asarray((-0.12, 0.04, 0.02), F), np.asarray((0.0610485, 0.0, 0.0, 0.99813479), F)))


def scene_frames():
    """The three frames test_gpu_tsdf._scene fuses."""
    return [seeded_frame(50 + f, CAMERAS["24x20"], depth=(0.9, 1.15)) for f in range(3)]


MODEL_CAMERA = (24.0, 24.0, 5.5, 4.5, 12, 10)
MODEL_RAY = (EYE, 0.3, 1.6, 0.15)  # camera_to_world, z_near, z_far, step
# the second volume lies around the last pixel's ray (xn = 0.23, yn = 0.19) where it meets the wall
SECOND_VOLUME = ((12, 10, 8), 0.05, (-0.1, -0.1, 0.8), 0.2)
SECOND_POSES = (EYE, (np.asarray((0.03, -0.02, 0.01), F), np.asarray((0.0, 0.02617695, 0.0, 0.99965732), F)))
RENDER_RADIUS = 0.03
