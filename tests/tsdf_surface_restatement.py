"""A numpy restatement of the TSDF surface rule (a3d_tsdf_volume_extract_surface), written from its statement in
include/align3d_hip.h alone: valid and inside voxels, owned edges, the vertex of a crossing edge, the vertex order and
marching tetrahedra on the Kuhn split with a table DERIVED here from the rule's paragraph.  Never from the kernel.  The
trilinear sample of the normal is the raycast rule's, tsdf_restatement.Volume.tri.

All arithmetic is f32 with every operation rounded on its own.  Voxels are [nz, ny, nx] arrays, x fastest."""
import os
import re

import numpy as np

import tsdf_restatement as T
from render_restatement import round_half_away

F = np.float32
INF = F(np.inf)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))  # xyz, xzy, yxz, yzx, zxy, zyx
CLOUD_CLASSES, MESH_CLASSES = (1, 2, 4), (1, 2, 3, 4, 5, 6, 7)


def class_offset(c):
    return c & 1, c >> 1 & 1, c >> 2 & 1


# ---- rule 5: the table -----------------------------------------------------------------------------------------------

def tetrahedron(permutation):
    """The four vertices (unit-cell corners as (x, y, z) tuples) of a permutation's tetrahedron."""
    p, q, _ = permutation
    v1 = [0, 0, 0]
    v1[p] = 1
    v2 = list(v1)
    v2[q] = 1
    return (0, 0, 0), tuple(v1), tuple(v2), (1, 1, 1)


def _corner(vertices, m, n):
    """The tetrahedron edge between local vertices m and n as (owner corner bits, class)."""
    lo, hi = vertices[min(m, n)], vertices[max(m, n)]
    d = [h - l for h, l in zip(hi, lo)]
    assert all(x in (0, 1) for x in d) and any(d)
    return lo[0] | lo[1] << 1 | lo[2] << 2, d[0] | d[1] << 1 | d[2] << 2


def _midpoint(corner):
    owner, c = corner
    a = np.asarray(class_offset(owner), np.float64)  # (the same bit layout)
    return a + 0.5 * np.asarray(class_offset(c), np.float64)


def derive_table():
    """table[t][s]: the triangles of tetrahedron t when bit n of s says local vertex n is inside; a triangle is three
    (owner corner bits, class) pairs, wound counter-clockwise seen from outside."""
    table = []
    for permutation in PERMUTATIONS:
        vertices = tetrahedron(permutation)
        row = []
        for s in range(16):
            inside = [n for n in range(4) if s >> n & 1]
            outside = [n for n in range(4) if not s >> n & 1]
            if len(inside) in (0, 4):
                triangles = []
            elif len(inside) in (1, 3):
                lone = inside[0] if len(inside) == 1 else outside[0]
                a, b, c = sorted(n for n in range(4) if n != lone)
                triangles = [[(lone, a), (lone, b), (lone, c)]]
            else:
                (p, q), (a, b) = inside, outside
                triangles = [[(p, a), (p, b), (q, b)], [(p, a), (q, b), (q, a)]]
            towards = (np.mean([vertices[n] for n in outside], axis=0) - np.mean([vertices[n] for n in inside], axis=0)
                       if triangles else None)
            wound = []
            for tri in triangles:
                corners = [_corner(vertices, m, n) for m, n in tri]
                p0, p1, p2 = (_midpoint(c) for c in corners)
                if np.dot(np.cross(p1 - p0, p2 - p0), towards) < 0:
                    corners[1], corners[2] = corners[2], corners[1]
                wound.append(tuple(corners))
            row.append(tuple(wound))
        table.append(tuple(row))
    return tuple(table)


def encode(table):
    """The committed form: one u64 per (tetrahedron, pattern): the triangle count in bits 0-1, then corner c of triangle
    t in the 6 bits from 2 + 18 t + 6 c: the owner's corner bits (x | y << 1 | z << 2) low, the class high."""
    out = np.zeros((6, 16), np.uint64)
    for t in range(6):
        for s in range(16):
            word = len(table[t][s])
            for k, tri in enumerate(table[t][s]):
                for c, (owner, cls) in enumerate(tri):
                    word |= (owner | cls << 3) << (2 + 18 * k + 6 * c)
            out[t, s] = word
    return out


def committed_table():
    """The 6 x 16 words as the kernel file holds them."""
    text = open(os.path.join(ROOT, "align3d_amd", "csrc", "tsdf_surface.hip")).read()
    body = re.search(r"TS_TET_TABLE\[6\]\[16\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    words = [int(w, 16) for w in re.findall(r"0x([0-9A-Fa-f]+)ull", body)]
    assert len(words) == 96, len(words)
    return np.asarray(words, np.uint64).reshape(6, 16)


TABLE = derive_table()


# ---- rules 1-5 over a volume -----------------------------------------------------------------------------------------

def volume_of(D, W, colors, voxel_size, origin):
    """A tsdf_restatement.Volume that holds the given field ([nz, ny, nx] f32 arrays, colours [nz, ny, nx, 3] u8 or None)."""
    D = np.asarray(D, F)
    nz, ny, nx = D.shape
    vol = T.Volume((nx, ny, nz), voxel_size, origin, 1.0, 1, colors is not None)
    vol.D, vol.W = D.copy(), np.asarray(W, F).copy()
    if colors is not None:
        vol.C = np.asarray(colors, np.uint8).copy()
    return vol


def valid_inside(vol, min_weight):
    with np.errstate(all="ignore"):
        valid = (vol.W >= F(min_weight)) & (np.abs(vol.D) < INF)  # (a NaN fails both)
        inside = valid & (vol.D <= F(0))                           # (-0 is inside)
    return valid, inside


def extract(vol, min_weight=1, want_faces=True):
    """The whole rule.  Returns a dict: points [V, 3] f32, normals [V, 3] f32, colors [V, 3] u8 or None, faces [F, 3] u32
    (None in the point-cloud form) and, for the tests' own checks, `voxel` [V] and `cls` [V]: each vertex's owner voxel
    number and edge class."""
    nx, ny, nz = vol.nx, vol.ny, vol.nz
    total = nx * ny * nz
    valid, inside = valid_inside(vol, min_weight)
    cross = np.zeros((nz, ny, nx, 8), bool)
    for c in (MESH_CLASSES if want_faces else CLOUD_CLASSES):  # rule 2
        ex, ey, ez = class_offset(c)
        a = (slice(0, nz - ez), slice(0, ny - ey), slice(0, nx - ex))
        b = (slice(ez, nz), slice(ey, ny), slice(ex, nx))
        cross[a + (c,)] = valid[a] & valid[b] & (inside[a] != inside[b])
    voxel, cls = np.nonzero(cross.reshape(total, 8))  # rule 4: ascending (voxel number, class)
    rank = np.full((total, 8), -1, np.int64)
    rank[voxel, cls] = np.arange(len(voxel))
    i, j, k = voxel % nx, voxel // nx % ny, voxel // (nx * ny)
    e = np.stack([cls & 1, cls >> 1 & 1, cls >> 2 & 1], -1)
    Dflat = vol.D.reshape(-1)
    Da, Db = Dflat[voxel], Dflat[voxel + e[:, 0] + nx * e[:, 1] + nx * ny * e[:, 2]]
    with np.errstate(all="ignore"):  # rule 3
        t = (Da / (Da - Db).astype(F)).astype(F)
        g = np.stack([(idx.astype(F) + (t * e[:, a].astype(F)).astype(F)).astype(F) for a, idx in enumerate((i, j, k))], -1)
        points = (vol.origin[None, :] + (g * vol.v).astype(F)).astype(F)
        G, all_valid = np.zeros((len(g), 3), F), np.ones(len(g), bool)
        for axis in range(3):
            unit = np.zeros(3, F)
            unit[axis] = 1
            ok_p, plus = vol.tri((g + unit).astype(F))
            ok_m, minus = vol.tri((g - unit).astype(F))
            all_valid &= ok_p & ok_m
            G[:, axis] = (plus - minus).astype(F)
        length = np.sqrt((((G[:, 0] * G[:, 0]).astype(F) + (G[:, 1] * G[:, 1]).astype(F)).astype(F)
                          + (G[:, 2] * G[:, 2]).astype(F)).astype(F)).astype(F)
        good = all_valid & (length > F(0)) & (length < INF)
        normals = np.zeros((len(g), 3), F)
        normals[good] = (G[good] / length[good][:, None]).astype(F)
    colors = None
    if vol.C is not None:
        at = [np.clip(round_half_away(g[:, axis]), F(0), F(m - 1)).astype(np.int64) for axis, m in enumerate((nx, ny, nz))]
        colors = vol.C[at[2], at[1], at[0]] if len(g) else np.zeros((0, 3), np.uint8)
    out = {"points": points.reshape(-1, 3), "normals": normals, "colors": colors, "faces": None, "voxel": voxel, "cls": cls}
    if not want_faces:
        return out
    # rule 5
    cell = np.ones((nz - 1, ny - 1, nx - 1), bool)
    corner_inside = []
    for corner in range(8):
        ox, oy, oz = class_offset(corner)
        s = (slice(oz, nz - 1 + oz), slice(oy, ny - 1 + oy), slice(ox, nx - 1 + ox))
        cell &= valid[s]
        corner_inside.append(inside[s])
    ck, cj, ci = np.nonzero(cell)
    number = (ck * ny + cj) * nx + ci
    rows = []
    for t, permutation in enumerate(PERMUTATIONS):
        vertices = tetrahedron(permutation)
        s = np.zeros(len(number), np.int64)
        for n, (x, y, z) in enumerate(vertices):
            s |= corner_inside[x | y << 1 | z << 2][ck, cj, ci].astype(np.int64) << n
        for pattern in range(1, 15):
            at = number[s == pattern]
            for m, tri in enumerate(TABLE[t][pattern]):
                index = []
                for owner, c in tri:
                    ox, oy, oz = class_offset(owner)
                    index.append(rank[at + ox + nx * oy + nx * ny * oz, c])
                rows.append(np.stack([at, np.full(len(at), t), np.full(len(at), m)] + index, -1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 6), np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]  # ascending (cell, tetrahedron, triangle)
    assert (rows[:, 3:] >= 0).all()
    out["faces"] = rows[:, 3:].astype(np.uint32)
    return out


# ---- what a closed, outward-wound surface looks like -----------------------------------------------------------------

def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def closed_and_oriented(faces):
    """Every undirected edge lies in exactly two triangles, once in each direction."""
    d = directed_edges(faces)
    if (d[:, 0] == d[:, 1]).any():
        return False
    pairs, counts = np.unique(d, axis=0, return_counts=True)
    if (counts != 1).any():
        return False
    back = {(int(a), int(b)) for a, b in pairs}
    return all((b, a) in back for a, b in back)


def euler_by_component(faces, n_vertices):
    """V - E + F of every connected component of the faces (vertices that no face uses are left out)."""
    f = np.asarray(faces, np.int64)
    parent = np.arange(n_vertices)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f:
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    root = np.asarray([find(x) for x in range(n_vertices)])
    used = np.zeros(n_vertices, bool)
    used[f.reshape(-1)] = True
    out = []
    for r in np.unique(root[used]):
        mine = f[root[f[:, 0]] == r]
        und = np.unique(np.sort(directed_edges(mine), axis=1), axis=0)
        out.append(int((used & (root == r)).sum()) - len(und) + len(mine))
    return out


def signed_volume(points, faces):
    p = np.asarray(points, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0)
