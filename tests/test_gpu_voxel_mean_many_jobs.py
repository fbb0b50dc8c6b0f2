"""voxel_mean.hip over batches of 65, 129 and 1000 clouds and over a cloud of more chunks than tiles, on the GPU, through
the raw ABI call.

What a batch of this size reaches and no smaller one does: the second and later trips of vmean_any_over's loop over the
jobs (k += 64), a find_job search of ten levels in all six passes, and per-job words (lens, dropped, the cursor of pass 3)
that travel back through cloud_of_job at indices past 63 with empty clouds in between.  The inputs are
voxel_mean_cases.batch_recipe: the clouds of test_cloud_batch_recipe_cpu.py (every third non-empty one without normals)
with seeded colours on every second non-empty one; test_voxel_mean_cases_cpu.py states what they have to contain.

The points and normals of a batch are views into one device allocation (the _Clouds of
test_gpu_cloud_batch_many_jobs.py), the colours views into one allocation of bytes, back to back, so a colour array starts
at any byte.  All outputs of a call lie in one canary-filled allocation (_Arena: five segments per cloud, a colour segment
rounded up to whole words), and every check compares the WHOLE allocation with the expectation laid out the same way.

Every comparison is on uint32 words, bit for bit; no tolerance appears.  The expected value is the numpy restatement
(voxel_mean_restatement.voxel_mean), computed once per cloud, never the library.  Every test prints its wall time."""
import ctypes as C
import time

import numpy as np
import pytest

import voxel_mean_cases as K
import voxel_mean_restatement as M
from align3d_amd import _abi
from test_cloud_batch_recipe_cpu import BATCHES, VOXEL, is_raw
from test_gpu_cloud_batch_many_jobs import UNSET, _Arena, _assert_words, _bits, _Clouds, _singled_out
from test_gpu_voxel_mean import _assert_matches, _call, _device_cloud, _uniform

pytestmark = pytest.mark.gpu

ORIGIN = (0.013, -0.4, 7.5)
PLANES = 5  # segments per cloud: points, normals, colours, index, counts


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"[wall time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


class _Batch:
    """The clouds of batch_recipe(n) resident on the device and what the restatement makes of each (computed once)."""

    def __init__(self, ctx, n, expected):
        self.ctx, self.n, self._expected = ctx, n, expected
        self.hosts = K.batch_recipe(n)
        self.w = _Clouds(ctx, n)
        self.lens = self.w.lens
        assert [nrm is None for _, nrm, _ in self.hosts] == self.w.bare and [len(p) for p, _, _ in self.hosts] == self.lens
        self.coloured = [col is not None for _, _, col in self.hosts]
        self.c_off = [int(x) for x in np.cumsum([0] + [3 * k if c else 0 for k, c in zip(self.lens, self.coloured)])]
        flat = np.concatenate([col.reshape(-1) for _, _, col in self.hosts if col is not None])
        self.d_colors = ctx.to_device(flat)
        assert sum(1 for o, c in zip(self.c_off, self.coloured) if c and o % 4) > sum(self.coloured) // 3  # off word boundaries

    def normals(self, i):
        return self.lens[i] > 0 and self.w.has_normals(i, True)

    def expected(self, i, origin=None):
        """(points, normals or None, colours or None, index, counts, dropped) of cloud i."""
        if (i, origin) not in self._expected:
            p, nrm, col = self.hosts[i]
            assert (nrm is not None) == bool(self.normals(i)) or self.lens[i] == 0
            self._expected[(i, origin)] = M.voxel_mean(p, nrm if self.normals(i) else None, col, VOXEL, origin)
        return self._expected[(i, origin)]

    def outputs(self, which):
        sizes = []
        for i in which:
            k = self.lens[i]
            sizes += [3 * k, 3 * k if self.normals(i) else 0, (3 * k + 3) // 4 if self.coloured[i] else 0, k, k]
        return _Arena(self.ctx, sizes)

    def call(self, which, arena, origin=None, capacities=None):
        """(status, lens, dropped) of the raw call over the clouds `which` into `arena` (outputs(which)), with every
        output a cloud's fields allow."""
        m = len(which)
        caps = [self.lens[i] for i in which] if capacities is None else list(capacities)
        lens, dropped = (C.c_uint64 * m)(*[UNSET] * m), (C.c_uint64 * m)(*[UNSET] * m)
        wanted = [(True, self.normals(i), self.coloured[i], True, True) for i in which]
        out = [(C.c_void_p * m)(*[arena.ptr(PLANES * k + plane) if wanted[k][plane] else None for k in range(m)])
               for plane in range(PLANES)]
        colors = (C.c_void_p * m)(*[self.d_colors.value + self.c_off[i] if self.coloured[i] else None for i in which])
        st = self.ctx.lib.a3d_point_clouds_voxel_mean_device(
            self.ctx.handle, self.w.views(which, True), colors, m, VOXEL, None if origin is None else (C.c_float * 3)(*origin),
            *out, (C.c_uint64 * m)(*caps), lens, dropped)
        return st, list(lens), list(dropped)

    def expectation(self, which, arena, origin=None):
        """(canvas, lens, dropped): the allocation as the call has to leave it."""
        canvas = arena.blank()
        as_bytes = canvas.view(np.uint8)
        for k, i in enumerate(which):
            p, nrm, col, index, counts, _ = self.expected(i, origin)
            arena.put(canvas, PLANES * k, _bits(p))
            if self.normals(i):
                arena.put(canvas, PLANES * k + 1, _bits(nrm))
            if self.coloured[i]:
                at = 4 * arena.offsets[PLANES * k + 2]
                as_bytes[at:at + col.size] = col.reshape(-1)  # (the last 0 to 3 bytes of the segment stay canary)
            arena.put(canvas, PLANES * k + 3, index)
            arena.put(canvas, PLANES * k + 4, counts)
        return canvas, [len(self.expected(i, origin)[3]) for i in which], [self.expected(i, origin)[5] for i in which]

    def free(self):
        self.w.free()
        self.ctx.free(self.d_colors)


@pytest.fixture(scope="module")
def batches(ctx):
    made, expected = {}, {}  # cloud i is the same in every batch size: one expectation serves all three

    def get(n):
        if n not in made:
            made[n] = _Batch(ctx, n, expected)
        return made[n]

    yield get
    for b in made.values():
        b.free()


@pytest.mark.parametrize("n", BATCHES)
def test_voxel_mean_of_every_job(batches, n):
    b = batches(n)
    which = list(range(n))
    arena = b.outputs(which)
    canvas, want_lens, want_dropped = b.expectation(which, arena)
    st, lens, dropped = b.call(which, arena)
    assert st == _abi.A3D_OK
    assert lens == want_lens and dropped == want_dropped
    assert all((lens[i], dropped[i]) == (0, 0) for i in which if b.lens[i] == 0) and 0 in b.lens
    if n > 65:  # raw-bits clouds behind job 64 drop what the restatement drops and keep the rest
        assert sum(1 for i in which[64:] if is_raw(i) and dropped[i] and lens[i]) >= (3 if n == 1000 else 1)
    assert any(b.normals(i) and b.coloured[i] for i in which) and any(not b.normals(i) and not b.coloured[i] for i in which)
    _assert_words(arena.read(), canvas, f"voxel mean of {n}")
    arena.free()


@pytest.mark.parametrize("n", BATCHES)
def test_capacity_one_short_in_one_job_writes_nothing_anywhere(batches, n):
    b = batches(n)
    which = list(range(n))
    arena = b.outputs(which)
    canvas, rows, want_dropped = b.expectation(which, arena)
    for short in _singled_out(n):
        assert rows[short] >= 2
        caps = list(b.lens)
        caps[short] = rows[short] - 1
        st, lens, dropped = b.call(which, arena, capacities=caps)
        assert st == _abi.A3D_INVALID_PARAMETER, short
        assert lens == rows and dropped == want_dropped, short
        _assert_words(arena.read(), arena.blank(), f"a voxel mean one short in cloud {short} of {n} wrote")
    st, lens, dropped = b.call(which, arena, capacities=rows)  # exactly enough is enough
    assert st == _abi.A3D_OK and lens == rows and dropped == want_dropped
    _assert_words(arena.read(), canvas, f"voxel mean of {n} with exact capacities")
    arena.free()


@pytest.mark.parametrize("n", BATCHES)
def test_alone_equals_in_the_batch_and_runs_are_identical(batches, n):
    b = batches(n)
    which = list(range(n))
    arena = b.outputs(which)
    runs = []
    for _ in range(2):
        arena.reset()
        st, lens, dropped = b.call(which, arena, ORIGIN)
        assert st == _abi.A3D_OK
        runs.append((arena.read(), lens, dropped))
    _assert_words(runs[1][0], runs[0][0], f"two voxel means of {n}")
    assert runs[1][1:] == runs[0][1:]
    for i in _singled_out(n):
        single = b.outputs([i])
        st, lens, dropped = b.call([i], single, ORIGIN)
        assert st == _abi.A3D_OK and (lens[0], dropped[0]) == (runs[0][1][i], runs[0][2][i])
        words = single.read()
        for plane in range(PLANES):
            _assert_words(single.segment(words, plane), arena.segment(runs[0][0], PLANES * i + plane),
                          f"voxel mean: cloud {i} of {n} alone, plane {plane}")
        # and against the restatement, once per cloud
        canvas, want_lens, want_dropped = b.expectation([i], single, ORIGIN)
        assert (lens, dropped) == (want_lens, want_dropped)
        _assert_words(words, canvas, f"voxel mean: cloud {i} alone")
        single.free()
    arena.free()


def test_cloud_of_more_chunks_than_tiles(ctx):
    # the smallest cloud whose tiles hold two chunks: 4096 * 1024 + 1 points are 4097 chunks of 1024, above the 4096 tiles a
    # cloud may have, so 2049 tiles of 2 chunks, the last of them with one point (the chunk loop and carried base of pass
    # 4, the span of 2048 of passes 1, 2, 5 and 6, the slot shares of pass 3 over 2049 tiles)
    points, _, colors = _uniform(150, 4096 * 1024 + 1, with_normals=False)
    t0 = time.perf_counter()
    expected = M.voxel_mean(points, None, colors, 0.02)
    print(f"[restatement] {time.perf_counter() - t0:.2f} s; {len(expected[3])} cells, counts up to {expected[4].max()}")
    assert len(expected[3]) > 2_000_000 and expected[4].max() > 4 and expected[5] == 0
    cloud = _device_cloud(ctx, points, None, colors)
    t0 = time.perf_counter()
    st, lens, dropped, outs = _call(ctx, [cloud], 0.02, None)
    print(f"[call, with its buffers and their read-back] {time.perf_counter() - t0:.2f} s")
    assert st == _abi.A3D_OK and outs[0]["normals"] is None
    assert all(outs[0][f] is not None for f in ("points", "colors", "index", "counts"))
    _assert_matches(outs[0], lens[0], dropped[0], expected)
    cloud.free()
