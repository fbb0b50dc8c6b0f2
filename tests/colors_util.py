"""What the colour tests share: input colours that identify their row, and device buffers with byte-granular guards.

Colours are a payload that follows a point, so the expected colour of an output row is colors_in[index], with `index`
from the mask or from the numpy restatement (voxel_restatement.py) and never from the code under test.  row_colors makes
every row's colour a function of (cloud, row) that differs between neighbours, clouds and channels: a wrong row, a
swapped channel or a stale winner shows."""
import ctypes as C

import numpy as np

CANARY_BYTE = 0xA5
GUARD_BYTES = 64  # a multiple of 4: a guarded body starts 4-byte aligned and ends wherever its length ends


def row_colors(cloud, n):
    """[n, 3] u8: for point i of cloud j, k = i * 2654435761 + j, r = k & 255, g = (k >> 8) & 255, b = (k >> 16) & 255."""
    k = np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(cloud)
    return np.stack([k & np.uint64(255), (k >> np.uint64(8)) & np.uint64(255), (k >> np.uint64(16)) & np.uint64(255)],
                    axis=1).astype(np.uint8).reshape(n, 3)


class Guarded:
    """A device buffer of `nbytes` bytes filled with CANARY_BYTE from end to end, with GUARD_BYTES more of it on both
    sides.  `ptr` is the body's address."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.total = 2 * GUARD_BYTES + self.nbytes
        self.base = ctx.to_device(np.full(self.total, CANARY_BYTE, np.uint8))
        self.ptr = C.c_void_p(self.base.value + GUARD_BYTES)
        assert self.ptr.value % 4 == 0

    def read(self):
        """(the body as uint8 [nbytes], True iff both guards are intact)."""
        raw = self.ctx.to_host(self.base, np.empty(self.total, np.uint8))
        body = raw[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        return body, bool((raw[:GUARD_BYTES] == CANARY_BYTE).all() and (raw[GUARD_BYTES + self.nbytes:] == CANARY_BYTE).all())

    def free(self):
        self.ctx.free(self.base)


def check_rows(buf, rows, expected, width, label=""):
    """Asserts that a Guarded buffer of elements of `width` bytes holds `expected` (any dtype, compared byte for byte) in
    its first `rows` elements, the canary in every byte after them, and intact guards; frees it."""
    body, intact = buf.read()
    buf.free()
    assert intact, f"{label}: a store outside the buffer"
    want = np.ascontiguousarray(expected).view(np.uint8).reshape(-1)
    assert want.size == rows * width, label
    assert np.array_equal(body[:rows * width], want), label
    assert (body[rows * width:] == CANARY_BYTE).all(), f"{label}: a store past row {rows}"


def untouched(buf, label=""):
    """Asserts that a Guarded buffer holds nothing but the canary; frees it."""
    check_rows(buf, 0, np.empty(0, np.uint8), 1, label)
