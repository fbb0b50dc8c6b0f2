"""One table of refusals, three calls: a3d_point_clouds_select_device, a3d_point_clouds_voxel_downsample_rgb_device and
a3d_point_clouds_voxel_mean_device share their host front (csrc/cloud_batch.hpp: compact_front), so for every malformed
batch of the table they give the same status, leave their result arrays alone and name themselves in a3d_last_error.
No device: the addresses are made up and every row is refused on the host before any HIP call."""
import ctypes as C

import pytest

from align3d_amd import _abi

SENTINEL = 0x7777
SELECT, DOWNSAMPLE, MEAN = "select", "downsample", "mean"
CALLS = (SELECT, DOWNSAMPLE, MEAN)
SYMBOL = {SELECT: "a3d_point_clouds_select_device", DOWNSAMPLE: "a3d_point_clouds_voxel_downsample_rgb_device",
          MEAN: "a3d_point_clouds_voxel_mean_device"}
# (the rgb downsample and the plain one are one call, the plain one forwards: both report under the plain one's name)
REPORTED = {SELECT: b"a3d_point_clouds_select_device", DOWNSAMPLE: b"a3d_point_clouds_voxel_downsample_device",
            MEAN: b"a3d_point_clouds_voxel_mean_device"}
INPUTS = ("points", "normals", "colors")
OUTPUTS = ("out_points", "out_normals", "out_colors", "out_index")


@pytest.fixture(scope="module")
def lib():
    return _abi.load_library()


class _Args:
    """Three clouds of 4 points at made-up, disjoint device addresses, 0x1000 apart per cloud: clouds 0 and 2 with normals
    and colours and every output, cloud 1 with points only; a made-up context; sentinel-filled result arrays."""

    def __init__(self):
        self.views = (_abi.PointCloudViewC * 3)()
        for i in range(3):
            self.views[i].points, self.views[i].len = 0x10000 + 0x1000 * i, 4
            self.views[i].normals = None if i == 1 else 0x20000 + 0x1000 * i
        self.ctx = C.c_void_p(0x900000)

        def per_cloud(base, cloud_1=True):
            return (C.c_void_p * 3)(*[base + 0x1000 * i if i != 1 or cloud_1 else None for i in range(3)])

        self.colors = per_cloud(0x30000, False)
        self.out_points, self.out_index = per_cloud(0x40000), per_cloud(0x70000)
        self.out_normals, self.out_colors = per_cloud(0x50000, False), per_cloud(0x60000, False)
        self.capacities = (C.c_uint64 * 3)(4, 4, 4)
        self.lens = (C.c_uint64 * 3)(*[SENTINEL] * 3)
        self.dropped = (C.c_uint64 * 3)(*[SENTINEL] * 3)
        self._results = (self.lens, self.dropped)  # (a row may pass NULL for one of them: the arrays are looked at all the same)
        self.n = 3
        # what only one of the calls takes
        self.values, self.lo, self.hi = per_cloud(0x80000), (C.c_uint32 * 3)(1, 1, 1), (C.c_uint32 * 3)(5, 5, 5)
        self.out_counts = per_cloud(0x90000)
        self.voxel, self.origin = 0.05, (C.c_float * 3)(0.0, 0.0, 0.0)

    def field(self, name):
        """The per-cloud array `name`: for points and normals, a stand-in that reads and writes the views."""
        if name not in ("points", "normals"):
            return getattr(self, name)
        views = self.views

        class _ViewField:
            def __getitem__(self, i):
                return getattr(views[i], name)

            def __setitem__(self, i, value):
                setattr(views[i], name, value)

        return _ViewField()

    def call(self, lib, which):
        f = getattr(lib, SYMBOL[which])
        if which == SELECT:
            return f(self.ctx, self.views, self.colors, self.n, self.values, self.lo, self.hi, self.out_points,
                     self.out_normals, self.out_colors, self.out_index, self.capacities, self.lens)
        if which == DOWNSAMPLE:
            return f(self.ctx, self.views, self.colors, self.n, self.voxel, self.origin, self.out_points, self.out_normals,
                     self.out_colors, self.out_index, self.capacities, self.lens, self.dropped)
        return f(self.ctx, self.views, self.colors, self.n, self.voxel, self.origin, self.out_points, self.out_normals,
                 self.out_colors, self.out_index, self.out_counts, self.capacities, self.lens, self.dropped)

    def untouched(self):
        return all(list(r) == [SENTINEL] * 3 for r in self._results)


def _null_argument(name):
    return lambda a: setattr(a, name, None)


def _entry(name, i, value):
    def change(a):
        a.field(name)[i] = value
    return change


def _length(i, value):
    def change(a):
        a.views[i].len = value
    return change


def _all_of(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


def _empty_between(change):
    """Cloud 1 empty with every pointer null, and `change` on the clouds around it."""
    nulls = [_entry(name, 1, None) for name in INPUTS + OUTPUTS + ("values", "out_counts")]
    return _all_of(_length(1, 0), *nulls, change)


def _address(a, name, i):
    return a.field(name)[i]


def _output_on(output, target, cloud):
    """Output `output` of cloud 0 at the address of array `target` of cloud `cloud`."""
    def change(a):
        a.field(output)[0] = _address(a, target, cloud)
    return change


INVALID, MISSING = _abi.A3D_INVALID_PARAMETER, _abi.A3D_MISSING_FIELD
TABLE = [(f"null {name}", _null_argument(name), INVALID) for name in ("ctx", "views", "out_points", "capacities", "lens")]
TABLE += [
    ("2^32 points in second place", _length(1, 1 << 32), INVALID),
    ("more than 2^32 points in second place", _length(1, (1 << 32) + 5), INVALID),
    ("within one tile of 2^32 points", _length(2, (1 << 32) - 1), INVALID),
    ("2^32 points ahead of a null pointer", _all_of(_length(1, 1 << 32), _entry("points", 2, None)), INVALID),
    ("null points", _entry("points", 0, None), INVALID),
    ("null points of the last cloud", _entry("points", 2, None), INVALID),
    ("null output", _entry("out_points", 1, None), INVALID),
    ("null points ahead of a missing field", _all_of(_entry("points", 0, None), _entry("out_normals", 1, 0xA0000)), INVALID),
    ("normals output without normals", _entry("out_normals", 1, 0xA0000), MISSING),
    ("normals output, the cloud's normals null", _entry("normals", 2, None), MISSING),
    ("colours output without colours", _entry("out_colors", 1, 0xA0000), MISSING),
    ("colours output, no colours array at all", _null_argument("colors"), MISSING),
    ("a missing field ahead of an overlap", _all_of(_entry("out_normals", 1, 0xA0000), _output_on("out_points", "points", 2)),
     MISSING),
    ("an empty cloud between two good ones, then an overlap", _empty_between(_output_on("out_index", "points", 2)), INVALID),
    ("one byte shared", _entry("out_colors", 0, 0x10000 + 47), INVALID),
    ("the output's last byte on the next cloud's input", _entry("out_index", 0, 0x22000 - 15), INVALID),
]
for _output in OUTPUTS:
    for _cloud in (0, 2):
        TABLE += [(f"{_output} of cloud 0 on {_input} of cloud {_cloud}", _output_on(_output, _input, _cloud), INVALID)
                  for _input in INPUTS]
        TABLE += [(f"{_output} of cloud 0 on {_other} of cloud {_cloud}", _output_on(_output, _other, _cloud), INVALID)
                  for _other in OUTPUTS if (_other, _cloud) != (_output, 0)]


@pytest.mark.parametrize("what,change,status", TABLE, ids=[row[0] for row in TABLE])
def test_the_three_calls_refuse_alike(lib, what, change, status):
    for which in CALLS:
        a = _Args()
        change(a)
        assert a.call(lib, which) == status, which
        assert a.untouched(), which
        assert REPORTED[which] in lib.a3d_last_error(), (which, lib.a3d_last_error())


def test_the_text_says_which_refusal_fired_first(lib):
    """The order of the checks, seen from outside: of two faults in one batch the earlier check's text is reported."""
    rows = [
        (_all_of(_null_argument("lens"), _length(0, 1 << 32)), b"null argument"),
        (_all_of(_length(1, 1 << 32), _entry("points", 0, None)), b"null points"),  # cloud 0 is looked at first
        (_all_of(_length(1, 1 << 32), _entry("points", 2, None)), b"2^32 points or more"),
        (_all_of(_entry("points", 0, None), _entry("out_normals", 1, 0xA0000)), b"null points"),
        (_all_of(_entry("out_normals", 1, 0xA0000), _entry("out_colors", 1, 0xA8000)), b"no normals"),
        (_all_of(_entry("out_colors", 1, 0xA8000), _length(1, (1 << 32) - 1)), b"no colours"),
        (_all_of(_length(0, (1 << 32) - 1), _output_on("out_points", "points", 2)), b"within one tile"),
        (_empty_between(_output_on("out_index", "points", 2)), b"overlaps"),
    ]
    for change, text in rows:
        for which in CALLS:
            a = _Args()
            change(a)
            assert a.call(lib, which) != _abi.A3D_OK and a.untouched()
            assert text in lib.a3d_last_error() and REPORTED[which] in lib.a3d_last_error(), (which, lib.a3d_last_error())


def test_arguments_of_one_call_only(lib):
    """What the table cannot share: select's values and bounds, the grid of the two downsamples, the counts of the mean."""
    for name in ("values", "lo", "hi"):
        a = _Args()
        setattr(a, name, None)
        assert a.call(lib, SELECT) == INVALID and a.untouched() and REPORTED[SELECT] in lib.a3d_last_error()
    a = _Args()
    a.values[2] = None
    assert a.call(lib, SELECT) == INVALID and a.untouched() and b"null points, values or output" in lib.a3d_last_error()
    for output in OUTPUTS:
        a = _Args()
        a.field(output)[0] = 0x82000 + 12  # the values' last word
        assert a.call(lib, SELECT) == INVALID and a.untouched() and b"overlaps" in lib.a3d_last_error()
    for which in (DOWNSAMPLE, MEAN):
        for voxel in (0.0, -0.05, float("nan"), float("inf")):
            a = _Args()
            a.voxel = voxel
            a.views[1].len = 1 << 32  # the scalar parameters come before the clouds
            assert a.call(lib, which) == INVALID and a.untouched()
            assert b"voxel size" in lib.a3d_last_error() and REPORTED[which] in lib.a3d_last_error()
        a = _Args()
        a.origin[1] = float("inf")
        assert a.call(lib, which) == INVALID and a.untouched()
        assert b"origin" in lib.a3d_last_error() and REPORTED[which] in lib.a3d_last_error()
    for target, cloud in [(name, c) for name in INPUTS + OUTPUTS for c in (0, 2)]:
        a = _Args()
        a.out_counts[0] = _address(a, target, cloud)
        assert a.call(lib, MEAN) == INVALID and a.untouched() and b"overlaps" in lib.a3d_last_error(), (target, cloud)


def test_a_capacity_below_the_length_still_covers_its_elements(lib):
    """An output counts for its first min(len, capacity) elements.  (That an array may lie right behind them, and that
    inputs may overlap inputs, is shown by tests/cpp/cloud_batch_host_test.cpp: a batch that is not refused goes on to the
    device.)"""
    for which in CALLS:
        a = _Args()
        a.capacities[0] = 2
        a.out_normals[0] = 0x40000 + 23  # on the last byte of the two points cloud 0 may write
        assert a.call(lib, which) == INVALID and b"overlaps" in lib.a3d_last_error() and a.untouched()


def test_a_batch_of_empty_clouds_is_ok_and_zeroes_the_results(lib):
    for which in CALLS:
        a = _Args()
        for i in range(3):
            _empty_between(lambda _: None)(a)
            a.views[i].len = 0
        assert a.call(lib, which) == _abi.A3D_OK
        assert list(a.lens) == [0, 0, 0]
        assert list(a.dropped) == ([SENTINEL] * 3 if which == SELECT else [0, 0, 0])
