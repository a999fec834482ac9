"""reverse, reverse_copy, rotate, rotate_copy, swap_ranges, replace(_if),
replace_copy(_if) and adjacent_difference on the GPU (hpx_amd/csrc/permute.hip,
include/hpxhip/kernels/permute_kernel.hpp) against the NumPy reference of
tests/permute_reference.py (pinned to the std loops by
tests/test_permute_host.py).  Every range sits between canaries, every buffer
is compared whole and bitwise, inputs must be unchanged."""
import os
import subprocess

import numpy as np
import pytest

import hpx_amd as hpx
import permute_reference as PR
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ALL_DT = PR.ALL_DT
TWO_DT = [np.float32, np.int64]  # one 4-byte, one 8-byte type for the offset cross products


def dt_id(dt):
    return np.dtype(dt).name


def geometry(dt):
    """(V, B, S) of a dtype.  V: elements of a 16-B vector.  B: elements per
    block, permute_detail::kThreads = 64 threads with one vector each
    (include/hpxhip/kernels/permute_kernel.hpp:39).  S: the smallest length
    that takes the shifted-load path when the written range starts on a 1-KiB
    boundary: make_span_shifted needs a head of at least V elements, so takes
    a whole 1 KiB, and then n >= head + 4 KiB (hpx_amd/csrc/elementwise.hip:
    212-213)."""
    es = np.dtype(dt).itemsize
    v = 16 // es
    return v, 64 * v, 5 * 1024 // es


def sizes(dt):
    v, b, s = geometry(dt)
    k = 1024 // np.dtype(dt).itemsize
    return sorted({0, 1, 2, 3, v - 1, v, v + 1, 2 * v - 1, 2 * v + 1, b - 1, b, b + 1, 2 * b - 1, 2 * b + 1,
                   s - 1, s, s + 1, k - 1, k + 1, 65534, 65537})


def offset_sizes(dt):
    """The sizes of the offset cross products: one per path and boundary."""
    v, b, s = geometry(dt)
    return sorted({1, v + 1, 2 * v - 1, 2 * v, b + 1, 2 * b - 1, 2 * b + 2, s - 1, s, s + 1, 2 * s + 3})


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


def canary(dt):
    return np.frombuffer(b"\x5a" * np.dtype(dt).itemsize, dtype=dt)[0]


def same(got, want):
    assert got.size == want.size and got.dtype == want.dtype
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


class Side:
    """A range on the device as [off canaries | range | one canary]."""

    def __init__(self, t, a, off=0):
        self.off, self.n = off, a.size
        self.host = np.full(off + a.size + 1, canary(a.dtype), dtype=a.dtype)
        self.host[off:off + a.size] = a
        self.dev = hpx.vector.from_host(self.host, t)
        self.first = self.dev.begin() + off
        self.last = self.first + a.size

    def unchanged(self):
        same(self.dev.to_host(), self.host)

    def holds(self, body):
        """The device buffer is `body` between the untouched canaries."""
        want = self.host.copy()
        want[self.off:self.off + self.n] = body
        same(self.dev.to_host(), want)


def blank(t, dt, n, off=0):
    return Side(t, np.full(n, canary(dt), dtype=dt), off)


# ----------------------------------------------------------------- reverse
def check_reverse(pol, t, a, off):
    s = Side(t, a, off)
    assert P.reverse(pol, s.first, s.last) == s.last
    s.holds(PR.reverse(a))
    if a.size % 2:  # the middle element of an odd range keeps its place
        assert s.dev.to_host()[off + a.size // 2].tobytes() == a[a.size // 2].tobytes()


def check_reverse_copy(pol, t, a, off_in, off_out):
    s, o = Side(t, a, off_in), blank(t, a.dtype, a.size, off_out)
    assert P.reverse_copy(pol, s.first, s.last, o.first) == (s.last, o.first + a.size)
    o.holds(PR.reverse(a))
    s.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_reverse_sizes(pol, gpu_target, dt):
    for n in sizes(dt):
        a = PR.sample(dt, n, 1)
        check_reverse(pol, gpu_target, a, 0)
        check_reverse_copy(pol, gpu_target, a, 0, 0)


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_reverse_in_place_offsets_and_parities(pol, gpu_target, dt):
    """offset x length parity: all four (first + last) % 16 classes of a
    4-byte type, both of an 8-byte type."""
    v = geometry(dt)[0]
    classes = set()
    for n in offset_sizes(dt) + [x + 1 for x in offset_sizes(dt)]:
        a = PR.sample(dt, n, 2)
        for off in range(v + 1):
            check_reverse(pol, gpu_target, a, off)
            classes.add(((2 * off + n) * a.itemsize) % 16)
    assert len(classes) == v


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_reverse_copy_offsets(pol, gpu_target, dt):
    v = geometry(dt)[0]
    for n in offset_sizes(dt):
        a = PR.sample(dt, n, 3)
        for oi in range(v + 1):
            for oo in range(v + 1):
                check_reverse_copy(pol, gpu_target, a, oi, oo)


# ------------------------------------------------------------------ rotate
def mids(dt, n):
    v, b, _ = geometry(dt)
    m = {0, 1, v - 1, v, n // 2, n - v, n - 1, n, b + b // 2 + 1}  # the last: a seam inside a block
    return sorted(x for x in m if 0 <= x <= n)


def check_rotate(pol, t, a, mid, off, off_out):
    s = Side(t, a, off)
    assert P.rotate(pol, s.first, s.first + mid, s.last) == (s.first + (a.size - mid), s.last)
    s.holds(PR.rotate(a, mid))
    s, o = Side(t, a, off), blank(t, a.dtype, a.size, off_out)
    assert P.rotate_copy(pol, s.first, s.first + mid, s.last, o.first) == (s.last, o.first + a.size)
    o.holds(PR.rotate(a, mid))
    s.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_rotate_sizes_and_mids(pol, gpu_target, dt):
    v, b, s = geometry(dt)
    for n in (0, 1, 2, 3, v + 1, 2 * v - 1, b + 1, 2 * b - 1, s + 1, 2 * s + 3, 65537):
        a = PR.sample(dt, n, 4)
        for mid in mids(dt, n):
            check_rotate(pol, gpu_target, a, mid, 0, 0)


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_rotate_offsets(pol, gpu_target, dt):
    v, b, s = geometry(dt)
    for n in (2 * v + 1, 2 * b + 2, 2 * s + 3):
        a = PR.sample(dt, n, 5)
        for mid in (1, v - 1, n // 2, n - v, s + 1):
            if not 0 < mid < n:
                continue
            for off in range(v + 1):
                for oo in range(v + 1):
                    check_rotate(pol, gpu_target, a, mid, off, oo)


# ------------------------------------------------------------- swap_ranges
def check_swap(pol, t, a, b, oa, ob):
    sa, sb = Side(t, a, oa), Side(t, b, ob)
    assert P.swap_ranges(pol, sa.first, sa.last, sb.first) == sb.first + a.size
    sa.holds(b)
    sb.holds(a)


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_swap_ranges_sizes(pol, gpu_target, dt):
    for n in sizes(dt):
        check_swap(pol, gpu_target, PR.sample(dt, n, 6), PR.sample(dt, n, 7), 0, 0)


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_swap_ranges_offsets(pol, gpu_target, dt):
    v = geometry(dt)[0]
    for n in offset_sizes(dt):
        a, b = PR.sample(dt, n, 8), PR.sample(dt, n, 9)
        for oa in range(v + 1):
            for ob in range(v + 1):
                check_swap(pol, gpu_target, a, b, oa, ob)


# ----------------------------------------------------------------- replace
PREDS = [F.less_than, F.less_equal, F.greater_than, F.greater_equal, F.equal_to, F.not_equal_to, F.not_less_than,
         F.any_bits]


def check_replace(pol, t, a, pred, new, off_in=0, off_out=0):
    want = PR.replace_if(a, pred.kind, pred.arg, new)
    s = Side(t, a, off_in)
    assert P.replace_if(pol, s.first, s.last, pred, new) == s.last
    s.holds(want)
    s, o = Side(t, a, off_in), blank(t, a.dtype, a.size, off_out)
    assert P.replace_copy_if(pol, s.first, s.last, o.first, pred, new) == (s.last, o.first + a.size)
    o.holds(want)
    s.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_replace_every_predicate(pol, gpu_target, dt):
    v, b, s = geometry(dt)
    for n in (0, 1, v + 1, 2 * b - 1, s + 1):
        a = PR.sample(dt, n, 10)
        for make in PREDS:
            if make is F.any_bits and np.dtype(dt).kind == "f":
                continue
            check_replace(pol, gpu_target, a, make(1), 9)


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_replace_sizes_by_value(pol, gpu_target, dt):
    t = gpu_target
    for n in sizes(dt):
        a = PR.sample(dt, n, 11)
        s = Side(t, a)
        assert P.replace(pol, s.first, s.last, 1, 7) == s.last
        s.holds(PR.replace(a, 1, 7))
        s, o = Side(t, a), blank(t, dt, n)
        assert P.replace_copy(pol, s.first, s.last, o.first, 1, 7) == (s.last, o.first + n)
        o.holds(PR.replace(a, 1, 7))
        s.unchanged()


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_replace_offsets(pol, gpu_target, dt):
    v = geometry(dt)[0]
    for n in offset_sizes(dt):
        a = PR.sample(dt, n, 12)
        for oi in range(v + 1):
            for oo in range(v + 1):
                check_replace(pol, gpu_target, a, F.less_than(1), 9, oi, oo)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=dt_id)
def test_replace_signed_zero_and_nan(pol, gpu_target, dt):
    t = gpu_target
    nan = dt("nan")
    a = np.tile(np.array([0.0, -0.0, 1.5, nan, -0.0, 2.0, -nan], dtype=dt), 1000)
    for old, new in ((0.0, 7.0), (-0.0, 7.0), (nan, 7.0), (1.5, nan), (2.0, -0.0)):
        s = Side(t, a, 1)
        P.replace(pol, s.first, s.last, old, new)
        want = PR.replace(a, old, new)
        s.holds(want)
        o = blank(t, dt, a.size, 3)
        s = Side(t, a, 1)
        P.replace_copy(pol, s.first, s.last, o.first, old, new)
        o.holds(want)
    assert PR.same(PR.replace(a, nan, 7.0), a)  # what the NaN-old case compared against
    assert PR.replace(a, 0.0, 7.0)[1] == 7.0    # ... and -0.0 was replaced by value


# ------------------------------------------------------ adjacent_difference
def check_adjacent(pol, t, a, op=None, off_in=0, off_out=0):
    s, o = Side(t, a, off_in), blank(t, a.dtype, a.size, off_out)
    r = P.adjacent_difference(pol, s.first, s.last, o.first, *([] if op is None else [op]))
    assert r == o.first + a.size
    o.holds(PR.adjacent_difference(a, L.B_SUB if op is None else op.kind))
    s.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_adjacent_difference_sizes(pol, gpu_target, dt):
    for n in sizes(dt):
        a = PR.sample(dt, n, 13)
        check_adjacent(pol, gpu_target, a)
    a = PR.sample(dt, geometry(dt)[2] + 1, 14)
    check_adjacent(pol, gpu_target, a, F.Binary(L.B_MAX))
    check_adjacent(pol, gpu_target, a, F.subtract())


@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_adjacent_difference_offsets(pol, gpu_target, dt):
    v = geometry(dt)[0]
    for n in offset_sizes(dt):
        a = PR.sample(dt, n, 15)
        for oi in range(v + 1):
            for oo in range(v + 1):
                check_adjacent(pol, gpu_target, a, None, oi, oo)


@pytest.mark.parametrize("dt", [np.int32, np.uint32, np.int64, np.uint64], ids=dt_id)
def test_adjacent_difference_inverts_inclusive_scan(pol, gpu_target, dt):
    t = gpu_target
    a = PR.sample(dt, 65537, 16)  # the extremes make the sums wrap
    s, mid, o = Side(t, a, 1), blank(t, dt, a.size, 2), blank(t, dt, a.size, 3)
    P.inclusive_scan(pol, s.first, s.last, mid.first)
    P.adjacent_difference(pol, mid.first, mid.last, o.first)
    o.holds(a)


# -------------------------------------------- device identities at 2^22 + 1
@pytest.mark.parametrize("dt", [np.int64, np.float32], ids=dt_id)
def test_device_identities(pol, gpu_target, dt):
    """No host copy of the data: everything is compared with `equal`."""
    t = gpu_target
    n = (1 << 22) + 1
    mid = (1 << 21) + 12345
    x = hpx.vector(n + 1, dtype=dt, tgt=t)
    P.generate(pol, x.begin(), x.end(), "range" if np.dtype(dt).kind != "f" else "unit", 7, 0, 1 << 40)
    ref, w, y = (hpx.vector(n + 1, dtype=dt, tgt=t) for _ in range(3))
    P.copy(pol, x.begin(), x.end(), ref.begin())
    for off in (0, 1):
        f, l = x.begin() + off, x.begin() + off + n - off
        m = l - f

        def is_ref():
            return P.equal(pol, x.begin(), x.end(), ref.begin())

        # reverse o reverse = id, and it is not the identity in between
        P.reverse(pol, f, l)
        assert not is_ref()
        # reverse equals reverse_copy
        P.reverse_copy(pol, ref.begin() + off, ref.begin() + off + m, w.begin())
        assert P.equal(pol, f, l, w.begin())
        P.reverse(pol, f, l)
        assert is_ref()
        # rotate(mid) equals rotate_copy(mid); then rotate(n - mid) = id
        P.rotate(pol, f, f + mid, l)
        P.rotate_copy(pol, ref.begin() + off, ref.begin() + off + mid, ref.begin() + off + m, w.begin() + 1)
        assert P.equal(pol, f, l, w.begin() + 1)
        assert not is_ref()
        P.rotate(pol, f, f + (m - mid), l)
        assert is_ref()
        # swap_ranges twice = id
        P.copy(pol, w.begin(), w.end(), y.begin())
        P.swap_ranges(pol, f, l, w.begin() + 1 - off)
        assert P.equal(pol, f, l, y.begin() + 1 - off)
        assert P.equal(pol, w.begin() + 1 - off, w.begin() + 1 - off + m, ref.begin() + off)
        P.swap_ranges(pol, f, l, w.begin() + 1 - off)
        assert is_ref()
        assert P.equal(pol, w.begin(), w.end(), y.begin())


# ------------------------------------------------------------------ plumbing
def test_task_policy_returns_futures(gpu_target):
    t = gpu_target
    pt = ex.par(ex.task).on(hpx.default_executor(t))
    a, b = PR.sample(np.int64, 5003, 20), PR.sample(np.int64, 5003, 21)
    mid = 1234

    def fut(r):
        assert isinstance(r, hpx.future)
        return r.get()

    s = Side(t, a, 1)
    assert fut(P.reverse(pt, s.first, s.last)) == s.last
    s.holds(PR.reverse(a))
    s, o = Side(t, a, 1), blank(t, np.int64, a.size)
    assert fut(P.reverse_copy(pt, s.first, s.last, o.first)) == (s.last, o.first + a.size)
    o.holds(PR.reverse(a))
    assert fut(P.rotate(pt, s.first, s.first + mid, s.last)) == (s.first + (a.size - mid), s.last)
    s.holds(PR.rotate(a, mid))
    s, o = Side(t, a, 1), blank(t, np.int64, a.size)
    assert fut(P.rotate_copy(pt, s.first, s.first + mid, s.last, o.first)) == (s.last, o.first + a.size)
    o.holds(PR.rotate(a, mid))
    sb = Side(t, b, 2)
    assert fut(P.swap_ranges(pt, s.first, s.last, sb.first)) == sb.first + a.size
    s.holds(b)
    sb.holds(a)
    s = Side(t, a, 1)
    assert fut(P.replace(pt, s.first, s.last, 1, 7)) == s.last
    assert fut(P.replace_if(pt, s.first, s.last, F.less_than(0), 7)) == s.last
    want = PR.replace_if(PR.replace(a, 1, 7), L.P_LT, 0, 7)
    s.holds(want)
    o = blank(t, np.int64, a.size)
    assert fut(P.replace_copy(pt, s.first, s.last, o.first, 7, 8)) == (s.last, o.first + a.size)
    o.holds(PR.replace(want, 7, 8))
    assert fut(P.replace_copy_if(pt, s.first, s.last, o.first, F.greater_than(3), 0)) == (s.last, o.first + a.size)
    o.holds(PR.replace_if(want, L.P_GT, 3, 0))
    assert fut(P.adjacent_difference(pt, s.first, s.last, o.first)) == o.first + a.size
    o.holds(PR.adjacent_difference(want))


def test_back_to_back_on_one_stream(gpu_target):
    """Dependent calls queued on one stream without a wait in between."""
    t = gpu_target
    pt = ex.par(ex.task).on(hpx.default_executor(t))
    a = PR.sample(np.float32, 70001, 22)
    s, o, o2 = Side(t, a, 3), blank(t, np.float32, a.size, 1), blank(t, np.float32, a.size, 2)
    fs = [P.reverse(pt, s.first, s.last),
          P.rotate(pt, s.first, s.first + 777, s.last),
          P.replace(pt, s.first, s.last, 0.25, 9.0),
          P.reverse_copy(pt, s.first, s.last, o.first),
          P.adjacent_difference(pt, o.first, o.last, o2.first),
          P.swap_ranges(pt, s.first, s.last, o.first)]
    for f in fs:
        assert isinstance(f, hpx.future)
        f.get()
    step = PR.replace(PR.rotate(PR.reverse(a), 777), 0.25, 9.0)
    s.holds(PR.reverse(step))
    o.holds(step)
    o2.holds(PR.adjacent_difference(PR.reverse(step)))


def test_injected_error_is_exception_list(pol, gpu_target):
    t = gpu_target
    a = PR.sample(np.int64, 1000, 23)
    s, o = Side(t, a), blank(t, np.int64, a.size)
    calls = [lambda: P.reverse(pol, s.first, s.last),
             lambda: P.reverse_copy(pol, s.first, s.last, o.first),
             lambda: P.rotate(pol, s.first, s.first + 10, s.last),
             lambda: P.rotate_copy(pol, s.first, s.first + 10, s.last, o.first),
             lambda: P.swap_ranges(pol, s.first, s.last, o.first),
             lambda: P.replace(pol, s.first, s.last, 1, 2),
             lambda: P.replace_if(pol, s.first, s.last, F.less_than(1), 2),
             lambda: P.replace_copy(pol, s.first, s.last, o.first, 1, 2),
             lambda: P.replace_copy_if(pol, s.first, s.last, o.first, F.less_than(1), 2),
             lambda: P.adjacent_difference(pol, s.first, s.last, o.first)]
    for call in calls:
        L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
        with pytest.raises(L.exception_list) as ei:
            call()
        assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
        L.call("hpxhip_debug_inject_error", 0, 0)
        s.unchanged()  # nothing was enqueued
        o.unchanged()
    # the refusals of the C ABI surface the same way
    with pytest.raises(L.exception_list):
        P.reverse_copy(pol, s.first, s.last, s.first + 1)
    with pytest.raises(L.exception_list):
        P.adjacent_difference(pol, s.first, s.last, s.first)
    s.unchanged()


# ---------------------------------------------------------- the C++ mirror
def test_cxx_permute_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "permute")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "permute: all tests passed" in r.stdout
