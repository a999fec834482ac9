"""unique_copy and unique on the GPU (hpxhip_unique_copy, the adjacent mode of
k_compact in compaction_kernel.hpp) against numpy with the device's meaning:
``keep = r_[True, ~rel(a[:-1], a[1:])]``, the result ``a[keep]``.  Every
buffer is compared whole and bitwise against what it held before the call
with the expected range written into it, so canary elements either side of a
range and, in place, the elements from the new end onward must keep their
values."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hpx_amd as hpx
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# Elements per tile: compaction_detail::tile_elems<T>() in
# include/hpxhip/kernels/compaction_kernel.hpp (kThreads = 1024 threads x
# kRounds = 8 vectors of 16 B per lane = 128 KiB).
T8 = 16384   # 8-byte elements
T4 = 32768   # 4-byte elements


def tile(dt):
    return T8 if np.dtype(dt).itemsize == 8 else T4


SIZES = {"0": lambda T: 0, "1": lambda T: 1, "2": lambda T: 2, "3": lambda T: 3, "63": lambda T: 63,
         "64": lambda T: 64, "65": lambda T: 65, "1023": lambda T: 1023, "1025": lambda T: 1025,
         "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1, "2T+1": lambda T: 2 * T + 1,
         "65T+3": lambda T: 65 * T + 3, "129T+5": lambda T: 129 * T + 5}
ALL_DT = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]


def size_of(label, dt):
    return SIZES[label](tile(dt))


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


def host_keep(a, rel=None):
    """Which elements survive, with the device's meaning: the first, and every
    element that the relation does not relate to its immediate predecessor."""
    if a.size == 0:
        return np.zeros(0, bool)
    if isinstance(rel, F.KeyCompareShifted):
        s = np.array(rel.bits, dtype=a.dtype)
        related = (a[:-1] >> s) == (a[1:] >> s)
    else:
        related = a[:-1] == a[1:]  # by value: NaN != NaN, -0.0 == +0.0
    return np.r_[True, ~related]


def canary(dt):
    return np.frombuffer(b"\x5a" * np.dtype(dt).itemsize, dtype=dt)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    assert got.size == want.size
    np.testing.assert_array_equal(bits(got), bits(want))


class Run:
    """One unique_copy (or, with in_place, unique) call through the Python
    mirror; the buffers are laid out as [off canaries | range | one canary]."""

    def __init__(self, pol, t, a, rel=None, it=0, ot=0, in_place=False):
        n, dt, c = a.size, a.dtype, canary(a.dtype)
        self.a, self.keep, self.in_place = a, host_keep(a, rel), in_place
        self.h_in = np.full(it + n + 1, c, dtype=dt)
        self.h_in[it:it + n] = a
        self.d_in = hpx.vector.from_host(self.h_in, t)
        self.first = self.d_in.begin() + it
        if in_place:
            self.d_out, self.h_out, self.ot, self.dest = self.d_in, self.h_in, it, self.first
            self.result = P.unique(pol, self.first, self.first + n, rel)
        else:
            self.h_out = np.full(ot + n + 1, c, dtype=dt)
            self.d_out = hpx.vector.from_host(self.h_out, t)
            self.ot, self.dest = ot, self.d_out.begin() + ot
            self.result = P.unique_copy(pol, self.first, self.first + n, self.dest, rel)

    def check(self, result=None):
        r = result if result is not None else self.result
        n, count = self.a.size, int(self.keep.sum())
        if self.in_place:
            assert r - self.first == count
        else:
            last, end = r
            assert last - self.first == n
            assert end - self.dest == count
            same(self.d_in.to_host(), self.h_in)
        want = self.h_out.copy()
        want[self.ot:self.ot + count] = self.a[self.keep]
        same(self.d_out.to_host(), want)
        return count


def both_ways(pol, t, a, rel=None, **kw):
    c1 = Run(pol, t, a, rel, **kw).check()
    c2 = Run(pol, t, a, rel, in_place=True, **{k: v for k, v in kw.items() if k != "ot"}).check()
    assert c1 == c2
    return c1


def distinct(n, dt):
    return np.arange(n).astype(dt)  # exact in float32 up to 2^24


def patterns(n, T, dt, seed):
    """name -> (array, expected count or None)."""
    rng = np.random.default_rng(seed)
    out = {"all equal": (np.full(n, 7, dtype=dt), min(n, 1)),
           "all distinct": (distinct(n, dt), n),
           "runs of 1-4": (np.repeat(np.arange(n), rng.integers(1, 5, n))[:n].astype(dt) if n else np.zeros(0, dt), None),
           "runs of about 3T": ((np.arange(n) // (3 * T - 5)).astype(dt), None)}
    return out


# ---------------------------------------------------------------- the sizes
@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("size", list(SIZES))
def test_unique_copy(pol, gpu_target, size, dt):
    n = size_of(size, dt)
    for name, (a, count) in patterns(n, tile(dt), dt, 100 + n % 97).items():
        got = Run(pol, gpu_target, a).check()
        if count is not None:
            assert got == count, name


@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("size", list(SIZES))
def test_in_place(pol, gpu_target, size, dt):
    """unique: the range sits 4 elements into its buffer (still 16-B aligned),
    so a canary lies either side; the elements from the new end to last keep
    their values."""
    n = size_of(size, dt)
    for name, (a, count) in patterns(n, tile(dt), dt, 200 + n % 89).items():
        got = Run(pol, gpu_target, a, it=4, in_place=True).check()
        if count is not None:
            assert got == count, name


# ----------------------------------------------------------- the neighbour
def boundary_positions(dt, base):
    """p such that the pair (p, p + 1) straddles each boundary of the tile's
    index order (wave, round, lane, element) in the tile that starts at base."""
    T, V = tile(dt), 16 // np.dtype(dt).itemsize
    ps = {"e -> e+1": 5 * V, "last e -> e+1": 5 * V + V - 2, "V-1 -> next lane": 5 * V + V - 1,
          "lane 63 -> round 1": 64 * V - 1, "lane 63 -> round 4": 4 * 64 * V - 1,
          "wave 0 -> 1": T // 16 - 1, "wave 7 -> 8": 8 * (T // 16) - 1, "tile": T - 1,
          "first pair": 0}
    return {k: base + p for k, p in ps.items()}


def pair_cases(dt):
    """(n, name, p): a pair (p, p + 1) inside [0, n)."""
    T = tile(dt)
    out = []
    n = 2 * T + 1
    for base in (0, T):
        out += [(n, f"{name} @{base // T}T", p) for name, p in boundary_positions(dt, base).items() if p + 1 < n]
    n = 65 * T + 3
    out += [(n, f"{name} @64T", p) for name, p in boundary_positions(dt, 64 * T).items()]
    out += [(n, "in the last tile", 65 * T), (n, "the last two elements", n - 2)]
    out += [(2, "n == 2", 0), (T + 1, "the last two of T+1", T - 1)]
    return out


@pytest.mark.parametrize("dt", ALL_DT)
def test_single_duplicate_pair_across_every_boundary(pol, gpu_target, dt):
    bases = {}
    for n, name, p in pair_cases(dt):
        a = bases.setdefault(n, distinct(n, dt)).copy()
        a[p + 1] = a[p]
        assert both_ways(pol, gpu_target, a) == n - 1, name


@pytest.mark.parametrize("dt", ALL_DT)
def test_single_change_across_every_boundary(pol, gpu_target, dt):
    for n, name, p in pair_cases(dt):
        a = np.full(n, 3, dtype=dt)
        a[p + 1:] = 4
        assert both_ways(pol, gpu_target, a) == 2, name


# ------------------------------------------------------------------- floats
def float_data(dt, n, seed):
    rng = np.random.default_rng(seed)
    a = np.repeat(rng.integers(-3, 4, n), rng.integers(1, 4, n))[:n].astype(dt)
    for v in (np.nan, -0.0, 0.0):
        at = np.flatnonzero(rng.random(n) < 0.1)
        a[at] = v
        a[np.minimum(at + 1, n - 1)] = v  # ... and pairs of them
    return a


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_float_meaning(pol, gpu_target, dt):
    """equal_to by value: every NaN is kept, -0.0 == +0.0 keeps the first."""
    a = np.array([np.nan, np.nan, 1.0, -0.0, 0.0, -0.0, 2.0, 0.0, -0.0, np.nan, 2.0, 2.0], dtype=dt)
    r = Run(pol, gpu_target, a)
    assert r.check() == 8
    got = r.d_out.to_host()[:8]
    same(got, a[[0, 1, 2, 3, 6, 7, 9, 10]])
    assert np.signbit(got[3]) and not np.signbit(got[5])
    n = 2 * tile(dt) + 1
    a = float_data(dt, n, 2)
    nan = np.isnan(a)
    assert (nan[:-1] & nan[1:]).any() and np.signbit(a[a == 0]).any() and (~np.signbit(a[a == 0])).any()
    r = Run(pol, gpu_target, a)
    count = r.check()
    assert np.isnan(r.d_out.to_host()[:count]).sum() == nan.sum()  # every NaN is kept
    Run(pol, gpu_target, a, it=4, in_place=True).check()


# ---------------------------------------------------------------- EQUAL_SHR
def shifted_data(dt, s, n, seed, negative=False):
    """Runs of equal x >> s whose low s bits vary within the run."""
    width = 8 * np.dtype(dt).itemsize
    rng = np.random.default_rng(seed)
    runs = np.cumsum(rng.random(n) < 0.4).astype(np.int64)
    if s == width - 1:
        b = runs % 2
        if np.dtype(dt).kind == "i":
            b = -b  # x >> (bits - 1) of a signed x is 0 or -1
    else:
        b = runs - (runs.max() + 5 if negative else 0)
    low = rng.integers(0, 1 << min(s, 16), n).astype(np.uint64) if s else np.zeros(n, np.uint64)
    u = (b.view(np.uint64) << np.uint64(s)) + low  # modulo 2^64
    if width == 32:
        u = u.astype(np.uint32)
    return u.view(dt)


@pytest.mark.parametrize("dt,negative", [(np.int32, False), (np.uint64, False), (np.int64, True)])
@pytest.mark.parametrize("shift", [0, 3, "bits-1"])
def test_equal_shifted(pol, gpu_target, dt, negative, shift):
    s = 8 * np.dtype(dt).itemsize - 1 if shift == "bits-1" else shift
    n = 2 * tile(dt) + 1
    a = shifted_data(dt, s, n, 30 + s, negative)
    rel = F.key_equal_shifted(s)
    keep = host_keep(a, rel)
    assert 1 < keep.sum() < n
    if negative:
        assert (a < 0).any()
    if s:
        # the low bits vary inside the runs, so keeping another element than the first shows
        assert (a[1:][~keep[1:]] != a[:-1][~keep[1:]]).any()
    both_ways(pol, gpu_target, a, rel)
    both_ways(pol, gpu_target, a, rel, it=1)


# --------------------------------------------------------------- sub-ranges
def runs_data(n, dt, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.random(n) < 0.5).astype(dt)


@pytest.mark.parametrize("dt", [np.int64, np.float32])
@pytest.mark.parametrize("ot", [0, 1, 3])
@pytest.mark.parametrize("it", [0, 1, 3])
def test_sub_ranges(pol, gpu_target, it, ot, dt):
    n = 2 * tile(dt) + 1
    Run(pol, gpu_target, runs_data(n, dt, 6), it=it, ot=ot).check()


@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("it", [1, 3])
def test_sub_range_in_place(pol, gpu_target, dt, it):
    n = 2 * tile(dt) + 1
    Run(pol, gpu_target, runs_data(n, dt, 7), it=it, in_place=True).check()


@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("n", [5, 1025])
def test_sub_range_element_wise_and_head(pol, gpu_target, n, dt):
    """n <= 4 * head takes the element-wise kernel, larger ones the split-off head."""
    a = runs_data(n, dt, 8)
    for it in (1, 3):
        both_ways(pol, gpu_target, a, it=it, ot=it)
        both_ways(pol, gpu_target, distinct(n, dt), it=it)
        both_ways(pol, gpu_target, np.full(n, 9, dtype=dt), it=it)


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("it", [1, 3])
def test_pair_across_the_head_and_the_vector_kernel(pol, gpu_target, dt, it):
    """The head kernel places the h elements in front of the first 16-B
    boundary; the vector kernel's element 0 compares with the head's last."""
    V = 16 // np.dtype(dt).itemsize
    h = -it % V
    assert h > 0
    n = 2 * tile(dt) + 1
    a = distinct(n, dt)
    a[h] = a[h - 1]
    assert both_ways(pol, gpu_target, a, it=it) == n - 1
    a = np.full(n, 3, dtype=dt)
    a[h:] = 4
    assert both_ways(pol, gpu_target, a, it=it) == 2
    # ... and no boundary effect where nothing changes or everything does
    assert both_ways(pol, gpu_target, np.full(n, 3, dtype=dt), it=it) == 1
    assert both_ways(pol, gpu_target, distinct(n, dt), it=it) == n


# ------------------------------------------------------------- 64-bit state
@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("size", ["2T+1", "65T+3"])
def test_state64(pol, gpu_target, monkeypatch, size, dt):
    """The 64-bit look-back state (used from 2^32 elements on) at small n."""
    n = size_of(size, dt)
    monkeypatch.setenv("HPXHIP_UNIQUE_STATE64", "1")
    a = runs_data(n, dt, 13)
    both_ways(pol, gpu_target, a)
    both_ways(pol, gpu_target, a, it=1)


# -------------------------------------------------- stream and policy use
def test_back_to_back_on_one_stream(gpu_target):
    """Calls queued on one stream with the cached scratch, a large one and then
    a small one: no stale tile state."""
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    a1, a2 = runs_data(70 * T8 + 9, np.int64, 15), runs_data(3 * T8 + 1, np.int64, 17)
    runs = [Run(pt, gpu_target, a1), Run(pt, gpu_target, a2), Run(pt, gpu_target, a1, it=4, in_place=True),
            Run(pt, gpu_target, a2, it=1, in_place=True)]
    for r in runs:
        assert isinstance(r.result, hpx.future)
        r.check(r.result.get())


def test_task_policy_returns_futures(gpu_target):
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    a = runs_data(100003, np.int32, 19)
    keep = host_keep(a)
    d, o = hpx.vector.from_host(a, gpu_target), hpx.vector(a.size, dtype=a.dtype, tgt=gpu_target)
    f = P.unique_copy(pt, d.begin(), d.end(), o.begin(), F.key_equal)
    assert isinstance(f, hpx.future)
    last, end = f.get()
    assert last - d.begin() == a.size and end - o.begin() == keep.sum()
    same(o.to_host()[:end - o.begin()], a[keep])
    f = P.unique(pt, d.begin(), d.end())
    assert isinstance(f, hpx.future)
    assert f.get() - d.begin() == keep.sum()
    same(d.to_host()[:keep.sum()], a[keep])


def test_sort_then_unique_then_is_sorted(pol, gpu_target):
    n = 1 << 20
    a = np.random.default_rng(21).integers(-1000, 1000, n).astype(np.int64)
    d = hpx.vector.from_host(a, gpu_target)
    P.sort(pol, d.begin(), d.end())
    end = P.unique(pol, d.begin(), d.end())
    want = np.unique(a)
    assert end - d.begin() == len(want)
    assert P.is_sorted(pol, d.begin(), end)
    same(d.to_host()[:len(want)], want)


# -------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("in_place", [False, True])
def test_caller_provided_scratch(gpu_target, in_place):
    """Exactly hpxhip_scratch_bytes bytes, a canary after them."""
    n = 65 * T8 + 3
    a = runs_data(n, np.int64, 22)
    keep = host_keep(a)
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_UNIQUE_COPY, L.I64, 0, n, ctypes.byref(need))
    assert need.value > 0 and need.value % 8 == 0
    words = need.value // 8
    h_scr = np.full(words + 32, canary(np.int64), dtype=np.int64)
    scratch = hpx.vector.from_host(h_scr, gpu_target)
    d = hpx.vector.from_host(a, gpu_target)
    o = d if in_place else hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    count = hpx.vector(1, dtype=np.uint64, tgt=gpu_target)
    vp = ctypes.c_void_p
    args = (L.I64, L.Q_EQUAL, None, vp(d.begin().address), vp(o.begin().address), n, vp(count.begin().address),
            gpu_target.stream, vp(scratch.begin().address))
    # a scratch that is one byte short is refused (before anything is queued)
    assert L.load().hpxhip_unique_copy(*args, need.value - 1) == L.ERROR_INVALID_ARGUMENT
    L.call("hpxhip_unique_copy", *args, need.value)
    L.call("hpxhip_stream_synchronize", gpu_target.stream)
    c = int(count.to_host()[0])
    assert c == keep.sum()
    same(o.to_host()[:c], a[keep])
    if in_place:
        same(o.to_host()[c:], a[c:])
    same(scratch.to_host()[words:], h_scr[words:])


def test_empty_range_writes_the_count_only(gpu_target):
    o = hpx.vector.from_host(np.full(4, 5, dtype=np.int64), gpu_target)
    count = hpx.vector.from_host(np.full(1, 77, dtype=np.uint64), gpu_target)
    vp = ctypes.c_void_p
    L.call("hpxhip_unique_copy", L.I64, L.Q_EQUAL, None, None, None, 0, vp(count.begin().address), gpu_target.stream,
           None, 0)
    L.call("hpxhip_stream_synchronize", gpu_target.stream)
    assert int(count.to_host()[0]) == 0
    same(o.to_host(), np.full(4, 5, dtype=np.int64))


def test_injected_error_is_exception_list(pol, gpu_target):
    a = runs_data(1000, np.int64, 24)
    d = hpx.vector.from_host(a, gpu_target)
    o = hpx.vector.from_host(np.zeros(a.size, dtype=a.dtype), gpu_target)
    calls = [lambda: P.unique_copy(pol, d.begin(), d.end(), o.begin()),
             lambda: P.unique(pol, d.begin(), d.end()),
             lambda: P.unique(pol, d.begin(), d.end(), F.key_equal_shifted(2))]
    for call in calls:
        L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
        with pytest.raises(L.exception_list) as ei:
            call()
        assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
        L.call("hpxhip_debug_inject_error", 0, 0)
        same(d.to_host(), a)  # nothing was enqueued
        same(o.to_host(), np.zeros(a.size, dtype=a.dtype))


# ---------------------------------------------------------- the C++ mirror
def test_cxx_unique_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "unique")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "unique: all tests passed" in r.stdout
