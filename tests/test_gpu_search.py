"""The search family on the GPU -- find / find_if / find_if_not, all_of /
any_of / none_of, count / count_if, min_element / max_element /
minmax_element, equal / mismatch (include/hpxhip/kernels/search_kernel.hpp,
hpx_amd/csrc/search.hip) -- against numpy.  Every input buffer is laid out as
[off canaries | range | one canary] and compared whole and bitwise with its
host mirror after the calls: no call may write to its input."""
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

# Elements per block chunk: reduce_detail::kThreads = 1024 threads x kSteps = 8
# vectors of 16 B (include/hpxhip/kernels/reduce_kernel.hpp).
T8 = 16384   # 8-byte elements
T4 = 32768   # 4-byte elements


def tile(dt):
    return T8 if np.dtype(dt).itemsize == 8 else T4


SIZES = {"0": lambda T: 0, "1": lambda T: 1, "2": lambda T: 2, "3": lambda T: 3, "63": lambda T: 63,
         "64": lambda T: 64, "65": lambda T: 65, "1023": lambda T: 1023, "1025": lambda T: 1025,
         "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1, "2T+1": lambda T: 2 * T + 1,
         "65T+3": lambda T: 65 * T + 3}
ALL_DT = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
CASES = [(s, dt) for dt in ALL_DT for s in SIZES] + [("129T+5", np.int64), ("129T+5", np.float32)]
OFFSETS = (0, 1, 3)  # elements past a 16-B boundary


def size_of(label, dt):
    T = tile(dt)
    return 129 * T + 5 if label == "129T+5" else SIZES[label](T)


def case_id(c):
    return f"{c[0]}-{np.dtype(c[1]).name}"


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


@pytest.fixture(scope="module")
def task(gpu_target):
    return ex.par(ex.task).on(hpx.default_executor(gpu_target))


def canary(dt):
    return np.frombuffer(b"\x5a" * np.dtype(dt).itemsize, dtype=dt)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Buf:
    """A range `off` elements past a 16-B boundary with a canary either side
    (hipMalloc'ed memory is 256-B aligned; off = 0 gets four canaries in
    front, which keeps the boundary)."""

    def __init__(self, pol, t, a, off=0):
        self.pol, self.n, dt = pol, a.size, a.dtype
        self.vw = 16 // dt.itemsize
        self.lead = off if off else self.vw
        self.h = np.full(self.lead + a.size + 1, canary(dt), dtype=dt)
        self.h[self.lead:self.lead + a.size] = a
        self.d = hpx.vector.from_host(self.h, t)
        self.first = self.d.begin() + self.lead
        self.last = self.first + a.size
        self.head = min((self.vw - off % self.vw) % self.vw, a.size)

    @property
    def a(self):
        return self.h[self.lead:self.lead + self.n]

    def plant(self, i, value):
        """a[i] = value on the host mirror and on the device."""
        self.a[i] = value
        P.copy(self.pol, self.a[i:i + 1].copy(), None, self.first + i)

    def positions(self):
        """0, the last head element, the first vector element, T-1, T, the
        first tail element, n-1 (those that exist)."""
        n, T = self.n, tile(self.h.dtype)
        tail0 = self.head + (n - self.head) // self.vw * self.vw
        want = [0, self.head - 1, self.head, T - 1, T, tail0, n - 1]
        return sorted({p for p in want if 0 <= p < n})

    def unchanged(self):
        np.testing.assert_array_equal(bits(self.d.to_host()), bits(self.h))


def first_true(mask):
    nz = np.flatnonzero(mask)
    return int(nz[0]) if nz.size else mask.size


def ascending(n, dt):
    return (np.arange(n) + 1).astype(dt)  # 1..n, exact in float32 up to 2^24


PRED_NP = {
    L.P_LT: lambda a, v: a < v, L.P_LE: lambda a, v: a <= v, L.P_GT: lambda a, v: a > v, L.P_GE: lambda a, v: a >= v,
    L.P_EQ: lambda a, v: a == v, L.P_NE: lambda a, v: a != v, L.P_NOT_LT: lambda a, v: ~(a < v),
    L.P_BITS: lambda a, v: (a & v) != 0,
}


def mask_of(a, pred):
    with np.errstate(invalid="ignore"):
        return PRED_NP[pred.kind](a, a.dtype.type(pred.arg))


def check_find_family(b, pred):
    """All six find-like algorithms and count_if for one predicate."""
    pol, m, n = b.pol, mask_of(b.a, pred), b.n
    assert P.find_if(pol, b.first, b.last, pred) - b.first == first_true(m)
    assert P.find_if_not(pol, b.first, b.last, pred) - b.first == first_true(~m)
    assert P.any_of(pol, b.first, b.last, pred) is bool(m.any())
    assert P.none_of(pol, b.first, b.last, pred) is (not m.any())
    assert P.all_of(pol, b.first, b.last, pred) is bool(m.all())
    c = P.count_if(pol, b.first, b.last, pred)
    assert isinstance(c, int) and c == int(m.sum())
    assert n == b.last - b.first


# ------------------------------------------------------------ find and count
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_find_and_count_sizes(pol, gpu_target, case):
    """The range holds 1..n, so find(p + 1) hits at p alone, greater_equal(p + 1)
    at p and everything after it (the first must win), and the counts are known."""
    n, dt = size_of(*case), case[1]
    for off in OFFSETS:
        b = Buf(pol, gpu_target, ascending(n, dt), off)
        for p in b.positions():
            assert P.find(pol, b.first, b.last, p + 1) - b.first == p
            assert P.find_if(pol, b.first, b.last, F.greater_equal(p + 1)) - b.first == p
            assert P.find_if_not(pol, b.first, b.last, F.less_than(p + 1)) - b.first == p
            assert P.count(pol, b.first, b.last, p + 1) == 1
            assert P.count_if(pol, b.first, b.last, F.greater_equal(p + 1)) == n - p
        # nowhere: last (first for an empty range)
        assert P.find(pol, b.first, b.last, 0) - b.first == n
        assert P.find_if(pol, b.first, b.last, F.less_than(1)) - b.first == n
        assert P.find_if_not(pol, b.first, b.last, F.greater_than(0)) - b.first == n
        # every element hits
        assert P.find_if(pol, b.first, b.last, F.greater_than(0)) - b.first == 0
        assert P.any_of(pol, b.first, b.last, F.greater_than(0)) is (n > 0)
        assert P.all_of(pol, b.first, b.last, F.greater_than(0)) is True
        assert P.none_of(pol, b.first, b.last, F.greater_than(0)) is (n == 0)
        assert P.any_of(pol, b.first, b.last, F.less_than(1)) is False
        assert P.all_of(pol, b.first, b.last, F.less_than(1)) is (n == 0)
        assert P.none_of(pol, b.first, b.last, F.less_than(1)) is True
        # 0 %, about 50 % and 100 %
        assert P.count_if(pol, b.first, b.last, F.less_than(1)) == 0
        assert P.count_if(pol, b.first, b.last, F.less_equal(n // 2)) == n // 2
        assert P.count_if(pol, b.first, b.last, F.greater_than(0)) == n
        b.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: np.dtype(d).name)
def test_every_predicate_kind(pol, gpu_target, dt):
    n = 3 * tile(dt) + 77
    rng = np.random.default_rng(5)
    a = rng.integers(0, 100, n).astype(dt)
    a[:2 * tile(dt) + 5] = 50  # the first element that differs sits in the third block
    b = Buf(pol, gpu_target, a, 1)
    preds = [F.less_than(50), F.less_equal(49), F.greater_than(50), F.greater_equal(51), F.equal_to(50),
             F.not_equal_to(50), F.not_less_than(51)]
    if np.issubdtype(dt, np.integer):
        preds += [F.any_bits(0x40), F.any_bits(1)]
    for pred in preds:
        check_find_family(b, pred)
    b.unchanged()


@pytest.mark.parametrize("dt", [np.int64, np.float32], ids=lambda d: np.dtype(d).name)
def test_several_hits_the_first_wins(pol, gpu_target, dt):
    """Two and three hits in different blocks, waves and lanes and inside one
    16-B vector."""
    T, vw = tile(dt), 16 // np.dtype(dt).itemsize
    n = 5 * T + 11
    wave = 64 * vw  # elements one wave loads per step
    groups = [(3 * T + 5, T + 9), (4 * T + 1, 2 * T + 3, 2 * T + 2), (T + 70 * vw, T + 3 * vw),
              (2 * wave + 5, wave + 7, 9 * wave), (8 * vw + 1, 8 * vw), (4 * vw + vw - 1, 4 * vw + vw - 2, n - 1),
              (n - 1, n - 2), (1024 * vw * 3 + 5, 1024 * vw * 7 + 5)]
    b = Buf(pol, gpu_target, np.zeros(n, dtype=dt), 0)
    for g in groups:
        for p in g:
            b.plant(p, 1)
        assert P.find(pol, b.first, b.last, 1) - b.first == min(g), g
        assert P.find_if_not(pol, b.first, b.last, F.equal_to(0)) - b.first == min(g), g
        assert P.count(pol, b.first, b.last, 1) == len(g)
        assert P.any_of(pol, b.first, b.last, F.equal_to(1)) is True
        for p in g:
            b.plant(p, 0)
    assert P.none_of(pol, b.first, b.last, F.equal_to(1)) is True
    b.unchanged()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_and_signed_zero_in_find_and_count(pol, gpu_target, dt):
    n = 2 * tile(dt) + 9
    a = np.full(n, 1.0, dtype=dt)
    p, q = tile(dt) + 3, tile(dt) + 900
    a[p], a[q], a[5], a[n - 1] = np.nan, np.nan, -0.0, 0.0
    b = Buf(pol, gpu_target, a, 3)
    # a NaN fails less_than, so find_if_not(less_than) finds it
    assert P.find_if_not(pol, b.first, b.last, F.less_than(2.0)) - b.first == p
    assert P.all_of(pol, b.first, b.last, F.less_than(2.0)) is False
    assert P.find(pol, b.first, b.last, float("nan")) - b.first == n
    assert P.count(pol, b.first, b.last, float("nan")) == 0
    assert P.count_if(pol, b.first, b.last, F.not_equal_to(float("nan"))) == n
    assert P.count(pol, b.first, b.last, 0.0) == 2
    assert P.count(pol, b.first, b.last, -0.0) == 2
    assert P.find(pol, b.first, b.last, 0.0) - b.first == 5
    b.unchanged()


# ------------------------------------------------------------- the extremes
def host_extremes(a, comp):
    """(min_element, max_element, minmax_element) indices under comp for a
    NaN-free array: first smallest, first largest, (first smallest, last
    largest), "smallest" being the largest value under greater."""
    if a.size == 0:
        return 0, 0, (0, 0)
    lo_first, hi_first = int(np.argmin(a)), int(np.argmax(a))
    lo_last, hi_last = a.size - 1 - int(np.argmin(a[::-1])), a.size - 1 - int(np.argmax(a[::-1]))
    if comp.descending:
        return hi_first, lo_first, (hi_first, lo_last)
    return lo_first, hi_first, (lo_first, hi_last)


def check_extremes(b, comps=(F.less, F.greater)):
    pol = b.pol
    for comp in comps:
        lo, hi, (mlo, mhi) = host_extremes(b.a, comp)
        assert P.min_element(pol, b.first, b.last, comp) - b.first == lo, comp.name
        assert P.max_element(pol, b.first, b.last, comp) - b.first == hi, comp.name
        r = P.minmax_element(pol, b.first, b.last, comp)
        assert (r[0] - b.first, r[1] - b.first) == (mlo, mhi), comp.name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_extremes_sizes(pol, gpu_target, case):
    """Distinct values 11.. with the extreme planted at each position: 0 as the
    smallest, n + 100 as the largest."""
    n, dt = size_of(*case), case[1]
    for off in OFFSETS:
        b = Buf(pol, gpu_target, (np.arange(n) + 11).astype(dt), off)
        assert P.min_element(pol, b.first, b.last) - b.first == 0
        assert P.max_element(pol, b.first, b.last) - b.first == max(n - 1, 0)
        comps = (F.less, F.greater) if off == 0 else ((F.less,) if off == 1 else (F.greater,))
        for p in b.positions():
            keep = b.a[p].copy()
            for v in (0, n + 100):
                b.plant(p, v)
                check_extremes(b, comps)
            b.plant(p, keep)
        b.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: np.dtype(d).name)
def test_extremes_ties(pol, gpu_target, dt):
    T, vw = tile(dt), 16 // np.dtype(dt).itemsize
    n = 5 * T + 11
    # a constant range: the first and, for minmax's largest, the last index
    b = Buf(pol, gpu_target, np.full(n, 7, dtype=dt), 1)
    for comp in (F.less, F.greater):
        assert P.min_element(pol, b.first, b.last, comp) - b.first == 0
        assert P.max_element(pol, b.first, b.last, comp) - b.first == 0
        r = P.minmax_element(pol, b.first, b.last, comp)
        assert (r[0] - b.first, r[1] - b.first) == (0, n - 1)
    b.unchanged()
    # the extreme repeated in several blocks, waves and lanes and in one vector
    a = np.random.default_rng(9).integers(10, 1000, n).astype(dt)
    lows = [3 * T + 5, T + 9, T + 9 + 64 * vw, T + 10, 4 * T + 1, n - 1]
    highs = [2 * T + 2, 2 * T + 3, 70 * vw, 3 * vw + 1, 4 * T + 7, 1024 * vw * 3 + 5]
    a[lows], a[highs] = 0, 5000
    b = Buf(pol, gpu_target, a, 3)
    assert P.min_element(pol, b.first, b.last) - b.first == min(lows)
    assert P.max_element(pol, b.first, b.last) - b.first == min(highs)
    r = P.minmax_element(pol, b.first, b.last)
    assert (r[0] - b.first, r[1] - b.first) == (min(lows), max(highs))
    assert P.min_element(pol, b.first, b.last, F.greater) - b.first == min(highs)
    assert P.max_element(pol, b.first, b.last, F.greater) - b.first == min(lows)
    r = P.minmax_element(pol, b.first, b.last, F.greater)
    assert (r[0] - b.first, r[1] - b.first) == (min(highs), max(lows))
    check_extremes(b)
    b.unchanged()


@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: np.dtype(d).name)
def test_extremes_of_the_type(pol, gpu_target, dt):
    """The signed and unsigned extremes of each integer type; +-inf."""
    n = 2 * tile(dt) + 5
    a = np.random.default_rng(11).integers(0, 1000, n).astype(dt)
    if np.issubdtype(dt, np.integer):
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    else:
        lo, hi = -np.inf, np.inf
    a[tile(dt) + 17], a[n - 2], a[3], a[tile(dt) - 1] = lo, lo, hi, hi
    if np.issubdtype(dt, np.signedinteger):
        a[40:50] = -1  # would be the largest if compared unsigned
    b = Buf(pol, gpu_target, a, 0)
    check_extremes(b)
    assert P.max_element(pol, b.first, b.last) - b.first == 3
    r = P.minmax_element(pol, b.first, b.last)
    assert r[1] - b.first == tile(dt) - 1
    if lo != 0:  # an unsigned type's smallest value also occurs in the random fill
        assert P.min_element(pol, b.first, b.last) - b.first == tile(dt) + 17
        assert r[0] - b.first == tile(dt) + 17
    b.unchanged()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_signed_zeros_tie(pol, gpu_target, dt):
    b = Buf(pol, gpu_target, np.array([0.0, -0.0], dtype=dt), 0)
    assert P.min_element(pol, b.first, b.last) - b.first == 0
    assert P.max_element(pol, b.first, b.last) - b.first == 0
    r = P.minmax_element(pol, b.first, b.last)
    assert (r[0] - b.first, r[1] - b.first) == (0, 1)
    b.unchanged()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_extremes_with_nans_are_valid_and_reproducible(pol, gpu_target, dt):
    n = 3 * tile(dt) + 7
    a = np.random.default_rng(13).random(n).astype(dt)
    a[np.random.default_rng(14).integers(0, n, 200)] = np.nan
    a[0] = np.nan
    b = Buf(pol, gpu_target, a, 1)
    for comp in (F.less, F.greater):
        for fn in (P.min_element, P.max_element):
            i1, i2 = fn(pol, b.first, b.last, comp) - b.first, fn(pol, b.first, b.last, comp) - b.first
            assert 0 <= i1 < n and i1 == i2
        r1, r2 = P.minmax_element(pol, b.first, b.last, comp), P.minmax_element(pol, b.first, b.last, comp)
        i1 = (r1[0] - b.first, r1[1] - b.first)
        assert all(0 <= i < n for i in i1) and i1 == (r2[0] - b.first, r2[1] - b.first)
    b.unchanged()


# ------------------------------------------------------- equal and mismatch
def check_pair(pol, b1, b2, want):
    n = b1.n
    r = P.mismatch(pol, b1.first, b1.last, b2.first)
    assert (r[0] - b1.first, r[1] - b2.first) == (want, want)
    assert P.equal(pol, b1.first, b1.last, b2.first) is (want == n)
    r = P.mismatch(pol, b1.first, b1.last, b2.first, b2.last)
    assert (r[0] - b1.first, r[1] - b2.first) == (want, want)
    assert P.equal(pol, b1.first, b1.last, b2.first, b2.last) is (want == n)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_equal_and_mismatch_sizes(pol, gpu_target, case):
    """Identical ranges, then one differing element at each position; the two
    ranges at the same offset (16-B loads) and at different ones (element
    loads)."""
    n, dt = size_of(*case), case[1]
    a = ascending(n, dt)
    for off1, off2 in ((0, 0), (1, 1), (3, 3), (0, 1), (3, 0)):
        b1, b2 = Buf(pol, gpu_target, a, off1), Buf(pol, gpu_target, a, off2)
        check_pair(pol, b1, b2, n)
        for p in sorted(set(b1.positions()) | set(b2.positions())):
            b2.plant(p, 0)
            check_pair(pol, b1, b2, p)
            if p + 1 < n:  # a second difference behind the first
                b2.plant(n - 1, 0)
                check_pair(pol, b1, b2, p)
                b2.plant(n - 1, a[n - 1])
            b2.plant(p, a[p])
        b1.unchanged()
        b2.unchanged()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_differs_from_itself(pol, gpu_target, dt):
    n = 2 * tile(dt) + 3
    a = np.ones(n, dtype=dt)
    a[7], a[tile(dt) + 5] = -0.0, np.nan
    b1 = Buf(pol, gpu_target, a, 0)
    z = a.copy()
    z[7] = 0.0  # -0.0 == +0.0 by value
    b2 = Buf(pol, gpu_target, z, 0)
    check_pair(pol, b1, b2, tile(dt) + 5)
    check_pair(pol, b1, b1, tile(dt) + 5)  # the range against itself
    b1.unchanged()
    b2.unchanged()


def test_four_iterators_with_different_lengths(pol, gpu_target):
    n = T8 + 100
    a = ascending(n, np.int64)
    b1, b2 = Buf(pol, gpu_target, a, 0), Buf(pol, gpu_target, a, 1)
    short = b2.first + (n - 40)
    assert P.equal(pol, b1.first, b1.last, b2.first, short) is False
    r = P.mismatch(pol, b1.first, b1.last, b2.first, short)
    assert (r[0] - b1.first, r[1] - b2.first) == (n - 40, n - 40)
    r = P.mismatch(pol, b1.first, b1.first + 10, b2.first, b2.last)
    assert (r[0] - b1.first, r[1] - b2.first) == (10, 10)
    b2.plant(5, 0)
    r = P.mismatch(pol, b1.first, b1.last, b2.first, short)
    assert (r[0] - b1.first, r[1] - b2.first) == (5, 5)
    assert P.equal(pol, b1.first, b1.first, b2.first, b2.first) is True
    assert P.equal(pol, b1.first, b1.first, b2.first, b2.first + 1) is False
    b1.unchanged()
    b2.unchanged()


# -------------------------------------------------- stream and policy use
def test_task_policy_returns_futures(pol, task, gpu_target):
    """One case of each algorithm: the future's get() is the synchronous result."""
    n = 3 * T8 + 5
    a = np.random.default_rng(17).integers(0, 1000, n).astype(np.int64)
    z = a.copy()
    z[2 * T8 + 1] = -1
    b, b2 = Buf(pol, gpu_target, a, 1), Buf(pol, gpu_target, z, 1)
    pred = F.greater_than(997)
    calls = [
        (lambda p: P.find(p, b.first, b.last, int(a[n - 3])), lambda r: r - b.first),
        (lambda p: P.find_if(p, b.first, b.last, pred), lambda r: r - b.first),
        (lambda p: P.find_if_not(p, b.first, b.last, F.less_than(999)), lambda r: r - b.first),
        (lambda p: P.all_of(p, b.first, b.last, F.less_than(1000)), lambda r: r),
        (lambda p: P.any_of(p, b.first, b.last, pred), lambda r: r),
        (lambda p: P.none_of(p, b.first, b.last, pred), lambda r: r),
        (lambda p: P.count(p, b.first, b.last, int(a[0])), lambda r: r),
        (lambda p: P.count_if(p, b.first, b.last, pred), lambda r: r),
        (lambda p: P.min_element(p, b.first, b.last), lambda r: r - b.first),
        (lambda p: P.max_element(p, b.first, b.last, F.greater), lambda r: r - b.first),
        (lambda p: P.minmax_element(p, b.first, b.last), lambda r: (r[0] - b.first, r[1] - b.first)),
        (lambda p: P.equal(p, b.first, b.last, b2.first), lambda r: r),
        (lambda p: P.equal(p, b.first, b.last, b2.first, b2.last - 1), lambda r: r),
        (lambda p: P.mismatch(p, b.first, b.last, b2.first), lambda r: (r[0] - b.first, r[1] - b2.first)),
    ]
    futures = [(call(task), call, key) for call, key in calls]  # all queued before the first get
    got = []
    for f, call, key in futures:
        assert isinstance(f, hpx.future)
        got.append(key(f.get()))
        assert got[-1] == key(call(pol))
    assert got[-1] == (2 * T8 + 1, 2 * T8 + 1) and got[-2] is False and got[-3] is False
    assert got[0] <= n - 3 and got[8] == int(np.argmin(a))
    b.unchanged()
    b2.unchanged()


def test_injected_error_is_exception_list(pol, gpu_target):
    b = Buf(pol, gpu_target, ascending(1000, np.int64), 0)
    calls = [lambda: P.find(pol, b.first, b.last, 5), lambda: P.count(pol, b.first, b.last, 5),
             lambda: P.min_element(pol, b.first, b.last), lambda: P.equal(pol, b.first, b.last, b.first),
             lambda: P.all_of(pol, b.first, b.last, F.less_than(5))]
    for call in calls:
        L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
        with pytest.raises(L.exception_list) as ei:
            call()
        assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
        L.call("hpxhip_debug_inject_error", 0, 0)
    b.unchanged()


# -------------------------------------------------------------- the C ABI
def test_caller_provided_scratch(gpu_target):
    """Exactly hpxhip_scratch_bytes bytes, a canary after them."""
    n = 65 * T8 + 3
    a = np.random.default_rng(19).integers(-1000, 1000, n).astype(np.int64)
    d = hpx.vector.from_host(a, gpu_target)
    out = hpx.vector.from_host(np.full(3, 77, dtype=np.uint64), gpu_target)
    vp = ctypes.c_void_p
    zero = L.scalar_buf(L.I64, 0)
    for algo, name, args, want in (
            (L.ALGO_COUNT_IF, "hpxhip_count_if", (L.I64, L.P_LT, zero, vp(d.begin().address), n), [int((a < 0).sum())]),
            (L.ALGO_MINMAX_ELEMENT, "hpxhip_minmax_element", (L.I64, L.X_MINMAX, 0, vp(d.begin().address), n),
             list(host_extremes(a, F.less)[2]))):
        need = ctypes.c_size_t()
        L.call("hpxhip_scratch_bytes", algo, L.I64, 0, n, ctypes.byref(need))
        assert need.value > 0 and need.value % 8 == 0
        words = need.value // 8
        h_scr = np.full(words + 32, canary(np.int64), dtype=np.int64)
        scratch = hpx.vector.from_host(h_scr, gpu_target)
        full = args + (vp(out.begin().address), gpu_target.stream, vp(scratch.begin().address))
        # a scratch that is one byte short is refused (before anything is queued)
        assert getattr(L.load(), name)(*full, need.value - 1) == L.ERROR_INVALID_ARGUMENT
        L.call(name, *full, need.value)
        L.call("hpxhip_stream_synchronize", gpu_target.stream)
        got = out.to_host()
        assert [int(x) for x in got[:len(want)]] == want
        assert int(got[2]) == 77
        np.testing.assert_array_equal(scratch.to_host()[words:], h_scr[words:])
    np.testing.assert_array_equal(d.to_host(), a)


def test_empty_range_writes_the_result_only(gpu_target):
    out = hpx.vector.from_host(np.full(4, 77, dtype=np.uint64), gpu_target)
    vp = ctypes.c_void_p
    o = out.begin().address
    s = gpu_target.stream
    L.call("hpxhip_find_if", L.I64, L.P_EQ, None, 0, None, 0, vp(o), s)
    L.call("hpxhip_stream_synchronize", s)
    assert [int(x) for x in out.to_host()] == [0, 77, 77, 77]
    L.call("hpxhip_mismatch", L.F32, None, None, 0, vp(o + 8), s)
    L.call("hpxhip_count_if", L.U32, L.P_BITS, None, None, 0, vp(o + 16), s, None, 0)
    L.call("hpxhip_stream_synchronize", s)
    assert [int(x) for x in out.to_host()] == [0, 0, 0, 77]
    out2 = hpx.vector.from_host(np.full(4, 77, dtype=np.uint64), gpu_target)
    o2 = out2.begin().address
    L.call("hpxhip_minmax_element", L.F64, L.X_MAX, 1, None, 0, vp(o2), s, None, 0)
    L.call("hpxhip_minmax_element", L.F64, L.X_MINMAX, 0, None, 0, vp(o2 + 16), s, None, 0)
    L.call("hpxhip_stream_synchronize", s)
    assert [int(x) for x in out2.to_host()] == [0, 77, 0, 0]


# ---------------------------------------------------------- the C++ mirror
def test_cxx_search_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "search")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "search: all tests passed" in r.stdout
