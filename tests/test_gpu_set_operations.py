"""set_union, set_intersection, set_difference, set_symmetric_difference and
includes on the GPU (hpxhip_set_operation, include/hpxhip/kernels/
set_kernel.hpp) against the host reference of tests/set_reference.py (pinned
to the std loops by tests/test_set_operations_host.py).  Every buffer is
compared whole and bitwise: the output must be the expected elements between
untouched canaries, the inputs (canaries included) unchanged, and the returned
iterator dest + the expected count."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hpx_amd as hpx
import set_reference as SR
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# Elements of the MERGED order per tile, for every dtype: merge_detail::kTile
# = kThreads * kItems = 256 * 8 (include/hpxhip/kernels/merge_kernel.hpp:23),
# which set_kernel.hpp takes over (`using merge_detail::kTile`).
T = 2048

ALL_DT = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
TWO_DT = [np.int64, np.float32]
NAMES = ["set_union", "set_intersection", "set_difference", "set_symmetric_difference"]


def dt_id(dt):
    return np.dtype(dt).name


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


def canary(dt):
    return np.frombuffer(b"\x5a" * np.dtype(dt).itemsize, dtype=dt)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    assert got.size == want.size
    np.testing.assert_array_equal(bits(got), bits(want))


def comp_of(desc):
    return F.greater if desc else F.less


def keys(values, dt, desc):
    """Integers -> dt (signed and float types get negatives too), sorted in
    the device's order."""
    v = np.asarray(values, dtype=np.int64)
    if np.dtype(dt).kind != "u":
        v = v - 5
    return SR.sort_keys(v.astype(dt), desc)


class Side:
    """A range on the device as [off canaries | range | one canary]."""

    def __init__(self, t, a, off):
        self.host = np.full(off + a.size + 1, canary(a.dtype), dtype=a.dtype)
        self.host[off:off + a.size] = a
        self.dev = hpx.vector.from_host(self.host, t)
        self.first = self.dev.begin() + off
        self.last = self.first + a.size

    def unchanged(self):
        same(self.dev.to_host(), self.host)


def check_all(pol, t, a, b, desc, i1=0, i2=0, ot=0, names=NAMES, with_includes=True):
    """Every operation in `names` (and includes both ways) on one pair of
    ranges; -> {name: count}."""
    comp = comp_of(desc)
    A, B = Side(t, a, i1), Side(t, b, i2)
    get = (lambda r: r.get()) if pol.is_task else (lambda r: r)
    counts = {}
    for name in names:
        want = SR.set_operation(SR.OPS[name], a, b, desc)
        h_out = np.full(ot + a.size + b.size + 1, canary(a.dtype), dtype=a.dtype)
        d_out = hpx.vector.from_host(h_out, t)
        dest = d_out.begin() + ot
        r = getattr(P, name)(pol, A.first, A.last, B.first, B.last, dest, comp)
        assert isinstance(r, hpx.future) == pol.is_task
        end = get(r)
        assert end - dest == want.size, name
        h_out[ot:ot + want.size] = want
        same(d_out.to_host(), h_out)
        counts[name] = want.size
    if with_includes:
        assert get(P.includes(pol, A.first, A.last, B.first, B.last, comp)) == SR.includes(a, b, desc)
        assert get(P.includes(pol, B.first, B.last, A.first, A.last, comp)) == SR.includes(b, a, desc)
    A.unchanged()
    B.unchanged()
    return counts


# ---------------------------------------------------------------- the sizes
SIZES = [0, 1, 2, 63, 65, T - 1, T, T + 1, 2 * T + 1, 33 * T + 3]
PAIRS = ([(k, k) for k in SIZES] + [(0, k) for k in SIZES[1:]] + [(k, 0) for k in SIZES[1:]] +
         [(1, 33 * T + 3), (33 * T + 3, 1), (63, T + 1), (T - 1, 65), (T + 1, T - 1), (2, 2 * T + 1), (2 * T + 1, T)])


@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", ALL_DT, ids=dt_id)
def test_sizes(pol, gpu_target, dt, desc):
    rng = np.random.default_rng(40 + ALL_DT.index(dt))
    for n1, n2 in PAIRS:
        span = max(2, (n1 + n2) // 3)  # about a third of the keys are in both ranges, runs of 1-4
        a, b = keys(rng.integers(0, span, n1), dt, desc), keys(rng.integers(0, span, n2), dt, desc)
        check_all(pol, gpu_target, a, b, desc)


# -------------------------------------------------------------- the patterns
def patterns(rng):
    n = 3 * T + 5
    rep = lambda m: np.repeat(np.arange(m), rng.integers(1, 5, m))  # noqa: E731
    return {
        "disjoint interleaved": (2 * np.arange(n), 2 * np.arange(n - 9) + 1),
        "identical": (np.arange(n), np.arange(n)),
        "A below B": (np.arange(n), n + np.arange(2 * T + 1)),
        "B below A": (n + np.arange(n), np.arange(2 * T + 1)),
        "one value, more in A": (np.full(3 * T + 1, 7), np.full(2 * T - 7, 7)),
        "one value, more in B": (np.full(2 * T - 7, 7), np.full(3 * T + 1, 7)),
        "runs of 1-4": (rep(n // 2), rep(n // 2 + 11)),
        "runs of about 3T/2": (np.arange(4 * T + 3) // (3 * T // 2 - 5), np.arange(5 * T + 1) // (3 * T // 2 + 9)),
        "small alphabet": (rng.integers(0, 9, n), rng.integers(0, 7, 2 * T + 3)),
    }


@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", TWO_DT, ids=dt_id)
def test_patterns(pol, gpu_target, dt, desc):
    for name, (va, vb) in patterns(np.random.default_rng(50)).items():
        a, b = keys(va, dt, desc), keys(vb, dt, desc)
        c = check_all(pol, gpu_target, a, b, desc)
        assert c["set_union"] + c["set_intersection"] == a.size + b.size, name
        if name == "disjoint interleaved":
            assert c == {"set_union": a.size + b.size, "set_intersection": 0, "set_difference": a.size,
                         "set_symmetric_difference": a.size + b.size}
        if name == "one value, more in A":
            assert c == {"set_union": 3 * T + 1, "set_intersection": 2 * T - 7, "set_difference": T + 8,
                         "set_symmetric_difference": T + 8}


# ------------------------------------------------------------ every boundary
@pytest.mark.parametrize("dt", [np.int64, np.uint32], ids=dt_id)
def test_single_match_across_every_boundary(pol, gpu_target, dt):
    """A distinct, B one key equal to A[p]: the pair (A[p], B[0]) sits at the
    merged positions p, p + 1, which sweep over both tile boundaries."""
    a = keys(3 * np.arange(3 * T), dt, False)
    for p in list(range(T - 2, T + 3)) + list(range(2 * T - 2, 2 * T + 3)):
        c = check_all(pol, gpu_target, a, a[p:p + 1].copy(), False)
        assert c == {"set_union": a.size, "set_intersection": 1, "set_difference": a.size - 1,
                     "set_symmetric_difference": a.size - 1}
        # ... and a key of B between two of A's
        c = check_all(pol, gpu_target, a, a[p:p + 1] + np.array(1, dtype=dt), False, names=["set_symmetric_difference"])
        assert c == {"set_symmetric_difference": a.size + 1}


@pytest.mark.parametrize("dt", [np.int64, np.uint32], ids=dt_id)
@pytest.mark.parametrize("ca,cb", [(5, 3), (3, 5)])
def test_run_across_every_boundary(pol, gpu_target, dt, ca, cb):
    """A run of ca equal keys in A and cb in B, eight merged positions, moved
    over a tile boundary one step at a time: the boundary falls at every
    offset inside A's part, at the A-before-B split and inside B's part."""
    for q in range(T - 9, T + 2):
        va = np.r_[np.arange(q), np.full(ca, q), q + 1 + np.arange(T)]
        vb = np.full(cb, q)
        c = check_all(pol, gpu_target, keys(3 * va, dt, False), keys(3 * vb, dt, False), False)
        assert c["set_intersection"] == min(ca, cb) and c["set_symmetric_difference"] == va.size - ca + abs(ca - cb)
        # B with neighbours of its own, so that its part of the tile is not the run alone
        vb = np.r_[3 * np.arange(0, q, 7) + 1, np.full(cb, 3 * q), 3 * (q + 1 + np.arange(0, T, 5)) + 1]
        check_all(pol, gpu_target, keys(3 * va, dt, False), keys(vb, dt, False), False)


# ------------------------------------------------------------- float meaning
@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=dt_id)
def test_float_meaning(pol, gpu_target, dt, desc):
    u = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    qnan = {4: 0x7fc00000, 8: 0x7ff8000000000000}[np.dtype(dt).itemsize]
    sign = 1 << (8 * np.dtype(dt).itemsize - 1)
    nans = np.array([qnan, qnan | 5, qnan | sign, qnan | sign | 5], dtype=u).view(dt)
    zn, zp = np.array([-0.0], dtype=dt), np.array([0.0], dtype=dt)
    # -0.0 and +0.0 are different keys
    c = check_all(pol, gpu_target, zn, zp, desc)
    assert c == {"set_union": 2, "set_intersection": 0, "set_difference": 1, "set_symmetric_difference": 2}
    # NaNs with the same bits are one key, other payloads and signs other keys
    c = check_all(pol, gpu_target, SR.sort_keys(nans[[0, 0, 2]], desc), SR.sort_keys(nans[[0, 1, 2, 3]], desc), desc)
    assert c == {"set_union": 5, "set_intersection": 2, "set_difference": 1, "set_symmetric_difference": 3}
    # a tile and a half of everything: NaNs of both signs sort to both ends
    rng = np.random.default_rng(60)
    pool = np.concatenate([nans, zn, zp, np.array([-np.inf, np.inf, -1.5, 1.5, 3.0], dtype=dt)])
    a, b = SR.sort_keys(rng.choice(pool, T + 77), desc), SR.sort_keys(rng.choice(pool, 2 * T + 5), desc)
    ends = np.isnan(a[[0, -1]])
    assert ends.all() and np.signbit(a[0]) != np.signbit(a[-1])
    check_all(pol, gpu_target, a, b, desc)
    mixed = np.concatenate([np.arange(-T, T).astype(dt) / 4, pool])
    check_all(pol, gpu_target, SR.sort_keys(rng.choice(mixed, 3 * T + 1), desc),
              SR.sort_keys(rng.choice(mixed, 2 * T + 9), desc), desc)


# ---------------------------------------------------------------- sub-ranges
@pytest.mark.parametrize("dt", [np.int64, np.int32], ids=dt_id)
@pytest.mark.parametrize("i1", [0, 1, 3])
def test_sub_ranges(pol, gpu_target, dt, i1):
    """Offsets on in1, in2 and out: the element-load path and the store head."""
    rng = np.random.default_rng(70 + i1)
    a, b = keys(rng.integers(0, 2 * T, 2 * T + 3), dt, False), keys(rng.integers(0, 2 * T, T + 5), dt, False)
    for i2 in (0, 1, 3):
        for ot in (0, 1, 3):
            check_all(pol, gpu_target, a, b, False, i1=i1, i2=i2, ot=ot, with_includes=(ot == 0))


# ---------------------------------------------------------------- identities
def test_identities_on_the_device(pol, gpu_target):
    """2^22 + 2^22 sorted random u64, no host reference."""
    t, n = gpu_target, 1 << 22
    rng = np.random.default_rng(80)
    A = hpx.vector.from_host(rng.integers(0, 3 * n, n, dtype=np.uint64), t)
    B = hpx.vector.from_host(rng.integers(0, 3 * n, n, dtype=np.uint64), t)
    P.sort(pol, A.begin(), A.end())
    P.sort(pol, B.begin(), B.end())

    def fresh():
        return hpx.vector.from_host(np.full(2 * n, 0x5a5a5a5a5a5a5a5a, dtype=np.uint64), t)

    def op(name, x, xe, y, ye):
        o = fresh()
        return o, getattr(P, name)(pol, x, xe, y, ye, o.begin())

    U, ue = op("set_union", A.begin(), A.end(), B.begin(), B.end())
    I, ie = op("set_intersection", A.begin(), A.end(), B.begin(), B.end())
    DAB, dabe = op("set_difference", A.begin(), A.end(), B.begin(), B.end())
    DBA, dbae = op("set_difference", B.begin(), B.end(), A.begin(), A.end())
    S, se = op("set_symmetric_difference", A.begin(), A.end(), B.begin(), B.end())
    nu, ni, nab, nba, ns = (e - v.begin() for v, e in ((U, ue), (I, ie), (DAB, dabe), (DBA, dbae), (S, se)))
    assert nu + ni == 2 * n
    assert 0 < ni < n and nab == n - ni and nba == n - ni and ns == nab + nba
    for v, e in ((U, ue), (I, ie), (DAB, dabe), (DBA, dbae), (S, se)):
        assert P.is_sorted(pol, v.begin(), e)
    M1, M2 = fresh(), fresh()
    P.merge(pol, A.begin(), A.end(), DBA.begin(), dbae, M1.begin())
    same(M1.to_host(), U.to_host())  # whole buffers, the canaries behind the result included
    P.merge(pol, DAB.begin(), dabe, DBA.begin(), dbae, M2.begin())
    same(M2.to_host(), S.to_host())
    assert P.includes(pol, U.begin(), ue, A.begin(), A.end())
    assert P.includes(pol, U.begin(), ue, B.begin(), B.end())
    assert P.includes(pol, A.begin(), A.end(), I.begin(), ie)
    assert P.includes(pol, B.begin(), B.end(), I.begin(), ie)
    assert nba > 0 and not P.includes(pol, A.begin(), A.end(), B.begin(), B.end())


# ------------------------------------------------------------------ includes
@pytest.mark.parametrize("dt", [np.int64, np.uint32], ids=dt_id)
def test_includes(pol, gpu_target, dt):
    t = gpu_target

    def inc(a, b, desc=False):
        A, B = Side(t, a, 0), Side(t, b, 1)
        r = P.includes(pol, A.first, A.last, B.first, B.last, comp_of(desc))
        assert r == SR.includes(a, b, desc)
        A.unchanged()
        B.unchanged()
        return r

    a = keys(2 * np.arange(2 * T + 7), dt, False)
    empty = a[:0]
    assert inc(a, empty) and inc(empty, empty) and not inc(empty, a[:1])
    assert inc(a, a) and inc(a, a[::2]) and inc(a, a[-1:]) and inc(a, a[:1])
    # multiplicity: two copies against three
    two, three = np.repeat(a, 2), np.repeat(a[T // 2:T // 2 + 1], 3)
    assert inc(two, three[:2]) and not inc(two, three)
    assert inc(np.repeat(a, 3), three)
    # one offending element at each place around the tile boundaries of the
    # merged order (it moves 3 merged positions per step of p)
    sub = a[::2]
    for p in list(range(2 * T // 3 - 4, 2 * T // 3 + 5)) + list(range(4 * T // 3 - 4, 4 * T // 3 + 5)):
        extra = a[p:p + 1] + np.array(1, dtype=dt)  # odd: between two of A's keys
        assert not inc(a, np.sort(np.concatenate([sub, extra])))
        assert not inc(a, np.sort(np.concatenate([sub, a[p:p + 1], a[p:p + 1]])))  # one copy too many
    d = keys(2 * np.arange(T + 3), dt, True)
    assert inc(d, d[::3], True) and not inc(d[::3], d, True)


# ------------------------------------------------------------------ plumbing
def runs_data(n, dt, seed):
    rng = np.random.default_rng(seed)
    return keys(rng.integers(0, max(2, n // 2), n), dt, False)


def test_task_policy_returns_futures(gpu_target):
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    check_all(pt, gpu_target, runs_data(5 * T + 3, np.int64, 90), runs_data(3 * T + 1, np.int64, 91), False)


def test_back_to_back_on_one_stream(gpu_target):
    """Calls queued on one stream with the cached scratch, a large one and
    then a small one: no stale tile state."""
    t = gpu_target
    pt = ex.par(ex.task).on(hpx.default_executor(t))
    big = (runs_data(70 * T + 9, np.int64, 92), runs_data(50 * T + 1, np.int64, 93))
    small = (runs_data(3 * T + 1, np.int64, 94), runs_data(T - 3, np.int64, 95))
    queued = []
    for a, b in (big, small, big, small):
        A, B = Side(t, a, 0), Side(t, b, 0)
        for name in NAMES:
            o = hpx.vector.from_host(np.full(a.size + b.size, canary(a.dtype), dtype=a.dtype), t)
            queued.append((name, a, b, A, B, o, getattr(P, name)(pt, A.first, A.last, B.first, B.last, o.begin())))
    for name, a, b, A, B, o, f in queued:
        assert isinstance(f, hpx.future)
        want = SR.set_operation(SR.OPS[name], a, b)
        assert f.get() - o.begin() == want.size
        h = np.full(a.size + b.size, canary(a.dtype), dtype=a.dtype)
        h[:want.size] = want
        same(o.to_host(), h)


@pytest.mark.parametrize("op", range(4), ids=NAMES)
def test_caller_provided_scratch(gpu_target, op):
    """Exactly hpxhip_scratch_bytes bytes, a canary after them."""
    t = gpu_target
    a, b = runs_data(40 * T + 3, np.int64, 96), runs_data(25 * T + 1, np.int64, 97)
    n = a.size + b.size
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_SET_OPERATION, L.I64, 0, n, ctypes.byref(need))
    assert need.value > 0 and need.value % 8 == 0
    words = need.value // 8
    h_scr = np.full(words + 32, canary(np.int64), dtype=np.int64)
    scratch = hpx.vector.from_host(h_scr, t)
    da, db = hpx.vector.from_host(a, t), hpx.vector.from_host(b, t)
    h_out = np.full(n + 1, canary(np.int64), dtype=np.int64)
    o = hpx.vector.from_host(h_out, t)
    count = hpx.vector(1, dtype=np.uint64, tgt=t)
    vp = ctypes.c_void_p
    args = (L.I64, op, vp(da.begin().address), a.size, vp(db.begin().address), b.size, vp(o.begin().address), 0,
            vp(count.begin().address), t.stream, vp(scratch.begin().address))
    # a scratch that is one byte short is refused (before anything is queued)
    assert L.load().hpxhip_set_operation(*args, need.value - 1) == L.ERROR_INVALID_ARGUMENT
    L.call("hpxhip_set_operation", *args, need.value)
    L.call("hpxhip_stream_synchronize", t.stream)
    want = SR.set_operation(op, a, b)
    assert int(count.to_host()[0]) == want.size
    h_out[:want.size] = want
    same(o.to_host(), h_out)
    same(scratch.to_host()[words:], h_scr[words:])


def test_count_only_and_empty_ranges_write_the_count_only(gpu_target):
    t = gpu_target
    vp = ctypes.c_void_p
    o = hpx.vector.from_host(np.full(4, 5, dtype=np.int64), t)
    for op in range(4):
        count = hpx.vector.from_host(np.full(1, 77, dtype=np.uint64), t)
        L.call("hpxhip_set_operation", L.I64, op, None, 0, None, 0, vp(o.begin().address), 0,
               vp(count.begin().address), t.stream, None, 0)
        L.call("hpxhip_stream_synchronize", t.stream)
        assert int(count.to_host()[0]) == 0
    same(o.to_host(), np.full(4, 5, dtype=np.int64))
    # out == NULL: the count alone
    a, b = runs_data(3 * T + 1, np.int64, 98), runs_data(2 * T + 5, np.int64, 99)
    da, db = hpx.vector.from_host(a, t), hpx.vector.from_host(b, t)
    for op in range(4):
        count = hpx.vector.from_host(np.full(1, 77, dtype=np.uint64), t)
        L.call("hpxhip_set_operation", L.I64, op, vp(da.begin().address), a.size, vp(db.begin().address), b.size,
               None, 0, vp(count.begin().address), t.stream, None, 0)
        L.call("hpxhip_stream_synchronize", t.stream)
        assert int(count.to_host()[0]) == SR.set_operation(op, a, b).size
    same(da.to_host(), a)
    same(db.to_host(), b)


def test_injected_error_is_exception_list(pol, gpu_target):
    a, b = runs_data(1000, np.int64, 100), runs_data(900, np.int64, 101)
    da, db = hpx.vector.from_host(a, gpu_target), hpx.vector.from_host(b, gpu_target)
    o = hpx.vector.from_host(np.zeros(a.size + b.size, dtype=a.dtype), gpu_target)
    calls = [lambda n=n: getattr(P, n)(pol, da.begin(), da.end(), db.begin(), db.end(), o.begin()) for n in NAMES]
    calls.append(lambda: P.includes(pol, da.begin(), da.end(), db.begin(), db.end()))
    for call in calls:
        L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
        with pytest.raises(L.exception_list) as ei:
            call()
        assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
        L.call("hpxhip_debug_inject_error", 0, 0)
        same(o.to_host(), np.zeros(a.size + b.size, dtype=a.dtype))  # nothing was enqueued
    same(da.to_host(), a)
    same(db.to_host(), b)


# ---------------------------------------------------------- the C++ mirror
def test_cxx_set_operations_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "set_operations")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "set_operations: all tests passed" in r.stdout
