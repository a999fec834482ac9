"""partition_copy, stable_partition / partition and the remove family on the
GPU (hpxhip_partition_copy, hpxhip_stable_partition, compaction_kernel.hpp)
against numpy: with m the predicate on the host array, the accepted side is
``a[m]``, the rejected side ``a[~m]``, the stable partition
``np.concatenate((a[m], a[~m]))``.  Every buffer is compared whole and
bitwise against what it held before the call with the expected range written
into it, so canary elements either side of a range and, in place, the
elements from the new end onward must keep their values."""
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


# T-1, T, T+1, 2T+1, past one 64-tile look-back group, past two groups
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


def host_mask(a, pred):
    """The predicate on the host array, with the device's meaning."""
    arg = np.array(pred.arg).astype(a.dtype)
    k = pred.kind
    if k == L.P_LT:
        return a < arg
    if k == L.P_LE:
        return a <= arg
    if k == L.P_GT:
        return a > arg
    if k == L.P_GE:
        return a >= arg
    if k == L.P_EQ:
        return a == arg
    if k == L.P_NE:
        return a != arg
    if k == L.P_NOT_LT:
        return ~(a < arg)
    assert k == L.P_BITS
    return (a & arg) != 0


def canary(dt):
    return np.frombuffer(b"\x5a" * np.dtype(dt).itemsize, dtype=dt)[0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    assert got.size == want.size
    np.testing.assert_array_equal(bits(got), bits(want))


def from_mask(m, dt, seed):
    """Accepted elements in [0, 50), rejected ones in [50, 100), all random, so
    that order within each side shows; the predicate is less_than(50)."""
    rng = np.random.default_rng(seed)
    lo, hi = rng.integers(0, 50, m.size), rng.integers(50, 100, m.size)
    return np.where(m, lo, hi).astype(dt)


PRED50 = F.less_than(50)


def patterns(n, T, seed):
    """name -> acceptance mask."""
    i = np.arange(n)
    out = {"random": np.random.default_rng(seed).random(n) < 0.5, "all": np.ones(n, bool), "none": np.zeros(n, bool),
           "alternating tiles": (i // T) % 2 == 0}
    if n:
        for name, p in (("first", 0), ("last", n - 1), ("tile boundary", min(T, n) - 1), ("past boundary", min(T, n - 1))):
            m = np.zeros(n, bool)
            m[p] = True
            out["one: " + name] = m
    return out


class Run:
    """One partition_copy call through the Python mirror, its buffers laid out
    as [off canaries | range | one canary]; alias = "true" / "false" makes
    that destination the input range itself."""

    def __init__(self, pol, t, a, pred, it=0, ot=0, of=0, alias=None, fn=None):
        n, dt, c = a.size, a.dtype, canary(a.dtype)
        self.a, self.m = a, host_mask(a, pred)

        def buf(off, fill=None):
            b = np.full(off + n + 1, c, dtype=dt)
            if fill is not None:
                b[off:off + n] = fill
            return b
        self.h_in = buf(it, a)
        self.d_in = hpx.vector.from_host(self.h_in, t)
        first = self.d_in.begin() + it
        self.bufs = {}
        dest = {}
        for side, off in (("true", ot), ("false", of)):
            if alias == side:
                dest[side], self.bufs[side] = first, (self.d_in, self.h_in, it)
            else:
                h = buf(off)
                d = hpx.vector.from_host(h, t)
                dest[side], self.bufs[side] = d.begin() + off, (d, h, off)
        self.first, self.dest = first, dest
        self.alias = alias
        self.result = (fn or P.partition_copy)(pol, first, first + n, dest["true"], dest["false"], pred)

    def check(self, result=None):
        last, te, fe = result if result is not None else self.result
        a, m, n = self.a, self.m, self.a.size
        assert last - self.first == n
        assert te - self.dest["true"] == int(m.sum())
        assert fe - self.dest["false"] == n - int(m.sum())
        for side, ref in (("true", a[m]), ("false", a[~m])):
            d, before, off = self.bufs[side]
            want = before.copy()
            want[off:off + ref.size] = ref
            same(d.to_host(), want)
        if self.alias is None:
            same(self.d_in.to_host(), self.h_in)


# --------------------------------------------------------- partition_copy
@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("size", list(SIZES))
def test_partition_copy(pol, gpu_target, size, dt):
    n = size_of(size, dt)
    for k, (name, m) in enumerate(patterns(n, tile(dt), 100 + n % 97).items()):
        Run(pol, gpu_target, from_mask(m, dt, k), PRED50).check()


def float_data(dt, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, n).astype(dt)
    a[rng.random(n) < 0.1] = np.nan
    a[rng.random(n) < 0.1] = -0.0
    a[rng.random(n) < 0.1] = 0.0
    return a


PRED_KINDS = ["less_than", "less_equal", "greater_than", "greater_equal", "equal_to", "not_equal_to", "not_less_than"]


# any_bits is an integer predicate
@pytest.mark.parametrize("kind,dt", [(k, d) for d in (np.int32, np.float64) for k in PRED_KINDS] +
                         [("any_bits", np.int32)])
def test_every_predicate_kind(pol, gpu_target, kind, dt):
    n = 2 * tile(dt) + 1
    if kind == "any_bits":
        a, pred = np.random.default_rng(1).integers(0, 64, n).astype(dt), F.any_bits(5)
    elif np.dtype(dt).kind == "f":
        a, pred = float_data(dt, n, 2), getattr(F, kind)(0.0)
        assert np.isnan(a).any() and np.signbit(a[a == 0]).any() and (~np.signbit(a[a == 0])).any()
    else:
        a, pred = np.random.default_rng(3).integers(-3, 4, n).astype(dt), getattr(F, kind)(0)
    r = Run(pol, gpu_target, a, pred)
    assert 0 < r.m.sum() < n
    r.check()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_nan_goes_to_the_false_side(pol, gpu_target, dt):
    a = np.array([1.0, np.nan, -1.0, np.nan, 5.0, -0.0], dtype=dt)
    r = Run(pol, gpu_target, a, F.less_than(0.5))
    r.check()
    _, te, fe = r.result
    assert te - r.dest["true"] == 2 and fe - r.dest["false"] == 4


def abi_partition_copy(t, a, pred, want_true=True, want_false=True):
    """The C ABI with either output absent -> (count, true buffer, false buffer)."""
    n, c = a.size, canary(a.dtype)
    d_in = hpx.vector.from_host(a, t)
    outs = [hpx.vector.from_host(np.full(n + 1, c, dtype=a.dtype), t) if w else None for w in (want_true, want_false)]
    count = hpx.vector.from_host(np.full(1, 77, dtype=np.uint64), t)
    vp = ctypes.c_void_p
    L.call("hpxhip_partition_copy", d_in.begin().dtype, pred.kind, L.scalar_buf(d_in.begin().dtype, pred.arg), vp(d_in.begin().address),
           vp(outs[0].begin().address) if outs[0] else None, vp(outs[1].begin().address) if outs[1] else None, n,
           vp(count.begin().address), t.stream, None, 0)
    L.call("hpxhip_stream_synchronize", t.stream)
    return int(count.to_host()[0]), [o.to_host() if o else None for o in outs]


@pytest.mark.parametrize("dt", [np.int64, np.float32])
@pytest.mark.parametrize("size", ["3", "T+1", "65T+3"])
def test_each_output_absent(gpu_target, size, dt):
    n = size_of(size, dt)
    a = from_mask(np.random.default_rng(4).random(n) < 0.5, dt, 5)
    c_both, (t_both, f_both) = abi_partition_copy(gpu_target, a, PRED50)
    m = host_mask(a, PRED50)
    assert c_both == m.sum()
    same(t_both[:c_both], a[m])
    same(f_both[:n - c_both], a[~m])
    c1, (t1, f1) = abi_partition_copy(gpu_target, a, PRED50, want_false=False)
    assert c1 == c_both and f1 is None
    same(t1, t_both)
    c2, (t2, f2) = abi_partition_copy(gpu_target, a, PRED50, want_true=False)
    assert c2 == c_both and t2 is None
    same(f2, f_both)


# ----------------------------------------------------------------- aliasing
@pytest.mark.parametrize("alias", ["true", "false"])
@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("size", list(SIZES))
def test_in_place(pol, gpu_target, size, dt, alias):
    """dest_true == first, and dest_false == first (the remove_if path): the
    range sits 4 elements into its buffer (still 16-B aligned), so a canary
    lies either side; the elements from the new end to last keep their values."""
    n = size_of(size, dt)
    for k, (name, m) in enumerate(patterns(n, tile(dt), 200 + n % 89).items()):
        if name.startswith("one: ") and name not in ("one: first", "one: tile boundary"):
            continue
        Run(pol, gpu_target, from_mask(m, dt, 10 + k), PRED50, it=4, ot=4, of=4, alias=alias).check()


# --------------------------------------------------------------- sub-ranges
@pytest.mark.parametrize("dt", [np.int64, np.float32])
@pytest.mark.parametrize("of", [0, 1, 3])
@pytest.mark.parametrize("ot", [0, 1, 3])
@pytest.mark.parametrize("it", [0, 1, 3])
def test_sub_ranges(pol, gpu_target, it, ot, of, dt):
    n = 2 * tile(dt) + 1
    a = from_mask(np.random.default_rng(6).random(n) < 0.5, dt, 7)
    Run(pol, gpu_target, a, PRED50, it=it, ot=ot, of=of).check()


@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("n", [5, 1025, "2T+1"])
def test_sub_range_smaller_than_a_tile_and_element_wise(pol, gpu_target, n, dt):
    """n <= 4 * head takes the element-wise kernel, larger ones the split-off head."""
    n = size_of(n, dt) if isinstance(n, str) else n
    a = from_mask(np.random.default_rng(8).random(n) < 0.5, dt, 9)
    for it in (1, 3):
        Run(pol, gpu_target, a, PRED50, it=it).check()


@pytest.mark.parametrize("alias", ["true", "false"])
@pytest.mark.parametrize("dt", [np.int64, np.int32])
def test_sub_range_in_place(pol, gpu_target, dt, alias):
    n = 2 * tile(dt) + 1
    a = from_mask(np.random.default_rng(10).random(n) < 0.5, dt, 11)
    Run(pol, gpu_target, a, PRED50, it=1, ot=3, of=3, alias=alias).check()


# ------------------------------------------- stable_partition / partition
def in_place_call(fn, pol, t, a, arg, off=4):
    """fn(pol, first, last, arg) on [off canaries | a | canary] -> (returned - first, buffer, buffer before)."""
    h = np.full(off + a.size + 1, canary(a.dtype), dtype=a.dtype)
    h[off:off + a.size] = a
    d = hpx.vector.from_host(h, t)
    first = d.begin() + off
    r = fn(pol, first, first + a.size, arg)
    if isinstance(r, hpx.future):
        r = r.get()
    return r - first, d.to_host(), h


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("size", list(SIZES))
def test_stable_partition(pol, gpu_target, size, dt):
    n = size_of(size, dt)
    pats = patterns(n, tile(dt), 300 + n % 83)
    for k, name in enumerate(("random", "all", "none", "alternating tiles")):
        a = from_mask(pats[name], dt, 20 + k)
        m = host_mask(a, PRED50)
        for fn, off in ((P.stable_partition, 4), (P.partition, 1)):
            count, got, before = in_place_call(fn, pol, gpu_target, a, PRED50, off)
            assert count == m.sum()
            want = before.copy()
            want[off:off + n] = np.concatenate((a[m], a[~m]))
            same(got, want)


# ------------------------------------------------------------ remove family
@pytest.mark.parametrize("dt", [np.int32, np.uint64, np.float64])
@pytest.mark.parametrize("size", ["0", "1", "1025", "T+1", "65T+3"])
def test_remove_family(pol, gpu_target, size, dt):
    n = size_of(size, dt)
    rng = np.random.default_rng(12)
    a = rng.integers(0, 4, n).astype(dt)
    for what, arg in (("if", F.greater_equal(2)), ("value", 3)):
        m = host_mask(a, arg) if what == "if" else a == np.array(arg, dtype=dt)
        kept = a[~m]
        # in place
        fn = P.remove_if if what == "if" else P.remove
        count, got, before = in_place_call(fn, pol, gpu_target, a, arg)
        assert count == kept.size
        want = before.copy()
        want[4:4 + kept.size] = kept
        same(got, want)
        # out of place
        d_in = hpx.vector.from_host(a, gpu_target) if n else hpx.vector(1, dtype=dt, tgt=gpu_target)
        h_out = np.full(n + 2, canary(dt), dtype=dt)
        d_out = hpx.vector.from_host(h_out, gpu_target)
        fn = P.remove_copy_if if what == "if" else P.remove_copy
        last, end = fn(pol, d_in.begin(), d_in.begin() + n, d_out.begin() + 1, arg)
        assert last - d_in.begin() == n and end - (d_out.begin() + 1) == kept.size
        want = h_out.copy()
        want[1:1 + kept.size] = kept
        same(d_out.to_host(), want)
        if n:
            same(d_in.to_host(), a)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_remove_float_meaning(pol, gpu_target, dt):
    """rejected = !(x == value): a NaN is never removed, 0.0 removes -0.0 too."""
    a = np.array([0.0, 1.0, -0.0, np.nan, 2.0, np.nan, 0.0], dtype=dt)
    count, got, _ = in_place_call(P.remove, pol, gpu_target, a, float("nan"))
    assert count == a.size
    same(got[4:4 + a.size], a)
    count, got, _ = in_place_call(P.remove, pol, gpu_target, a, 0.0)
    assert count == 4
    same(got[4:8], a[[1, 3, 4, 5]])
    count, got, _ = in_place_call(P.remove, pol, gpu_target, a, -0.0)
    assert count == 4
    same(got[4:8], a[[1, 3, 4, 5]])


# ------------------------------------------------------------- 64-bit state
@pytest.mark.parametrize("dt", [np.int64, np.int32])
@pytest.mark.parametrize("size", ["2T+1", "65T+3"])
def test_state64(pol, gpu_target, monkeypatch, size, dt):
    """The 64-bit look-back state (used from 2^32 elements on) at small n."""
    n = size_of(size, dt)
    a = from_mask(np.random.default_rng(13).random(n) < 0.5, dt, 14)
    monkeypatch.setenv("HPXHIP_PARTITION_STATE64", "1")
    Run(pol, gpu_target, a, PRED50).check()
    Run(pol, gpu_target, a, PRED50, it=1, alias="false").check()
    m = host_mask(a, PRED50)
    count, got, _ = in_place_call(P.stable_partition, pol, gpu_target, a, PRED50)
    assert count == m.sum()
    same(got[4:4 + n], np.concatenate((a[m], a[~m])))


# -------------------------------------------------- stream and policy use
def test_back_to_back_on_one_stream(gpu_target):
    """Two calls queued on one stream with the cached scratch, the second on
    an input with fewer tiles: no stale tile state."""
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    a1 = from_mask(np.random.default_rng(15).random(70 * T8 + 9) < 0.5, np.int64, 16)
    a2 = from_mask(np.random.default_rng(17).random(3 * T8 + 1) < 0.3, np.int64, 18)
    r1 = Run(pt, gpu_target, a1, PRED50)
    r2 = Run(pt, gpu_target, a2, PRED50)
    h3 = a1.copy()
    d3 = hpx.vector.from_host(h3, gpu_target)
    f3 = P.stable_partition(pt, d3.begin(), d3.end(), PRED50)
    r4 = Run(pt, gpu_target, a2, PRED50, alias="false")
    for r in (r1, r2, r4):
        assert isinstance(r.result, hpx.future)
        r.check(r.result.get())
    assert f3.get() - d3.begin() == r1.m.sum()
    same(d3.to_host(), np.concatenate((a1[r1.m], a1[~r1.m])))


def test_task_policy_returns_futures(gpu_target):
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    a = from_mask(np.random.default_rng(19).random(100003) < 0.5, np.int32, 20)
    m = host_mask(a, PRED50)
    r = Run(pt, gpu_target, a, PRED50)
    assert isinstance(r.result, hpx.future)
    r.check(r.result.get())
    for fn, cnt in ((P.stable_partition, m.sum()), (P.partition, m.sum()), (P.remove_if, a.size - m.sum())):
        d = hpx.vector.from_host(a, gpu_target)
        f = fn(pt, d.begin(), d.end(), PRED50)
        assert isinstance(f, hpx.future)
        assert f.get() - d.begin() == cnt
    d, o = hpx.vector.from_host(a, gpu_target), hpx.vector(a.size, dtype=a.dtype, tgt=gpu_target)
    f = P.remove_copy_if(pt, d.begin(), d.end(), o.begin(), PRED50)
    assert isinstance(f, hpx.future)
    last, end = f.get()
    assert last - d.begin() == a.size and end - o.begin() == a.size - m.sum()
    same(o.to_host()[:end - o.begin()], a[~m])


def test_sort_then_remove_if_then_is_sorted(pol, gpu_target):
    n = 1 << 20
    a = np.random.default_rng(21).integers(-1000, 1000, n).astype(np.int64)
    d = hpx.vector.from_host(a, gpu_target)
    P.sort(pol, d.begin(), d.end())
    end = P.remove_if(pol, d.begin(), d.end(), F.any_bits(1))
    kept = np.sort(a)
    kept = kept[(kept & 1) == 0]
    assert end - d.begin() == kept.size
    assert P.is_sorted(pol, d.begin(), end)
    same(d.to_host()[:kept.size], kept)


# -------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("stable", [False, True])
def test_caller_provided_scratch(gpu_target, stable):
    """Exactly hpxhip_scratch_bytes bytes, a canary after them."""
    n = 65 * T8 + 3
    a = from_mask(np.random.default_rng(22).random(n) < 0.5, np.int64, 23)
    m = host_mask(a, PRED50)
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_STABLE_PARTITION if stable else L.ALGO_PARTITION_COPY, L.I64, 0, n,
           ctypes.byref(need))
    assert need.value > 0 and need.value % 8 == 0
    words = need.value // 8
    h_scr = np.full(words + 32, canary(np.int64), dtype=np.int64)
    scratch = hpx.vector.from_host(h_scr, gpu_target)
    d = hpx.vector.from_host(a, gpu_target)
    ot, of = (hpx.vector(n, dtype=np.int64, tgt=gpu_target) for _ in range(2))
    count = hpx.vector(1, dtype=np.uint64, tgt=gpu_target)
    vp = ctypes.c_void_p
    arg = L.scalar_buf(L.I64, PRED50.arg)
    lib = L.load()
    if stable:
        args = (L.I64, PRED50.kind, arg, vp(d.begin().address), n, vp(count.begin().address), gpu_target.stream,
                vp(scratch.begin().address))
        name = "hpxhip_stable_partition"
    else:
        args = (L.I64, PRED50.kind, arg, vp(d.begin().address), vp(ot.begin().address), vp(of.begin().address), n,
                vp(count.begin().address), gpu_target.stream, vp(scratch.begin().address))
        name = "hpxhip_partition_copy"
    L.call(name, *args, need.value)
    L.call("hpxhip_stream_synchronize", gpu_target.stream)
    c = int(count.to_host()[0])
    assert c == m.sum()
    if stable:
        same(d.to_host(), np.concatenate((a[m], a[~m])))
    else:
        same(ot.to_host()[:c], a[m])
        same(of.to_host()[:n - c], a[~m])
    same(scratch.to_host()[words:], h_scr[words:])
    # a scratch that is one byte short is refused
    assert getattr(lib, name)(*args, need.value - 1) == L.ERROR_INVALID_ARGUMENT


def test_injected_error_is_exception_list(pol, gpu_target):
    a = from_mask(np.random.default_rng(24).random(1000) < 0.5, np.int64, 25)
    d = hpx.vector.from_host(a, gpu_target)
    o = hpx.vector(a.size, dtype=a.dtype, tgt=gpu_target)
    calls = [lambda: P.partition_copy(pol, d.begin(), d.end(), d.begin(), o.begin(), PRED50),
             lambda: P.stable_partition(pol, d.begin(), d.end(), PRED50),
             lambda: P.remove_if(pol, d.begin(), d.end(), PRED50)]
    for call in calls:
        L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
        with pytest.raises(L.exception_list) as ei:
            call()
        assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
        L.call("hpxhip_debug_inject_error", 0, 0)
        same(d.to_host(), a)  # nothing was enqueued


# ---------------------------------------------------------- the C++ mirror
def test_cxx_partition_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "partition")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "partition: all tests passed" in r.stdout
