"""reduce_by_key on the GPU (hpxhip_reduce_by_key, reduce_by_key_kernel.hpp)
against a numpy reference: run boundaries are ``k[1:] != k[:-1]`` and the
run values ``ufunc.reduceat(v, starts, dtype=v.dtype)`` (without ``dtype=``
numpy widens small integer sums).  Integer values compare exactly; signed
sums stay inside the type's range, wrap-around uses unsigned values."""
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

# Elements per tile, for every key / value width: reduce_by_key_detail::
# tile_elems() in include/hpxhip/kernels/reduce_by_key_kernel.hpp (kThreads =
# 512 threads x kLaneElems = 16 elements per lane).
T = 8192
T8 = T4 = T

# T-1, T, T+1, 2T+1, past one 64-tile look-back group, past two groups
SIZES = [0, 1, 2, 3, 63, 64, 65, 1023, 1025, 100003, T - 1, T, T + 1, 2 * T + 1, 65 * T + 3, 129 * T + 5]
INT_DT = [np.int32, np.uint32, np.int64, np.uint64]
ALL_DT = INT_DT + [np.float32, np.float64]

UFUNC = {"plus": np.add, "multiplies": np.multiply, "minimum": np.minimum, "maximum": np.maximum,
         "bit_and": np.bitwise_and, "bit_or": np.bitwise_or, "bit_xor": np.bitwise_xor}


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


def run_starts(k):
    if k.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate(([0], np.flatnonzero(k[1:] != k[:-1]) + 1))


def reference(k, v, op="plus"):
    s = run_starts(k)
    if k.size == 0:
        return k[:0], v[:0]
    return k[s], UFUNC[op].reduceat(v, s, dtype=v.dtype)


def placed(a, off, t, extra=0):
    """Device vector holding a at element offset off."""
    buf = np.zeros(a.size + off + extra, dtype=a.dtype)
    buf[off:off + a.size] = a
    return hpx.vector.from_host(buf, t)


def gpu_rbk(pol, t, k, v, op="plus", offs=(0, 0, 0, 0), alias_k=False, alias_v=False):
    """-> (keys, values) of the runs, through the Python mirror."""
    n = k.size
    ko, vo, koo, voo = offs
    dk, dv = placed(k, ko, t, 1), placed(v, vo, t, 1)
    ok = dk if alias_k else hpx.vector(n + koo + 1, dtype=k.dtype, tgt=t)
    ov = dv if alias_v else hpx.vector(n + voo + 1, dtype=v.dtype, tgt=t)
    if alias_k:
        koo = ko
    if alias_v:
        voo = vo
    kb, vb = ok.begin() + koo, ov.begin() + voo
    ke, ve = P.reduce_by_key(pol, dk.begin() + ko, dk.begin() + ko + n, dv.begin() + vo, kb, vb, None,
                             getattr(F, op))
    c = ke - kb
    assert ve - vb == c
    assert 0 <= c <= n
    return ok.to_host()[koo:koo + c], ov.to_host()[voo:voo + c]


def check(pol, t, k, v, op="plus", **kw):
    gk, gv = gpu_rbk(pol, t, k, v, op, **kw)
    ek, ev = reference(k, v, op)
    assert gk.size == ek.size, (gk.size, ek.size)
    # bitwise on the keys: nan == nan, and -0.0 is told from +0.0
    np.testing.assert_array_equal(gk.view(np.uint8), ek.view(np.uint8))
    np.testing.assert_array_equal(gv, ev)


def keys_from_lengths(lens, n, dt=np.int64, seed=0):
    """Runs of the given lengths, consecutive runs with different keys."""
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 4, lens.size)) % 120  # steps of 1..3 mod 120: neighbours differ
    return np.repeat(ids, lens)[:n].astype(dt)


def recipe(n, seed, kdt=np.int64, vdt=np.int64):
    """The reference test's input: run lengths uniform in 1..256, consecutive
    runs with different keys, values uniform in [-256, 256]."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 257, n // 64 + 8)
    while lens.sum() < n:
        lens = np.concatenate((lens, rng.integers(1, 257, n // 64 + 8)))
    k = keys_from_lengths(lens, n, kdt, seed + 1)
    v = rng.integers(-256, 256, n, endpoint=True).astype(vdt)
    return k, v


def small_values(n, seed, dt=np.int64):
    return np.random.default_rng(seed).integers(-256, 256, n, endpoint=True).astype(dt)


# ------------------------------------------------------------- run shapes
@pytest.mark.parametrize("n", SIZES)
def test_all_keys_equal(pol, gpu_target, n):
    """One run through every tile."""
    k, v = np.full(n, 7, dtype=np.int64), small_values(n, 1)
    gk, gv = gpu_rbk(pol, gpu_target, k, v)
    assert gk.size == min(n, 1)
    check(pol, gpu_target, k, v)


@pytest.mark.parametrize("n", SIZES)
def test_all_keys_distinct(pol, gpu_target, n):
    k, v = np.arange(n, dtype=np.int64) * 3 - 5, small_values(n, 2)
    gk, gv = gpu_rbk(pol, gpu_target, k, v)
    assert gk.size == n
    np.testing.assert_array_equal(gk, k)
    np.testing.assert_array_equal(gv, v)


@pytest.mark.parametrize("n", SIZES)
def test_reference_recipe(pol, gpu_target, n):
    check(pol, gpu_target, *recipe(n, 3 + n))


@pytest.mark.parametrize("first", [T - 1, T, T + 1])
def test_runs_of_one_tile(pol, gpu_target, first):
    """Run length exactly T; the first boundary at T-1, T, T+1."""
    n = first + 4 * T + 17
    lens = np.array([first] + [T] * 5)
    check(pol, gpu_target, keys_from_lengths(lens, n), small_values(n, 4))


def test_long_run_between_short_runs(pol, gpu_target):
    """A run of 3.5 tiles: tiles without any boundary between tiles with one."""
    lens = np.array([5, 3, 100, 1, 7 * T // 2, 2, 9, 1, 1, 400, 7 * T // 2, 3])
    n = int(lens.sum())
    check(pol, gpu_target, keys_from_lengths(lens, n), small_values(n, 5))


def test_lengths_1_and_100000_alternating(pol, gpu_target):
    lens = np.array([1, 100000] * 6 + [1])
    n = int(lens.sum())
    check(pol, gpu_target, keys_from_lengths(lens, n), small_values(n, 6))


# --------------------------------------------------------- dtypes and ops
def values_for(dt, n, seed):
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    if dt.kind == "u":
        return rng.integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)  # sums wrap
    return rng.integers(-256, 256, n, endpoint=True).astype(dt)  # exact in every dtype


@pytest.mark.parametrize("kdt", ALL_DT)
def test_every_key_dtype(pol, gpu_target, kdt):
    n = 2 * T4 + 1
    k, _ = recipe(n, 11, kdt)
    check(pol, gpu_target, k, small_values(n, 12))


@pytest.mark.parametrize("vdt", ALL_DT)
def test_every_value_dtype(pol, gpu_target, vdt):
    n = 2 * T4 + 1
    k, _ = recipe(n, 13)
    check(pol, gpu_target, k, values_for(vdt, n, 14))


@pytest.mark.parametrize("kdt,vdt", [(np.uint32, np.float64), (np.int64, np.int32), (np.float32, np.uint64),
                                     (np.float64, np.float32)])
@pytest.mark.parametrize("n", [100003, 65 * T8 + 3])
def test_mixed_widths(pol, gpu_target, kdt, vdt, n):
    k, _ = recipe(n, 15, kdt)
    check(pol, gpu_target, k, values_for(vdt, n, 16))


@pytest.mark.parametrize("vdt", ALL_DT)
@pytest.mark.parametrize("op", ["plus", "minimum", "maximum"])
def test_ops(pol, gpu_target, vdt, op):
    n = 2 * T4 + 1
    k, _ = recipe(n, 17, np.int32)
    check(pol, gpu_target, k, values_for(vdt, n, 18), op)


@pytest.mark.parametrize("vdt", ALL_DT)
def test_multiplies(pol, gpu_target, vdt):
    """Values in {-1, 1, 2} ({1, 2} unsigned), runs of 1..16: products fit."""
    n = 2 * T4 + 1
    rng = np.random.default_rng(19)
    lens = rng.integers(1, 17, n // 4 + 8)
    k = keys_from_lengths(lens, n, np.int64, 20)
    choices = [1, 2] if np.dtype(vdt).kind == "u" else [-1, 1, 2]
    v = rng.choice(choices, n).astype(vdt)
    check(pol, gpu_target, k, v, "multiplies")


@pytest.mark.parametrize("vdt", INT_DT)
@pytest.mark.parametrize("op", ["bit_and", "bit_or", "bit_xor"])
def test_bit_ops(pol, gpu_target, vdt, op):
    n = 2 * T4 + 1
    k, _ = recipe(n, 21)
    info = np.iinfo(vdt)
    v = np.random.default_rng(22).integers(info.min, info.max, n, dtype=vdt, endpoint=True)
    check(pol, gpu_target, k, v, op)


@pytest.mark.parametrize("vdt", [np.float32, np.float64])
@pytest.mark.parametrize("op", ["bit_and", "bit_or", "bit_xor"])
def test_bit_ops_on_floats_unsupported(pol, gpu_target, vdt, op):
    k, v = recipe(1000, 23, np.int64, vdt)
    with pytest.raises(L.exception_list) as ei:
        gpu_rbk(pol, gpu_target, k, v, op)
    assert ei.value.status == L.ERROR_UNSUPPORTED


# -------------------------------------------------------------- float keys
@pytest.mark.parametrize("kdt", [np.float32, np.float64])
def test_float_keys_compare_by_value(pol, gpu_target, kdt):
    """-0.0 == +0.0 is one run, every NaN a run of its own (std::equal_to)."""
    k = np.array([0.0, -0.0, np.nan, np.nan, 1.0, 1.0], dtype=kdt)
    v = np.arange(1, 7, dtype=np.int64)
    gk, gv = gpu_rbk(pol, gpu_target, k, v)
    np.testing.assert_array_equal(gv, [3, 3, 4, 11])
    np.testing.assert_array_equal(gk.view(np.uint8), k[[0, 2, 3, 4]].view(np.uint8))
    # the same pattern tiled across tile boundaries (6 does not divide T)
    reps = (2 * T8 + 6) // 6
    kk, vv = np.tile(k, reps), small_values(6 * reps, 24)
    gk, gv = gpu_rbk(pol, gpu_target, kk, vv)
    ek, ev = reference(kk, vv)
    assert ek.size == 4 * reps
    np.testing.assert_array_equal(gk.view(np.uint8), ek.view(np.uint8))
    np.testing.assert_array_equal(gv, ev)


# ---------------------------------------------------- floating-point values
@pytest.mark.parametrize("vdt,n", [(np.float64, 129 * T8 + 5), (np.float32, 65 * T8 + 3)])
def test_integer_valued_floats_exact(pol, gpu_target, vdt, n):
    """Run sums below 2^53 / 2^24 in magnitude: any association is exact."""
    k, v = recipe(n, 25, np.int64, vdt)  # |sum| <= 256 * 256 = 2^16
    check(pol, gpu_target, k, v)


@pytest.mark.parametrize("vdt,kdt,n", [(np.float64, np.int64, 129 * T8 + 5), (np.float32, np.int32, 129 * T4 + 5),
                                       (np.float64, np.int32, 100003), (np.float32, np.int64, 100003)])
def test_float_sums_bound_and_reproducible(pol, gpu_target, vdt, kdt, n):
    """|gpu - longdouble| <= m * u * sum|x| per run of length m (the bound of
    any summation order), and three runs agree bit for bit."""
    rng = np.random.default_rng(26)
    # long and short runs: lengths 1..256 and a few of several tiles
    lens = rng.integers(1, 257, n // 64 + 8)
    lens[::97] = 3 * T8 + 11
    k = keys_from_lengths(lens, n, kdt, 27)
    v = rng.standard_normal(n).astype(vdt)
    gk, gv = gpu_rbk(pol, gpu_target, k, v)
    s = run_starts(k)
    np.testing.assert_array_equal(gk, k[s])
    m = np.diff(np.concatenate((s, [n])))
    exact = np.add.reduceat(v.astype(np.longdouble), s)
    mag = np.add.reduceat(np.abs(v).astype(np.longdouble), s)
    u = 2.0 ** -53 if vdt == np.float64 else 2.0 ** -24
    err = np.abs(gv.astype(np.longdouble) - exact)
    bad = np.flatnonzero(err > m * u * mag)
    assert bad.size == 0, (bad[:5], err[bad[:5]], (m * u * mag)[bad[:5]])
    for _ in range(2):
        _, again = gpu_rbk(pol, gpu_target, k, v)
        np.testing.assert_array_equal(again.view(np.uint8), gv.view(np.uint8))


# ----------------------------------------------------------------- in place
def inplace_inputs(kind, n):
    if kind == "distinct":
        return np.arange(n, dtype=np.int64), small_values(n, 28)
    if kind == "equal":
        return np.full(n, 3, dtype=np.int64), small_values(n, 29)
    return recipe(n, 30)


@pytest.mark.parametrize("alias_k,alias_v", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("kind", ["distinct", "equal", "recipe"])
@pytest.mark.parametrize("n", [2 * T + 1, 129 * T + 5])
def test_in_place(pol, gpu_target, kind, alias_k, alias_v, n):
    """keys_output == key_first and / or values_output == values_first (as the
    reference's own test runs it); the tail past count is not checked."""
    k, v = inplace_inputs(kind, n)
    check(pol, gpu_target, k, v, alias_k=alias_k, alias_v=alias_v)


# --------------------------------------------------------------- sub-ranges
OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 3), (3, 1, 0, 0), (1, 3, 3, 1), (3, 3, 3, 3),
           (1, 1, 3, 0)]


@pytest.mark.parametrize("offs", OFFSETS)
@pytest.mark.parametrize("n", [2 * T + 1, 100003])
@pytest.mark.parametrize("kdt,vdt", [(np.int64, np.int64), (np.int32, np.float32), (np.uint32, np.float64)])
def test_sub_ranges(pol, gpu_target, kdt, vdt, n, offs):
    """Element offsets (keys, values, keys_output, values_output)."""
    k, v = recipe(n, 31, kdt, vdt)
    check(pol, gpu_target, k, v, offs=offs)


def test_sub_ranges_in_place(pol, gpu_target):
    k, v = recipe(2 * T + 1, 32)
    check(pol, gpu_target, k, v, offs=(1, 3, 0, 0), alias_k=True, alias_v=True)


# ------------------------------------------------------------- 64-bit state
@pytest.mark.parametrize("n", [1025, 2 * T + 1, 65 * T + 3])
@pytest.mark.parametrize("kdt,vdt", [(np.int64, np.int64), (np.int32, np.float32)])
def test_state64(pol, gpu_target, monkeypatch, kdt, vdt, n):
    """The 64-bit run count (used from 2^32 elements on) at small n."""
    k, v = recipe(n, 33, kdt, vdt)
    first = gpu_rbk(pol, gpu_target, k, v)
    monkeypatch.setenv("HPXHIP_REDUCE_BY_KEY_STATE64", "1")
    second = gpu_rbk(pol, gpu_target, k, v)
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[1], second[1])
    check(pol, gpu_target, k, v)


# -------------------------------------------------- stream and policy use
def test_back_to_back_on_one_stream(gpu_target):
    """Two calls queued on one stream with the cached scratch, the second on
    an input with fewer tiles: no stale tile state."""
    k1, v1 = recipe(70 * T + 9, 34)
    k2, v2 = recipe(3 * T + 1, 35)
    d = [hpx.vector.from_host(a, gpu_target) for a in (k1, v1, k2, v2)]
    o = [hpx.vector(a.size, dtype=a.dtype, tgt=gpu_target) for a in (k1, v1, k2, v2)]
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    f1 = P.reduce_by_key(pt, d[0].begin(), d[0].end(), d[1].begin(), o[0].begin(), o[1].begin())
    f2 = P.reduce_by_key(pt, d[2].begin(), d[2].end(), d[3].begin(), o[2].begin(), o[3].begin())
    for f, (k, v), (ok, ov) in ((f1, (k1, v1), o[:2]), (f2, (k2, v2), o[2:])):
        ke, ve = f.get()
        ek, ev = reference(k, v)
        assert ke - ok.begin() == ek.size and ve - ov.begin() == ek.size
        np.testing.assert_array_equal(ok.to_host()[:ek.size], ek)
        np.testing.assert_array_equal(ov.to_host()[:ek.size], ev)


def test_task_policy_returns_future(gpu_target):
    k, v = recipe(100003, 36)
    dk, dv = hpx.vector.from_host(k, gpu_target), hpx.vector.from_host(v, gpu_target)
    ok, ov = hpx.vector(k.size, dtype=k.dtype, tgt=gpu_target), hpx.vector(v.size, dtype=v.dtype, tgt=gpu_target)
    pt = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    f = P.reduce_by_key(pt, dk.begin(), dk.end(), dv.begin(), ok.begin(), ov.begin(), F.key_equal, F.plus)
    assert isinstance(f, hpx.future)
    ke, ve = f.get()
    ek, ev = reference(k, v)
    assert ke - ok.begin() == ek.size and ve - ov.begin() == ek.size
    np.testing.assert_array_equal(ov.to_host()[:ek.size], ev)


def test_sort_by_key_then_reduce_by_key(pol, gpu_target):
    """The group-by pipeline: counts per key equal np.unique's."""
    n = 1 << 20
    k = np.random.default_rng(37).integers(0, 1000, n).astype(np.int64)
    dk, dv = hpx.vector.from_host(k, gpu_target), hpx.vector.from_host(np.ones(n, dtype=np.int64), gpu_target)
    P.sort_by_key(pol, dk.begin(), dk.end(), dv.begin())
    ke, ve = P.reduce_by_key(pol, dk.begin(), dk.end(), dv.begin(), dk.begin(), dv.begin())
    uk, uc = np.unique(k, return_counts=True)
    assert ke - dk.begin() == uk.size and ve - dv.begin() == uk.size
    np.testing.assert_array_equal(dk.to_host()[:uk.size], uk)
    np.testing.assert_array_equal(dv.to_host()[:uk.size], uc)


# -------------------------------------------------------------- the C ABI
def test_caller_provided_scratch(gpu_target):
    n = 65 * T + 3
    k, v = recipe(n, 38)
    dk, dv = hpx.vector.from_host(k, gpu_target), hpx.vector.from_host(v, gpu_target)
    ok, ov = hpx.vector(n, dtype=np.int64, tgt=gpu_target), hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_REDUCE_BY_KEY, L.I64, L.I64, n, ctypes.byref(need))
    assert need.value > 0
    scratch = hpx.vector((need.value + 7) // 8, dtype=np.int64, tgt=gpu_target)
    count = hpx.vector(1, dtype=np.uint64, tgt=gpu_target)
    vp = ctypes.c_void_p
    L.call("hpxhip_reduce_by_key", L.I64, L.I64, L.PLUS, vp(dk.begin().address), vp(dv.begin().address),
           vp(ok.begin().address), vp(ov.begin().address), n, vp(count.begin().address), gpu_target.stream,
           vp(scratch.begin().address), need.value)
    L.call("hpxhip_stream_synchronize", gpu_target.stream)
    ek, ev = reference(k, v)
    assert int(count.to_host()[0]) == ek.size
    np.testing.assert_array_equal(ok.to_host()[:ek.size], ek)
    np.testing.assert_array_equal(ov.to_host()[:ek.size], ev)
    # a scratch that is too small is refused
    lib = L.load()
    rc = lib.hpxhip_reduce_by_key(L.I64, L.I64, L.PLUS, vp(dk.begin().address), vp(dv.begin().address),
                                  vp(ok.begin().address), vp(ov.begin().address), n, vp(count.begin().address),
                                  gpu_target.stream, vp(scratch.begin().address), 64)
    assert rc == L.ERROR_INVALID_ARGUMENT


def test_injected_error_is_exception_list(pol, gpu_target):
    k, v = recipe(1000, 39)
    dk, dv = hpx.vector.from_host(k, gpu_target), hpx.vector.from_host(v, gpu_target)
    L.call("hpxhip_debug_inject_error", L.ERROR_INVALID_ARGUMENT, 1)
    with pytest.raises(L.exception_list) as ei:
        P.reduce_by_key(pol, dk.begin(), dk.end(), dv.begin(), dk.begin(), dv.begin())
    assert len(ei.value) == 1 and ei.value.status == L.ERROR_INVALID_ARGUMENT
    np.testing.assert_array_equal(dk.to_host(), k)  # nothing was enqueued
    L.call("hpxhip_debug_inject_error", 0, 0)


# ---------------------------------------------------------- the C++ mirror
def test_cxx_reduce_by_key_program():
    exe = os.path.join(ROOT, "tests", "cxx", "bin", "reduce_by_key")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} not built (run `make cxxtests` / __graft_entry__.build())")
    r = subprocess.run([exe, "20261019"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "reduce_by_key: all tests passed" in r.stdout
