"""The set operations without a GPU: the host reference the GPU tests use
(tests/set_reference.py) against a literal two-pointer transcription of the
std::set_* loops and std::includes, the C++ mirror under the host compiler
(result types included; closures rejected there), the Python mirror's
argument checks before any device call, the C ABI's refusals and
hpxhip_scratch_bytes for the new algorithm."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import set_reference as SR
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from hpx_amd.compute import iterator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]
ALL_DT = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
NAMES = ["set_union", "set_intersection", "set_difference", "set_symmetric_difference"]


# ------------------------------------------------ the std loops, transcribed
# (keys: python ints from ordered_bits, so `<` is the device's comparator; the
# outputs are (range, index) pairs: which element went where)
def std_set_union(a, b):
    out, i, j = [], 0, 0
    while i < len(a):
        if j == len(b):
            return out + [(0, k) for k in range(i, len(a))]
        if b[j] < a[i]:
            out.append((1, j))
            j += 1
        else:
            out.append((0, i))
            if not a[i] < b[j]:
                j += 1
            i += 1
    return out + [(1, k) for k in range(j, len(b))]


def std_set_intersection(a, b):
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        else:
            if not b[j] < a[i]:
                out.append((0, i))
                i += 1
            j += 1
    return out


def std_set_difference(a, b):
    out, i, j = [], 0, 0
    while i < len(a):
        if j == len(b):
            return out + [(0, k) for k in range(i, len(a))]
        if a[i] < b[j]:
            out.append((0, i))
            i += 1
        else:
            if not b[j] < a[i]:
                i += 1
            j += 1
    return out


def std_set_symmetric_difference(a, b):
    out, i, j = [], 0, 0
    while i < len(a):
        if j == len(b):
            return out + [(0, k) for k in range(i, len(a))]
        if a[i] < b[j]:
            out.append((0, i))
            i += 1
        else:
            if b[j] < a[i]:
                out.append((1, j))
            else:
                i += 1
            j += 1
    return out + [(1, k) for k in range(j, len(b))]


def std_includes(a, b):
    i, j = 0, 0
    while j < len(b):
        if i == len(a) or b[j] < a[i]:
            return False
        if not a[i] < b[j]:
            j += 1
        i += 1
    return True


STD = {"set_union": std_set_union, "set_intersection": std_set_intersection, "set_difference": std_set_difference,
       "set_symmetric_difference": std_set_symmetric_difference}


def small_multiset(rng, dt, n, descending):
    """n keys from a small alphabet, sorted in the device's order; floats
    include both zeros, NaNs of both signs and two payloads, infinities."""
    if np.dtype(dt).kind == "f":
        u = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
        qnan = {4: 0x7fc00000, 8: 0x7ff8000000000000}[np.dtype(dt).itemsize]
        sign = 1 << (8 * np.dtype(dt).itemsize - 1)
        special = np.array([qnan, qnan | 1, qnan | sign, qnan | sign | 1], dtype=u).view(dt)
        alphabet = np.concatenate([np.array([-np.inf, -1.5, -0.0, 0.0, 1.5, 2.0, np.inf], dtype=dt), special])
    elif np.dtype(dt).kind == "i":
        alphabet = np.array([np.iinfo(dt).min, -3, -1, 0, 1, 2, 7, np.iinfo(dt).max], dtype=dt)
    else:
        alphabet = np.array([0, 1, 2, 3, 7, 1 << 31, np.iinfo(dt).max - 1, np.iinfo(dt).max], dtype=dt)
    k = int(rng.integers(1, len(alphabet) + 1))
    return SR.sort_keys(rng.choice(alphabet[rng.permutation(len(alphabet))[:k]], n), descending)


@pytest.mark.parametrize("descending", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", ALL_DT, ids=lambda d: np.dtype(d).name)
def test_reference_is_the_std_loops(dt, descending):
    rng = np.random.default_rng(1000 + ALL_DT.index(dt) * 2 + descending)
    for _ in range(300):
        a = small_multiset(rng, dt, int(rng.integers(0, 14)), descending)
        b = small_multiset(rng, dt, int(rng.integers(0, 14)), descending)
        ka = [int(x) for x in SR.ordered_bits(a, descending)]
        kb = [int(x) for x in SR.ordered_bits(b, descending)]
        assert ka == sorted(ka) and kb == sorted(kb)
        for name in NAMES:
            picks = STD[name](ka, kb)
            want = np.array([(a, b)[r][i] for r, i in picks], dtype=dt)
            got, src = SR.set_operation(SR.OPS[name], a, b, descending, with_source=True)
            assert got.tobytes() == want.tobytes(), (name, a, b)       # bitwise: -0.0, NaN payloads
            assert src.tolist() == [r for r, _ in picks], (name, a, b)  # and from which range
        assert SR.includes(a, b, descending) == std_includes(ka, kb), (a, b)
        assert SR.includes(b, a, descending) == std_includes(kb, ka), (a, b)


def test_reference_float_meaning():
    z = np.array([-0.0, 0.0], dtype=np.float64)
    assert SR.sort_keys(z[::-1]).tobytes() == z.tobytes()                      # -0.0 sorts before +0.0
    assert SR.set_operation(SR.INTERSECTION, z[:1], z[1:]).size == 0           # and does not match it
    assert not SR.includes(z[:1], z[1:])
    nan = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)
    assert SR.set_operation(SR.INTERSECTION, nan, nan.copy()).tobytes() == nan.tobytes()  # equal bits match
    neg = (nan.view(np.uint64) | np.uint64(1 << 63)).view(np.float64)
    s = SR.sort_keys(np.concatenate([nan, np.array([1.0]), neg]))
    assert s.tobytes() == np.concatenate([neg, np.array([1.0]), nan]).tobytes()  # NaNs at both ends


# ------------------------------------------------------------ the C++ mirror
def _compile(src: str):
    with tempfile.NamedTemporaryFile("w", suffix=".cpp", delete=False) as f:
        f.write(src)
        path = f.name
    try:
        return subprocess.run(CXX + [path], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)


PROLOGUE = """
#include <hpx/hpx.hpp>
#include <hpx/include/parallel_set_operations.hpp>
#include <functional>
#include <type_traits>
namespace ex = hpx::parallel::execution;
using vec = hpx::compute::vector<long>;
using It = vec::iterator;
"""


def test_mapped_comparators_compile_with_host_compiler():
    body = ""
    for name in NAMES:
        body += f"""
    e = hpx::parallel::{name}(p, a.begin(), a.end(), b.begin(), b.end(), c.begin());
    e = hpx::parallel::{name}(p, a.begin(), a.end(), b.begin(), b.end(), c.begin(), std::less<long>());
    e = hpx::{name}(ex::seq, a.begin(), a.end(), b.begin() + 1, b.end(), c.begin(), std::greater<>());
    e = hpx::{name}(ex::par, a.begin(), a.end(), b.begin(), b.end(), c.begin(), std::less<>());
    e = hpx::{name}(ex::par_unseq, a.begin(), a.end(), b.begin(), b.end(), c.begin(), std::greater<long>());
    fe = hpx::parallel::{name}(t, a.begin(), a.end(), b.begin(), b.end(), c.begin());
    fe = hpx::{name}(t, a.begin(), a.end(), b.begin(), b.end(), c.begin(), std::greater<>());
    static_assert(std::is_same<decltype(hpx::parallel::{name}(p, a.begin(), a.end(), b.begin(), b.end(), c.begin())),
                               It>::value, "FwdIter3");
    static_assert(std::is_same<decltype(hpx::parallel::{name}(t, a.begin(), a.end(), b.begin(), b.end(), c.begin(),
                                                              std::greater<>())),
                               hpx::future<It>>::value, "future of FwdIter3");
"""
    r = _compile(PROLOGUE + """
void f(vec& a, vec& b, vec& c) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    auto t = ex::par(ex::task).on(exec);
    It e;
    hpx::future<It> fe;
""" + body + """
    bool i = hpx::parallel::includes(p, a.begin(), a.end(), b.begin(), b.end());
    i = hpx::parallel::includes(p, a.begin(), a.end(), b.begin(), b.end(), std::less<long>());
    i = hpx::includes(ex::seq, a.begin(), a.end(), b.begin(), b.end(), std::greater<>());
    i = hpx::includes(ex::par, a.begin(), a.end(), b.begin(), b.end(), std::less<>());
    i = hpx::includes(ex::par_unseq, a.begin(), a.end(), b.begin(), b.end());
    hpx::future<bool> fi = hpx::parallel::includes(t, a.begin(), a.end(), b.begin(), b.end());
    fi = hpx::includes(t, a.begin(), a.end(), b.begin(), b.end(), std::greater<long>());
    static_assert(std::is_same<decltype(hpx::parallel::includes(p, a.begin(), a.end(), b.begin(), b.end())),
                               bool>::value, "bool");
    static_assert(std::is_same<decltype(hpx::parallel::includes(t, a.begin(), a.end(), b.begin(), b.end(),
                                                                std::less<>())),
                               hpx::future<bool>>::value, "future of bool");
    (void)e; (void)i; (void)fe; (void)fi;
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


def test_umbrella_header_lists_the_set_operations():
    r = _compile("""
#include <hpx/hpx.hpp>
#include <hpx/include/parallel_algorithm.hpp>
using It = hpx::compute::vector<int>::iterator;
bool f(It a, It b) { return hpx::includes(hpx::parallel::execution::par, a, b, a, b); }
""")
    assert r.returncode == 0, r.stderr[-4000:]


LAMBDA = "[](long x, long y) { return x / 2 < y / 2; }"


@pytest.mark.parametrize("call", [f"hpx::parallel::{n}(p, a.begin(), a.end(), b.begin(), b.end(), c.begin(), {LAMBDA});"
                                  for n in NAMES] +
                         [f"hpx::parallel::includes(p, a.begin(), a.end(), b.begin(), b.end(), {LAMBDA});"],
                         ids=NAMES + ["includes"])
def test_closures_need_hipcc(call):
    r = _compile(PROLOGUE + f"""
void f(vec& a, vec& b, vec& c) {{
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    {call}
}}
""")
    assert r.returncode != 0, call
    assert "compile the translation unit with hipcc" in r.stderr, r.stderr[-2000:]


# --------------------------------------------------------- the Python mirror
class _NoDeviceVector:
    """Stands in for a device vector: any device call through it fails."""

    def __init__(self, dtype, n=16):
        self.dtype, self.value_size, self._n = dtype, L.DTYPE_SIZE[dtype], n

    def __len__(self):
        return self._n

    def data(self):
        return 0x1000

    def target(self):
        raise AssertionError("a device call was made")


def _it(dt=L.I64):
    return iterator(_NoDeviceVector(dt), 0)


ALL = NAMES + ["includes"]


def _call(name, pol, f1, l1, f2, l2, dest, *comp):
    if name == "includes":
        return P.includes(pol, f1, l1, f2, l2, *comp)
    return getattr(P, name)(pol, f1, l1, f2, l2, dest, *comp)


@pytest.mark.parametrize("name", ALL)
def test_python_non_policy_is_type_error(name):
    a, b = _it(), _it()
    with pytest.raises(TypeError, match="execution policy"):
        _call(name, "par", a, a + 16, b, b + 16, _it())


@pytest.mark.parametrize("name", ALL)
def test_python_comparator_must_be_a_compare(name):
    a, b = _it(), _it()
    for bad in (F.plus, F.key_equal, F.less_than(3), lambda x, y: x < y, None):
        with pytest.raises(TypeError):
            _call(name, ex.par, a, a + 16, b, b + 16, _it(), bad)


@pytest.mark.parametrize("name", ALL)
def test_python_host_arrays_are_type_errors(name):
    h = np.zeros(16, dtype=np.int64)
    a = _it()
    with pytest.raises(TypeError, match="device iterators"):
        _call(name, ex.par, h, h, a, a + 16, _it())
    with pytest.raises(TypeError, match="device iterators"):
        _call(name, ex.par, a, a + 16, h, h, _it())
    if name != "includes":
        with pytest.raises(TypeError, match="device iterator"):
            _call(name, ex.par, a, a + 16, a, a + 16, h)


@pytest.mark.parametrize("name", ALL)
def test_python_mixed_dtypes_are_type_errors(name):
    a, u = _it(L.I64), _it(L.U64)
    with pytest.raises(TypeError, match="one dtype"):
        _call(name, ex.par, a, a + 16, u, u + 16, _it(L.I64))
    with pytest.raises(TypeError, match="one dtype"):
        _call(name, ex.par, u, u + 16, a, a + 16, _it(L.I64))
    if name != "includes":
        b = _it(L.I64)
        with pytest.raises(TypeError, match="one dtype"):
            _call(name, ex.par, a, a + 16, b, b + 16, _it(L.F64))


@pytest.mark.parametrize("name", ALL)
def test_python_reversed_range_is_value_error(name):
    a, b = _it(), _it()
    with pytest.raises(ValueError, match="last precedes first"):
        _call(name, ex.par, a + 8, a, b, b + 16, _it())
    with pytest.raises(ValueError, match="last precedes first"):
        _call(name, ex.par, a, a + 8, b + 16, b, _it())


# ------------------------------------------------------------------ the C ABI
def test_c_abi_invalid_arguments():
    lib = L.load()
    bufs = [(ctypes.c_int64 * 8)() for _ in range(3)]
    a, b, o = (ctypes.cast(x, ctypes.c_void_p) for x in bufs)
    count = ctypes.c_uint64(77)
    cp = ctypes.cast(ctypes.byref(count), ctypes.c_void_p)
    bad = L.ERROR_INVALID_ARGUMENT
    so = lib.hpxhip_set_operation
    for op in range(4):
        assert so(L.I64, op, a, 8, b, 8, o, 0, None, None, None, 0) == bad      # null count
        assert so(L.I64, op, None, 8, b, 8, o, 0, cp, None, None, 0) == bad     # null in1, n1 > 0
        assert so(L.I64, op, a, 8, None, 8, o, 0, cp, None, None, 0) == bad     # null in2, n2 > 0
        assert so(L.I64, op, None, 1, None, 0, None, 1, cp, None, None, 0) == bad
        assert so(77, op, a, 8, b, 8, o, 0, cp, None, None, 0) == bad           # unknown dtype
    for op in (-1, 4, 100):
        assert so(L.I64, op, a, 8, b, 8, o, 0, cp, None, None, 0) == bad        # unknown op
        assert so(L.I64, op, None, 0, None, 0, None, 0, cp, None, None, 0) == bad
    assert count.value == 77  # nothing was written
    assert (L.SET_UNION, L.SET_INTERSECTION, L.SET_DIFFERENCE, L.SET_SYMMETRIC_DIFFERENCE) == (0, 1, 2, 3)


@pytest.mark.parametrize("dt", [L.I32, L.U32, L.I64, L.U64, L.F32, L.F64])
def test_scratch_bytes_for_set_operation(dt):
    lib = L.load()
    prev = 0
    for n in (0, 1, 1000, 2047, 2048, 2049, 4097, 1 << 20, (1 << 20) + 1, 1 << 28, 1 << 33):
        v = ctypes.c_size_t()
        assert lib.hpxhip_scratch_bytes(L.ALGO_SET_OPERATION, dt, 0, n, ctypes.byref(v)) == 0
        assert v.value > 0 and v.value >= prev  # non-decreasing in n
        prev = v.value
    v = ctypes.c_size_t()
    assert L.ALGO_SET_OPERATION == 14
    assert lib.hpxhip_scratch_bytes(L.ALGO_SET_OPERATION + 1, dt, 0, 8, ctypes.byref(v)) == L.ERROR_INVALID_ARGUMENT
    assert lib.hpxhip_scratch_bytes(L.ALGO_SET_OPERATION, 77, 0, 8, ctypes.byref(v)) == L.ERROR_INVALID_ARGUMENT
