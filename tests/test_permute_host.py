"""reverse, rotate, swap_ranges, replace and adjacent_difference without a
GPU: the NumPy reference the GPU tests use (tests/permute_reference.py)
against literal transcriptions of the sequential loops (std::reverse as in
reverse.hpp:48, sequential_rotate_helper of rotate.hpp:39-55, std::replace_if
/ std::replace_copy_if of replace.hpp, std::adjacent_difference of
adjacent_difference.hpp), the C ABI's refusals -- every one of them before
any device call, so they hold on a machine without a device --, the ctypes
table, the Python mirror's argument checks and the C++ mirror's result types
under the host compiler."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import permute_reference as PR
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from hpx_amd.compute import iterator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]
ALL_DT = PR.ALL_DT
SIZES = list(range(10)) + [255, 256, 257, 300]


# ------------------------------------------------ the std loops, transcribed
def std_reverse(a):
    a = a.copy()
    first, last = 0, len(a)
    while first != last:
        last -= 1
        if first == last:
            break
        a[first], a[last] = a[last], a[first]
        first += 1
    return a


def std_rotate(a, mid):
    """sequential_rotate (rotate.hpp:39-64) -> (array, index of the old first)."""
    a = a.copy()
    first, new_first, last = 0, mid, len(a)
    if first != new_first and new_first != last:
        nxt = new_first
        while first != nxt:
            a[first], a[nxt] = a[nxt], a[first]
            first += 1
            nxt += 1
            if nxt == last:
                nxt = new_first
            elif first == new_first:
                new_first = nxt
    return a, len(a) - mid


def std_replace_copy_if(a, pred, new):
    out = a.copy()
    for i in range(len(a)):
        out[i] = new if pred(a[i]) else a[i]
    return out


def std_adjacent_difference(a, op):
    out = a.copy()
    if len(a) == 0:
        return out
    acc = a[0]
    for i in range(1, len(a)):
        val = a[i]
        out[i] = op(val, acc)
        acc = val
    return out


@pytest.mark.parametrize("dt", ALL_DT)
def test_reference_reverse_and_rotate_match_the_std_loops(dt):
    for n in SIZES:
        a = PR.sample(dt, n)
        assert PR.same(PR.reverse(a), std_reverse(a))
        for mid in sorted({0, 1, n // 2, max(n - 1, 0), n} & set(range(n + 1))):
            want, ret = std_rotate(a, mid)
            assert PR.same(PR.rotate(a, mid), want), (n, mid)
            assert ret == n - mid


@pytest.mark.parametrize("dt", ALL_DT)
def test_reference_replace_matches_the_std_loop(dt):
    preds = {L.P_LT: lambda x, a: x < a, L.P_LE: lambda x, a: x <= a, L.P_GT: lambda x, a: x > a,
             L.P_GE: lambda x, a: x >= a, L.P_EQ: lambda x, a: x == a, L.P_NE: lambda x, a: x != a,
             L.P_NOT_LT: lambda x, a: not x < a}
    if np.dtype(dt).kind != "f":
        preds[L.P_BITS] = lambda x, a: (x & a) != 0
    for n in SIZES:
        a = PR.sample(dt, n)
        for kind, fn in preds.items():
            arg, new = dt(1), dt(5)
            want = std_replace_copy_if(a, lambda x: fn(x, arg), new)
            assert PR.same(PR.replace_if(a, kind, arg, new), want), (n, kind)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_reference_replace_float_corner_cases(dt):
    nan = dt("nan")
    a = np.array([0.0, -0.0, 1.5, nan, -0.0, 2.0], dtype=dt)
    # 0.0 replaces -0.0 too (compared by value)
    r = PR.replace(a, 0.0, 7.0)
    assert PR.same(r, np.array([7.0, 7.0, 1.5, nan, 7.0, 2.0], dtype=dt))
    assert PR.same(r, std_replace_copy_if(a, lambda x: x == dt(0.0), dt(7.0)))
    # a NaN old value replaces nothing
    assert PR.same(PR.replace(a, nan, 7.0), a)
    assert PR.same(std_replace_copy_if(a, lambda x: x == nan, dt(7.0)), a)
    # a NaN new value is written with its bits
    r = PR.replace(a, 1.5, nan)
    assert np.isnan(r[2]) and PR.same(r[2:3], np.array([nan], dtype=dt))
    assert PR.same(np.delete(r, 2), np.delete(a, 2))


@pytest.mark.parametrize("dt", ALL_DT)
def test_reference_adjacent_difference_matches_the_std_loop(dt):
    with np.errstate(over="ignore", invalid="ignore"):
        for n in SIZES:
            a = PR.sample(dt, n)
            assert PR.same(PR.adjacent_difference(a), std_adjacent_difference(a, lambda x, y: x - y)), n
            assert PR.same(PR.adjacent_difference(a, L.B_MAX),
                           std_adjacent_difference(a, lambda x, y: y if x < y else x)), n


def test_reference_differences_wrap():
    a = np.array([0, 1, 0], dtype=np.uint32)
    assert PR.adjacent_difference(a).tolist() == [0, 1, 0xFFFFFFFF]
    a = np.array([5, 2**64 - 1, 0], dtype=np.uint64)
    assert PR.adjacent_difference(a).tolist() == [5, 2**64 - 6, 1]
    a = np.array([np.iinfo(np.int32).max, np.iinfo(np.int32).min, 3], dtype=np.int32)
    assert PR.adjacent_difference(a).tolist() == [2**31 - 1, 1, -(2**31) + 3]
    # first differences undo a wrapping inclusive scan
    x = PR.sample(np.int32, 300)
    assert PR.same(PR.adjacent_difference(np.cumsum(x, dtype=np.int32)), x)


# ------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ["hpxhip_reverse", "hpxhip_reverse_copy", "hpxhip_rotate", "hpxhip_rotate_copy", "hpxhip_swap_ranges",
               "hpxhip_replace_if", "hpxhip_adjacent_difference"]


def test_ctypes_table_covers_the_new_symbols():
    lib = L.load()
    want = {"hpxhip_reverse": 4, "hpxhip_reverse_copy": 5, "hpxhip_rotate": 5, "hpxhip_rotate_copy": 6,
            "hpxhip_swap_ranges": 5, "hpxhip_replace_if": 8, "hpxhip_adjacent_difference": 7}
    for name in NEW_SYMBOLS:
        assert len(L.SIGNATURES[name]) == want[name]
        assert getattr(lib, name).argtypes == L.SIGNATURES[name]
    assert lib.hpxhip_abi_version() == 1
    # no entry point takes scratch: no new algorithm id
    v = ctypes.c_size_t()
    for algo in (11, 15):
        assert lib.hpxhip_scratch_bytes(algo, L.I64, 0, 8, ctypes.byref(v)) == L.ERROR_INVALID_ARGUMENT


def _vp(x):
    return ctypes.c_void_p(x)


BAD = L.ERROR_INVALID_ARGUMENT
A, B = 0x10000, 0x20000  # fake addresses: a refusal must come before any device call


def _calls(dt, a, b, n, mid=0):
    """Every entry point with the two ranges a, b (b unused by the in-place ones)."""
    lib = L.load()
    one = L.scalar_buf(dt if dt in L.CTYPE else L.I64, 1)
    return {
        "reverse": lambda: lib.hpxhip_reverse(dt, _vp(a), n, None),
        "reverse_copy": lambda: lib.hpxhip_reverse_copy(dt, _vp(a), _vp(b), n, None),
        "rotate": lambda: lib.hpxhip_rotate(dt, _vp(a), mid, n, None),
        "rotate_copy": lambda: lib.hpxhip_rotate_copy(dt, _vp(a), mid, n, _vp(b), None),
        "swap_ranges": lambda: lib.hpxhip_swap_ranges(dt, _vp(a), _vp(b), n, None),
        "replace_if": lambda: lib.hpxhip_replace_if(dt, L.P_EQ, one, one, _vp(a), _vp(b), n, None),
        "adjacent_difference": lambda: lib.hpxhip_adjacent_difference(dt, L.B_SUB, None, _vp(a), _vp(b), n, None),
    }


TWO_RANGES = ["reverse_copy", "rotate_copy", "swap_ranges", "replace_if", "adjacent_difference"]


@pytest.mark.parametrize("dt", [L.I32, L.U32, L.I64, L.U64, L.F32, L.F64])
def test_c_abi_refusals_need_no_device(dt):
    es = L.DTYPE_SIZE[dt]
    # n == 0 returns 0 and touches nothing, also with null pointers
    for name, call in _calls(dt, None, None, 0).items():
        assert call() == 0, name
    # null pointers with n > 0
    for name, call in _calls(dt, None, B, 8, 3).items():
        assert call() == BAD, name
    for name, call in _calls(dt, A, None, 8, 3).items():
        if name in TWO_RANGES:
            assert call() == BAD, name
    # pointers not aligned to the element
    for off in (1, 2, es - 1):
        for name, call in _calls(dt, A + off, B, 8, 3).items():
            assert call() == BAD, (name, off)
        for name, call in _calls(dt, A, B + off, 8, 3).items():
            if name in TWO_RANGES:
                assert call() == BAD, (name, off)
    # mid > n
    lib = L.load()
    for n, mid in ((8, 9), (0, 1), (8, 2**63)):
        assert lib.hpxhip_rotate(dt, _vp(A), mid, n, None) == BAD
        assert lib.hpxhip_rotate_copy(dt, _vp(A), mid, n, _vp(B), None) == BAD
    # mid == 0 and mid == n launch nothing (no device is needed)
    assert lib.hpxhip_rotate(dt, _vp(A), 0, 8, None) == 0
    assert lib.hpxhip_rotate(dt, _vp(A), 8, 8, None) == 0
    # unknown dtype
    for name, call in _calls(77, A, B, 8, 3).items():
        assert call() == BAD, name


@pytest.mark.parametrize("dt", [L.I32, L.F64])
def test_c_abi_overlap_is_refused(dt):
    es = L.DTYPE_SIZE[dt]
    n = 100
    # out inside in, in inside out, by one element at either end
    for b in (A + es, A - es, A + (n - 1) * es, A - (n - 1) * es, A + (n // 2) * es):
        for name, call in _calls(dt, A, b, n, 3).items():
            if name in TWO_RANGES:
                assert call() == BAD, (name, hex(b))
    # exactly the same range: only replace_if accepts it (then it goes on to
    # the device, so it is not called here)
    for name, call in _calls(dt, A, A, n, 3).items():
        if name in TWO_RANGES and name != "replace_if":
            assert call() == BAD, name
    # touching ranges do not overlap: the call passes the host checks (what it
    # returns without a device is not INVALID_ARGUMENT on a GPU machine; here
    # only n == 0 can show it without a device call)
    for name, call in _calls(dt, A, A + n * es, 0, 0).items():
        assert call() == 0, name


def test_c_abi_unknown_kinds_and_bits_on_floats():
    lib = L.load()
    one = L.scalar_buf(L.I64, 1)
    for kind in (-1, 8, 100):
        assert lib.hpxhip_replace_if(L.I64, kind, one, one, _vp(A), _vp(B), 8, None) == BAD
    for kind in (-1, 7, 100):
        assert lib.hpxhip_adjacent_difference(L.I64, kind, None, _vp(A), _vp(B), 8, None) == BAD
    for dt in (L.F32, L.F64):
        f1 = L.scalar_buf(dt, 1.0)
        assert lib.hpxhip_replace_if(dt, L.P_BITS, f1, f1, _vp(A), _vp(B), 8, None) == L.ERROR_UNSUPPORTED
    # null pred_arg / new_value
    assert lib.hpxhip_replace_if(L.I64, L.P_EQ, None, one, _vp(A), _vp(B), 8, None) == BAD
    assert lib.hpxhip_replace_if(L.I64, L.P_EQ, one, None, _vp(A), _vp(B), 8, None) == BAD


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


def _all_calls(pol, a, b):
    """name -> call with first range [a, a + 16) and second iterator b."""
    return {
        "reverse": lambda: P.reverse(pol, a, a + 16),
        "reverse_copy": lambda: P.reverse_copy(pol, a, a + 16, b),
        "rotate": lambda: P.rotate(pol, a, a + 3, a + 16),
        "rotate_copy": lambda: P.rotate_copy(pol, a, a + 3, a + 16, b),
        "swap_ranges": lambda: P.swap_ranges(pol, a, a + 16, b),
        "replace": lambda: P.replace(pol, a, a + 16, 1, 2),
        "replace_if": lambda: P.replace_if(pol, a, a + 16, F.less_than(1), 2),
        "replace_copy": lambda: P.replace_copy(pol, a, a + 16, b, 1, 2),
        "replace_copy_if": lambda: P.replace_copy_if(pol, a, a + 16, b, F.less_than(1), 2),
        "adjacent_difference": lambda: P.adjacent_difference(pol, a, a + 16, b),
    }


NAMES = list(_all_calls(None, _it(), _it()))
WITH_SECOND = ["reverse_copy", "rotate_copy", "swap_ranges", "replace_copy", "replace_copy_if", "adjacent_difference"]


def test_python_exports():
    assert len(NAMES) == 10
    for name in NAMES:
        assert callable(getattr(P, name))


@pytest.mark.parametrize("name", NAMES)
def test_python_non_policy_is_type_error(name):
    with pytest.raises(TypeError, match="execution policy"):
        _all_calls("par", _it(), _it())[name]()


@pytest.mark.parametrize("name", NAMES)
def test_python_host_policy_is_type_error(name):
    # a policy bound to something that is no hip executor
    with pytest.raises(TypeError, match="hip executors"):
        _all_calls(ex.par.on(object()), _it(), _it())[name]()


@pytest.mark.parametrize("name", WITH_SECOND)
def test_python_second_range_must_be_a_device_iterator_of_the_same_dtype(name):
    h = np.zeros(16, dtype=np.int64)
    with pytest.raises(TypeError, match="device iterators"):
        _all_calls(ex.par, _it(), h)[name]()
    with pytest.raises(TypeError, match="one dtype"):
        _all_calls(ex.par, _it(L.I64), _it(L.U64))[name]()


@pytest.mark.parametrize("name", NAMES)
def test_python_host_arrays_and_reversed_ranges(name):
    h = np.zeros(16, dtype=np.int64)
    with pytest.raises(TypeError):
        _all_calls(ex.par, h, _it())[name]()
    a = _it()
    with pytest.raises(ValueError, match="last precedes first"):
        P.reverse(ex.par, a + 8, a)
    with pytest.raises(ValueError, match="last precedes first"):
        P.rotate(ex.par, a + 8, a + 8, a)
    with pytest.raises(ValueError):
        P.rotate(ex.par, a, a + 9, a + 8)  # new_first beyond last
    with pytest.raises(ValueError):
        P.rotate_copy(ex.par, a, a + 9, a + 8, _it())


def test_python_functor_checks():
    a, b = _it(), _it()
    for bad in (F.plus, F.less, lambda x: x < 1, None, 3):
        with pytest.raises(TypeError):
            P.replace_if(ex.par, a, a + 16, bad, 2)
        with pytest.raises(TypeError):
            P.replace_copy_if(ex.par, a, a + 16, b, bad, 2)
    for bad in (F.plus, F.less_than(1), lambda x, y: x - y, 3):
        with pytest.raises(TypeError):
            P.adjacent_difference(ex.par, a, a + 16, b, bad)
    with pytest.raises(ValueError):
        P.adjacent_difference(ex.par, a, a + 16, b, F.triad_step(3.0, "float64"))


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
#include <hpx/include/parallel_reverse.hpp>
#include <hpx/include/parallel_rotate.hpp>
#include <hpx/include/parallel_swap_ranges.hpp>
#include <hpx/include/parallel_replace.hpp>
#include <hpx/include/parallel_adjacent_difference.hpp>
#include <functional>
#include <type_traits>
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using vec = hpx::compute::vector<long>;
using It = vec::iterator;
using Pair = hpx::parallel::util::tagged_pair<It, It>;
template <typename A, typename B> constexpr bool same = std::is_same<A, B>::value;
"""


def test_cxx_result_types_with_host_compiler():
    r = _compile(PROLOGUE + """
void f(vec& a, vec& b) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    auto t = ex::par(ex::task).on(exec);
    It f = a.begin(), m = a.begin() + 1, l = a.end(), d = b.begin();
    static_assert(same<decltype(hpx::parallel::reverse(p, f, l)), It>, "reverse");
    static_assert(same<decltype(hpx::reverse(t, f, l)), hpx::future<It>>, "reverse task");
    static_assert(same<decltype(hpx::parallel::reverse_copy(p, f, l, d)), Pair>, "reverse_copy");
    static_assert(same<decltype(hpx::reverse_copy(t, f, l, d)), hpx::future<Pair>>, "reverse_copy task");
    static_assert(same<decltype(hpx::parallel::rotate(p, f, m, l)), Pair>, "rotate");
    static_assert(same<decltype(hpx::rotate(t, f, m, l)), hpx::future<Pair>>, "rotate task");
    static_assert(same<decltype(hpx::parallel::rotate(p, f, m, l).begin()), It>, "tag::begin");
    static_assert(same<decltype(hpx::parallel::rotate(p, f, m, l).end()), It>, "tag::end");
    static_assert(same<decltype(hpx::parallel::rotate_copy(p, f, m, l, d)), Pair>, "rotate_copy");
    static_assert(same<decltype(hpx::parallel::rotate_copy(p, f, m, l, d).in()), It>, "tag::in");
    static_assert(same<decltype(hpx::parallel::rotate_copy(p, f, m, l, d).out()), It>, "tag::out");
    static_assert(same<decltype(hpx::rotate_copy(t, f, m, l, d)), hpx::future<Pair>>, "rotate_copy task");
    static_assert(same<decltype(hpx::parallel::swap_ranges(p, f, l, d)), It>, "swap_ranges");
    static_assert(same<decltype(hpx::swap_ranges(t, f, l, d)), hpx::future<It>>, "swap_ranges task");
    static_assert(same<decltype(hpx::parallel::replace(p, f, l, 1, 2)), It>, "replace");
    static_assert(same<decltype(hpx::replace(t, f, l, 1L, 2L)), hpx::future<It>>, "replace task");
    static_assert(same<decltype(hpx::parallel::replace_if(p, f, l, fn::less_than<long>{3}, 2)), It>, "replace_if");
    static_assert(same<decltype(hpx::replace_if(t, f, l, fn::equal_to<long>{3}, 2)), hpx::future<It>>, "task");
    static_assert(same<decltype(hpx::parallel::replace_copy(p, f, l, d, 1, 2)), Pair>, "replace_copy");
    static_assert(same<decltype(hpx::replace_copy(t, f, l, d, 1, 2)), hpx::future<Pair>>, "replace_copy task");
    static_assert(same<decltype(hpx::parallel::replace_copy_if(p, f, l, d, fn::less_than<long>{3}, 2)), Pair>,
                  "replace_copy_if");
    static_assert(same<decltype(hpx::replace_copy_if(t, f, l, d, fn::less_than<long>{3}, 2)), hpx::future<Pair>>,
                  "replace_copy_if task");
    static_assert(same<decltype(hpx::parallel::adjacent_difference(p, f, l, d)), It>, "adjacent_difference");
    static_assert(same<decltype(hpx::adjacent_difference(t, f, l, d, std::minus<long>())), hpx::future<It>>, "task");
    static_assert(same<decltype(hpx::adjacent_difference(ex::seq, f, l, d, std::plus<>())), It>, "seq");
    static_assert(same<decltype(hpx::adjacent_difference(ex::par_unseq, f, l, d, fn::maximum())), It>, "unseq");
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


def test_umbrella_header_lists_the_new_algorithms():
    r = _compile("""
#include <hpx/hpx.hpp>
#include <hpx/include/parallel_algorithm.hpp>
using It = hpx::compute::vector<int>::iterator;
It f(It a, It b, It c) {
    hpx::reverse(hpx::parallel::execution::par, a, b);
    hpx::rotate(hpx::parallel::execution::par, a, a, b);
    hpx::replace(hpx::parallel::execution::par, a, b, 1, 2);
    hpx::swap_ranges(hpx::parallel::execution::par, a, b, c);
    return hpx::adjacent_difference(hpx::parallel::execution::par, a, b, c);
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("call", [
    "hpx::parallel::replace_if(p, a.begin(), a.end(), [](long x) { return x % 3 == 0; }, 2);",
    "hpx::parallel::replace_copy_if(p, a.begin(), a.end(), b.begin(), [](long x) { return x % 3 == 0; }, 2);",
    "hpx::parallel::adjacent_difference(p, a.begin(), a.end(), b.begin(), [](long x, long y) { return x ^ y; });",
], ids=["replace_if", "replace_copy_if", "adjacent_difference"])
def test_closures_need_hipcc(call):
    r = _compile(PROLOGUE + f"""
void f(vec& a, vec& b) {{
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    {call}
}}
""")
    assert r.returncode != 0, call
    assert "compile the translation unit with hipcc" in r.stderr, r.stderr[-2000:]
