"""The search family without a GPU: the C++ mirror compiles with the host
compiler for the mapped functors (result types included) and rejects closures
there, the Python mirror's argument checks raise before any device call, the C
ABI refuses invalid arguments before it touches a device, and
hpxhip_scratch_bytes answers for the two new algorithms."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from hpx_amd.compute import iterator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = ["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]


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
#include <hpx/include/parallel_all_any_none.hpp>
#include <hpx/include/parallel_count.hpp>
#include <hpx/include/parallel_equal.hpp>
#include <hpx/include/parallel_find.hpp>
#include <hpx/include/parallel_minmax.hpp>
#include <hpx/include/parallel_mismatch.hpp>
#include <functional>
#include <iterator>
#include <type_traits>
#include <utility>
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using vec = hpx::compute::vector<long>;
using It = vec::iterator;
using pair2 = std::pair<It, It>;
using diff = std::iterator_traits<It>::difference_type;
"""


def test_mapped_forms_compile_with_host_compiler():
    r = _compile(PROLOGUE + """
void f(vec& a, vec& b) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    auto t = ex::par(ex::task).on(exec);

    It i = hpx::parallel::find(p, a.begin(), a.end(), 5);
    i = hpx::find_if(ex::seq, a.begin(), a.end(), fn::less_than<long>{3});
    i = hpx::parallel::find_if_not(ex::par, a.begin() + 1, a.end(), fn::any_bits<long>{4});
    hpx::future<It> fi = hpx::parallel::find(t, a.begin(), a.end(), 5L);
    fi = hpx::find_if_not(t, a.begin(), a.end(), fn::not_less_than<long>{0});

    bool q = hpx::parallel::all_of(p, a.begin(), a.end(), fn::greater_equal<long>{0});
    q = hpx::any_of(ex::par_unseq, a.begin(), a.end(), fn::equal_to<long>{1});
    q = hpx::parallel::none_of(p, a.begin(), a.end(), fn::not_equal_to<long>{1});
    hpx::future<bool> fq = hpx::parallel::any_of(t, a.begin(), a.end(), fn::greater_than<long>{9});

    diff c = hpx::parallel::count(p, a.begin(), a.end(), 7);
    c = hpx::count_if(ex::par, a.begin(), a.end(), fn::less_equal<long>{7});
    hpx::future<diff> fc = hpx::parallel::count_if(t, a.begin(), a.end(), fn::less_equal<long>{7});

    i = hpx::parallel::min_element(p, a.begin(), a.end());
    i = hpx::max_element(p, a.begin(), a.end(), std::greater<long>());
    i = hpx::parallel::max_element(ex::seq, a.begin(), a.end(), std::less<>());
    pair2 m = hpx::parallel::minmax_element(p, a.begin(), a.end());
    m = hpx::minmax_element(p, a.begin(), a.end(), std::greater<>());
    fi = hpx::parallel::min_element(t, a.begin(), a.end(), std::less<long>());
    hpx::future<pair2> fm = hpx::parallel::minmax_element(t, a.begin(), a.end());

    q = hpx::parallel::equal(p, a.begin(), a.end(), b.begin());
    q = hpx::equal(p, a.begin(), a.end(), b.begin(), b.end());
    q = hpx::parallel::equal(p, a.begin(), a.end(), b.begin(), std::equal_to<long>());
    q = hpx::parallel::equal(p, a.begin(), a.end(), b.begin(), b.end(), std::equal_to<>());
    fq = hpx::parallel::equal(t, a.begin(), a.end(), b.begin(), b.end());
    m = hpx::parallel::mismatch(p, a.begin(), a.end(), b.begin());
    m = hpx::mismatch(p, a.begin(), a.end(), b.begin(), b.end());
    m = hpx::parallel::mismatch(p, a.begin(), a.end(), b.begin(), std::equal_to<>());
    m = hpx::parallel::mismatch(p, a.begin(), a.end(), b.begin(), b.end(), std::equal_to<long>());
    fm = hpx::parallel::mismatch(t, a.begin(), a.end(), b.begin());
    (void)i; (void)q; (void)c; (void)m; (void)fi; (void)fq; (void)fc; (void)fm;

    static_assert(std::is_same<decltype(hpx::parallel::find(p, a.begin(), a.end(), 1)), It>::value, "iterator");
    static_assert(std::is_same<decltype(hpx::parallel::count(p, a.begin(), a.end(), 1)), diff>::value,
                  "difference_type");
    static_assert(std::is_same<decltype(hpx::parallel::minmax_element(p, a.begin(), a.end())), pair2>::value, "pair");
    static_assert(std::is_same<decltype(hpx::parallel::mismatch(t, a.begin(), a.end(), b.begin())),
                               hpx::future<pair2>>::value, "future of a pair");
    static_assert(std::is_same<decltype(hpx::parallel::all_of(t, a.begin(), a.end(), fn::less_than<long>{1})),
                               hpx::future<bool>>::value, "future of a bool");
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


PRED = "[](long x) { return x % 7 == 3; }"
COMP = "[](long x, long y) { return (x & 0xff) < (y & 0xff); }"
REL = "[](long x, long y) { return x / 2 == y / 2; }"
PROJ = "[](long x) { return x / 4; }"


@pytest.mark.parametrize("call", [
    f"hpx::parallel::find_if(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::find_if_not(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::all_of(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::any_of(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::none_of(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::count_if(p, a.begin(), a.end(), {PRED});",
    f"hpx::parallel::min_element(p, a.begin(), a.end(), {COMP});",
    f"hpx::parallel::max_element(p, a.begin(), a.end(), {COMP});",
    f"hpx::parallel::minmax_element(p, a.begin(), a.end(), {COMP});",
    f"hpx::parallel::min_element(p, a.begin(), a.end(), std::less<>(), {PROJ});",
    f"hpx::parallel::equal(p, a.begin(), a.end(), b.begin(), {REL});",
    f"hpx::parallel::equal(p, a.begin(), a.end(), b.begin(), b.end(), {REL});",
    f"hpx::parallel::mismatch(p, a.begin(), a.end(), b.begin(), {REL});",
    f"hpx::parallel::mismatch(p, a.begin(), a.end(), b.begin(), b.end(), {REL});",
], ids=["find_if", "find_if_not", "all_of", "any_of", "none_of", "count_if", "min_element", "max_element",
        "minmax_element", "min_element projection", "equal", "equal four iterators", "mismatch",
        "mismatch four iterators"])
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


PRED_ALGOS = ["find_if", "find_if_not", "all_of", "any_of", "none_of", "count_if"]
VALUE_ALGOS = ["find", "count"]
COMP_ALGOS = ["min_element", "max_element", "minmax_element"]
PAIR_ALGOS = ["equal", "mismatch"]
ALL = PRED_ALGOS + VALUE_ALGOS + COMP_ALGOS + PAIR_ALGOS


def _args(name, first, last):
    if name in PRED_ALGOS:
        return (first, last, F.less_than(3))
    if name in VALUE_ALGOS:
        return (first, last, 3)
    if name in COMP_ALGOS:
        return (first, last)
    return (first, last, _it())


def test_the_names_are_exported():
    for name in ALL:
        assert callable(getattr(P, name)), name


@pytest.mark.parametrize("name", ALL)
def test_python_non_policy_is_type_error(name):
    a = _it()
    with pytest.raises(TypeError, match="execution policy"):
        getattr(P, name)("par", *_args(name, a, a + 16))


@pytest.mark.parametrize("name", ALL)
def test_python_host_arrays_are_type_errors(name):
    h = np.zeros(16, dtype=np.int64)
    with pytest.raises(TypeError, match="device iterators"):
        getattr(P, name)(ex.par, *_args(name, h, h))
    if name in PAIR_ALGOS:
        a = _it()
        with pytest.raises(TypeError, match="device iterators"):
            getattr(P, name)(ex.par, a, a + 16, h)
        with pytest.raises(TypeError, match="device iterators"):
            getattr(P, name)(ex.par, a, a + 16, _it(), h)


@pytest.mark.parametrize("name", PRED_ALGOS)
def test_python_predicate_must_be_a_functor(name):
    a = _it()
    for bad in (lambda x: x < 3, F.plus, F.less, F.key_equal, 3):
        with pytest.raises(TypeError, match="not an hpx_amd functor"):
            getattr(P, name)(ex.par, a, a + 16, bad)


@pytest.mark.parametrize("name", COMP_ALGOS)
def test_python_comparator_must_be_a_compare(name):
    a = _it()
    for bad in (lambda x, y: x < y, F.less_than(3), F.minimum, F.key_equal):
        with pytest.raises(TypeError, match="not an hpx_amd functor"):
            getattr(P, name)(ex.par, a, a + 16, bad)


@pytest.mark.parametrize("name", PAIR_ALGOS)
def test_python_mismatched_dtypes_are_type_errors(name):
    a = _it(L.I64)
    with pytest.raises(TypeError, match="dtypes differ"):
        getattr(P, name)(ex.par, a, a + 16, _it(L.I32))
    b = _it(L.F64)
    with pytest.raises(TypeError, match="dtypes differ"):
        getattr(P, name)(ex.par, a, a + 16, b, b + 16)


@pytest.mark.parametrize("name", ALL)
def test_python_reversed_range_is_value_error(name):
    a = _it()
    with pytest.raises(ValueError, match="last precedes first"):
        getattr(P, name)(ex.par, *_args(name, a + 4, a))


def test_c_abi_invalid_arguments():
    lib = L.load()
    bufs = [(ctypes.c_int64 * 8)() for _ in range(2)]
    a, b = (ctypes.cast(x, ctypes.c_void_p) for x in bufs)
    out = (ctypes.c_uint64 * 2)(77, 77)
    op = ctypes.cast(out, ctypes.c_void_p)
    bad, unsupported = L.ERROR_INVALID_ARGUMENT, L.ERROR_UNSUPPORTED
    odd = ctypes.c_void_p(a.value + 4)
    odd_out = ctypes.c_void_p(op.value + 4)
    z = L.scalar_buf(L.I64, 0)

    ff = lib.hpxhip_find_if
    assert ff(L.I64, L.P_LT, z, 0, a, 8, None, None) == bad          # null result
    assert ff(L.I64, L.P_LT, z, 0, None, 8, op, None) == bad         # null input
    assert ff(L.I64, L.P_LT, z, 1, odd, 4, op, None) == bad          # input not element-aligned
    assert ff(L.I32, L.P_LT, z, 0, ctypes.c_void_p(a.value + 2), 4, op, None) == bad
    assert ff(L.I64, L.P_LT, z, 0, a, 8, odd_out, None) == bad       # result not 8-byte aligned
    assert ff(L.I64, 8, z, 0, a, 8, op, None) == bad                 # unknown pred_kind
    assert ff(L.I64, -1, z, 0, a, 8, op, None) == bad
    assert ff(77, L.P_LT, z, 0, a, 8, op, None) == bad               # unknown dtype
    for dt in (L.F32, L.F64):
        assert ff(dt, L.P_BITS, z, 0, a, 2, op, None) == unsupported

    mm = lib.hpxhip_mismatch
    assert mm(L.I64, a, b, 8, None, None) == bad
    assert mm(L.I64, None, b, 8, op, None) == bad
    assert mm(L.I64, a, None, 8, op, None) == bad
    assert mm(L.I64, odd, b, 4, op, None) == bad
    assert mm(L.I64, a, odd, 4, op, None) == bad
    assert mm(L.I64, a, b, 8, odd_out, None) == bad
    assert mm(-3, a, b, 8, op, None) == bad

    ci = lib.hpxhip_count_if
    assert ci(L.I64, L.P_EQ, z, a, 8, None, None, None, 0) == bad
    assert ci(L.I64, L.P_EQ, z, None, 8, op, None, None, 0) == bad
    assert ci(L.I64, L.P_EQ, z, odd, 4, op, None, None, 0) == bad
    assert ci(L.I64, L.P_EQ, z, a, 8, odd_out, None, None, 0) == bad
    assert ci(L.I64, 99, z, a, 8, op, None, None, 0) == bad
    assert ci(6, L.P_EQ, z, a, 8, op, None, None, 0) == bad
    for dt in (L.F32, L.F64):
        assert ci(dt, L.P_BITS, z, a, 2, op, None, None, 0) == unsupported
    need = ctypes.c_size_t()
    assert lib.hpxhip_scratch_bytes(L.ALGO_COUNT_IF, L.I64, 0, 8, ctypes.byref(need)) == 0
    assert ci(L.I64, L.P_EQ, z, a, 8, op, None, b, need.value - 1) == bad   # scratch too small
    assert ci(L.I64, L.P_EQ, z, a, 8, op, None, b, 0) == bad

    me = lib.hpxhip_minmax_element
    assert me(L.I64, L.X_MIN, 0, a, 8, None, None, None, 0) == bad
    assert me(L.I64, L.X_MAX, 1, None, 8, op, None, None, 0) == bad
    assert me(L.I64, L.X_MINMAX, 0, odd, 4, op, None, None, 0) == bad
    assert me(L.I64, L.X_MIN, 0, a, 8, odd_out, None, None, 0) == bad
    assert me(L.I64, 3, 0, a, 8, op, None, None, 0) == bad                  # unknown which
    assert me(L.I64, -1, 0, a, 8, op, None, None, 0) == bad
    assert me(-1, L.X_MIN, 0, a, 8, op, None, None, 0) == bad
    assert lib.hpxhip_scratch_bytes(L.ALGO_MINMAX_ELEMENT, L.I64, 0, 8, ctypes.byref(need)) == 0
    assert me(L.I64, L.X_MINMAX, 0, a, 8, op, None, b, need.value - 1) == bad
    assert me(L.I64, L.X_MIN, 0, a, 8, op, None, b, 0) == bad
    assert list(out) == [77, 77]  # nothing was written


@pytest.mark.parametrize("dt", [L.I32, L.U32, L.I64, L.U64, L.F32, L.F64])
def test_scratch_bytes_for_the_new_algorithms(dt):
    lib = L.load()

    def need(algo, n):
        v = ctypes.c_size_t()
        assert lib.hpxhip_scratch_bytes(algo, dt, 0, n, ctypes.byref(v)) == 0
        return v.value
    prev_c = prev_m = 0
    for n in (0, 1, 1000, 8192, 8193, 16385, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 33):
        c, m = need(L.ALGO_COUNT_IF, n), need(L.ALGO_MINMAX_ELEMENT, n)
        assert c == need(L.ALGO_REDUCE, n)  # count_if is the reduce kernel
        blocks = max(1, -(-n // 8192))      # an upper bound: one block per 8192 elements
        assert m >= 2 * 16 * blocks and m % 256 == 0  # a 16-byte pair per block and extreme
        assert c >= prev_c and m >= prev_m  # non-decreasing in n
        prev_c, prev_m = c, m
    assert L.ALGO_COUNT_IF != L.ALGO_UNIQUE_COPY + 1  # that id stays unassigned
