"""unique and unique_copy without a GPU: the C++ mirror compiles with the host
compiler for the mapped relations (result types included) and rejects
closures there, the Python mirror's argument checks raise before any device
call, the C ABI refuses invalid arguments, and hpxhip_scratch_bytes answers
for the new algorithm."""
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
#include <hpx/include/parallel_unique.hpp>
#include <functional>
#include <type_traits>
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using vec = hpx::compute::vector<long>;
using It = vec::iterator;
using pair2 = hpx::parallel::util::tagged_pair<It, It>;
"""


def test_mapped_relations_compile_with_host_compiler():
    r = _compile(PROLOGUE + """
void f(vec& a, vec& b) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    auto t = ex::par(ex::task).on(exec);

    pair2 r2 = hpx::parallel::unique_copy(p, a.begin(), a.end(), b.begin());
    It i = r2.in(), o = r2.out();
    r2 = hpx::parallel::unique_copy(p, a.begin(), a.end(), b.begin(), std::equal_to<long>());
    r2 = hpx::unique_copy(ex::seq, a.begin(), a.end(), a.begin(), std::equal_to<>());
    r2 = hpx::unique_copy(ex::par, a.begin() + 1, a.end(), b.begin(), fn::equal_shifted<long>{3});
    hpx::future<pair2> f2 = hpx::parallel::unique_copy(t, a.begin(), a.end(), b.begin());
    f2 = hpx::parallel::unique_copy(t, a.begin(), a.end(), b.begin(), fn::equal_shifted<long>{3});

    It e = hpx::parallel::unique(p, a.begin(), a.end());
    e = hpx::parallel::unique(p, a.begin(), a.end(), std::equal_to<long>());
    e = hpx::unique(ex::par_unseq, a.begin(), a.end(), std::equal_to<>());
    e = hpx::unique(ex::par, a.begin(), a.end(), fn::equal_shifted<long>{0});
    hpx::future<It> fe = hpx::parallel::unique(t, a.begin(), a.end());
    fe = hpx::unique(t, a.begin(), a.end(), fn::equal_shifted<long>{63});
    (void)i; (void)o; (void)e; (void)f2; (void)fe;

    static_assert(std::is_same<decltype(hpx::parallel::unique_copy(p, a.begin(), a.end(), b.begin())),
                               pair2>::value, "tagged_pair");
    static_assert(std::is_same<decltype(hpx::parallel::unique(p, a.begin(), a.end())), It>::value, "iterator");
    static_assert(std::is_same<decltype(hpx::parallel::unique_copy(t, a.begin(), a.end(), b.begin(),
                                                                   std::equal_to<>())),
                               hpx::future<pair2>>::value, "future of a tagged_pair");
    static_assert(std::is_same<decltype(hpx::parallel::unique(t, a.begin(), a.end(), fn::equal_shifted<long>{1})),
                               hpx::future<It>>::value, "future of an iterator");
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


LAMBDA = "[](long x, long y) { return x / 2 == y / 2; }"
PROJ = "[](long x) { return x / 4; }"


@pytest.mark.parametrize("call", [
    f"hpx::parallel::unique_copy(p, a.begin(), a.end(), b.begin(), {LAMBDA});",
    f"hpx::parallel::unique(p, a.begin(), a.end(), {LAMBDA});",
    f"hpx::parallel::unique_copy(p, a.begin(), a.end(), b.begin(), std::equal_to<>(), {PROJ});",
    f"hpx::parallel::unique(p, a.begin(), a.end(), std::equal_to<>(), {PROJ});",
    "hpx::parallel::unique(p, a.begin(), a.end(), fn::equal_shifted<int>{1});",
], ids=["unique_copy", "unique", "unique_copy projection", "unique projection", "relation of another type"])
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


def _calls(first, last, dest, pred=None):
    return {"unique_copy": lambda: P.unique_copy(ex.par, first, last, dest, pred),
            "unique": lambda: P.unique(ex.par, first, last, pred)}


ALL = ["unique_copy", "unique"]


@pytest.mark.parametrize("name", ALL)
def test_python_non_policy_is_type_error(name):
    a = _it()
    args = (a, a + 16, _it()) if name == "unique_copy" else (a, a + 16)
    with pytest.raises(TypeError, match="execution policy"):
        getattr(P, name)("par", *args)


@pytest.mark.parametrize("name", ALL)
def test_python_predicate_is_not_a_relation(name):
    a = _it()
    for bad in (F.less_than(3), F.equal_to(3), lambda x, y: x == y, F.plus, F.less):
        with pytest.raises(TypeError, match="not an hpx_amd functor"):
            _calls(a, a + 16, _it(), bad)[name]()


def test_python_mismatched_dtypes_are_type_errors():
    a = _it(L.I64)
    with pytest.raises(TypeError, match="source and destination dtypes differ"):
        P.unique_copy(ex.par, a, a + 16, _it(L.I32))
    with pytest.raises(TypeError, match="source and destination dtypes differ"):
        P.unique_copy(ex.par, a, a + 16, _it(L.F64), F.key_equal)


@pytest.mark.parametrize("name", ALL)
def test_python_host_arrays_are_type_errors(name):
    h = np.zeros(16, dtype=np.int64)
    with pytest.raises(TypeError, match="device iterators"):
        _calls(h, h, _it())[name]()
    if name == "unique_copy":
        a = _it()
        with pytest.raises(TypeError, match="device iterators"):
            _calls(a, a + 16, h)[name]()


@pytest.mark.parametrize("name", ALL)
def test_python_shift_on_floats_and_out_of_range(name):
    for dt in (L.F32, L.F64):
        a = _it(dt)
        with pytest.raises(TypeError, match="integer vector"):
            _calls(a, a + 16, _it(dt), F.key_equal_shifted(1))[name]()
    for dt, bad in ((L.I32, 32), (L.U32, -1), (L.I64, 64), (L.U64, 1000)):
        a = _it(dt)
        with pytest.raises(ValueError, match="outside"):
            _calls(a, a + 16, _it(dt), F.key_equal_shifted(bad))[name]()
    with pytest.raises(TypeError):
        F.key_equal_shifted(1.5)


def test_key_equal_shifted_leaves_key_compare_alone():
    assert F.key_equal == F.KeyCompare("std::equal_to")
    assert not isinstance(F.key_equal_shifted(2), F.KeyCompare)
    assert F.key_equal_shifted(2)(13, 15) and not F.key_equal_shifted(2)(13, 16)
    assert F.key_equal_shifted(63)(-1, -5) and not F.key_equal_shifted(63)(-1, 5)


def test_c_abi_invalid_arguments():
    lib = L.load()
    bufs = [(ctypes.c_int64 * 8)() for _ in range(2)]
    a, b = (ctypes.cast(x, ctypes.c_void_p) for x in bufs)
    count = ctypes.c_uint64()
    cp = ctypes.cast(ctypes.byref(count), ctypes.c_void_p)
    bad, unsupported = L.ERROR_INVALID_ARGUMENT, L.ERROR_UNSUPPORTED
    uc = lib.hpxhip_unique_copy

    def shift(s):
        return L.scalar_buf(L.I32, s)
    assert uc(L.I64, L.Q_EQUAL, None, a, b, 8, None, None, None, 0) == bad       # null count
    assert uc(L.I64, L.Q_EQUAL, None, None, b, 8, cp, None, None, 0) == bad      # null input
    assert uc(L.I64, L.Q_EQUAL, None, a, None, 8, cp, None, None, 0) == bad      # null output
    odd = ctypes.c_void_p(a.value + 4)
    assert uc(L.I64, L.Q_EQUAL, None, odd, b, 4, cp, None, None, 0) == bad       # input not element-aligned
    assert uc(L.I64, L.Q_EQUAL, None, a, odd, 4, cp, None, None, 0) == bad       # output not element-aligned
    assert uc(L.I32, L.Q_EQUAL, None, ctypes.c_void_p(a.value + 2), b, 4, cp, None, None, 0) == bad
    assert uc(L.I64, 2, None, a, b, 8, cp, None, None, 0) == bad                 # unknown rel_kind
    assert uc(L.I64, -1, None, a, b, 8, cp, None, None, 0) == bad
    assert uc(77, L.Q_EQUAL, None, a, b, 8, cp, None, None, 0) == bad            # unknown dtype
    for dt, bits in ((L.I32, 32), (L.U32, 32), (L.I64, 64), (L.U64, 64)):
        assert uc(dt, L.Q_EQUAL_SHR, shift(bits), a, b, 2, cp, None, None, 0) == bad  # a shift outside [0, bits)
        assert uc(dt, L.Q_EQUAL_SHR, shift(-1), a, b, 2, cp, None, None, 0) == bad
        assert uc(dt, L.Q_EQUAL_SHR, None, a, b, 2, cp, None, None, 0) == bad         # no shift at all
    for dt in (L.F32, L.F64):
        assert uc(dt, L.Q_EQUAL_SHR, shift(1), a, b, 2, cp, None, None, 0) == unsupported
    # scratch too small: refused before the device is touched
    need = ctypes.c_size_t()
    assert lib.hpxhip_scratch_bytes(L.ALGO_UNIQUE_COPY, L.I64, 0, 8, ctypes.byref(need)) == 0
    assert uc(L.I64, L.Q_EQUAL, None, a, b, 8, cp, None, a, need.value - 1) == bad
    assert uc(L.I64, L.Q_EQUAL_SHR, shift(3), a, a, 8, cp, None, a, 0) == bad
    assert count.value == 0  # nothing was written


@pytest.mark.parametrize("dt", [L.I32, L.U32, L.I64, L.U64, L.F32, L.F64])
def test_scratch_bytes_for_unique_copy(dt):
    lib = L.load()

    def need(algo, n):
        v = ctypes.c_size_t()
        assert lib.hpxhip_scratch_bytes(algo, dt, 0, n, ctypes.byref(v)) == 0
        return v.value
    prev = 0
    for n in (0, 1, 1000, 8192, 8193, 16385, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 33):
        u = need(L.ALGO_UNIQUE_COPY, n)
        assert u > 0 and u >= prev  # non-decreasing in n
        assert u == need(L.ALGO_PARTITION_COPY, n)  # the same tile state, an id of its own
        prev = u
    v = ctypes.c_size_t()
    assert lib.hpxhip_scratch_bytes(L.ALGO_UNIQUE_COPY + 1, dt, 0, 8, ctypes.byref(v)) == L.ERROR_INVALID_ARGUMENT
