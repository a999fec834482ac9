"""The partition and remove families without a GPU: the C++ mirror compiles
with the host compiler for mapped predicates (result types included) and
rejects closures there, the Python mirror's argument checks raise before any
device call, the C ABI refuses invalid arguments, and hpxhip_scratch_bytes
answers for the two new algorithms."""
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
#include <hpx/include/parallel_partition.hpp>
#include <hpx/include/parallel_remove.hpp>
#include <type_traits>
namespace ex = hpx::parallel::execution;
namespace fn = hpx::compute::hip::functional;
using vec = hpx::compute::vector<long>;
using It = vec::iterator;
using tuple3 = hpx::parallel::util::tagged_tuple<It, It, It>;
using pair2 = hpx::parallel::util::tagged_pair<It, It>;
"""


def test_mapped_predicates_compile_with_host_compiler():
    r = _compile(PROLOGUE + """
void f(vec& a, vec& b, vec& c) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    auto t = ex::par(ex::task).on(exec);
    fn::less_than<long> lt{3};

    tuple3 r3 = hpx::parallel::partition_copy(p, a.begin(), a.end(), b.begin(), c.begin(), lt);
    It i = r3.in(), o1 = r3.out1(), o2 = r3.out2();
    i = r3.in1(); o1 = r3.in2(); o2 = r3.out();  // the accessors that were there stay
    r3 = hpx::partition_copy(ex::seq, a.begin(), a.end(), a.begin(), c.begin(), fn::any_bits<long>{1});
    hpx::future<tuple3> f3 = hpx::parallel::partition_copy(t, a.begin(), a.end(), b.begin(), c.begin(), lt);

    It e = hpx::parallel::stable_partition(p, a.begin(), a.end(), lt);
    e = hpx::stable_partition(ex::par, a.begin(), a.end(), fn::not_less_than<long>{0});
    e = hpx::parallel::partition(p, a.begin(), a.end(), lt);
    e = hpx::partition(ex::par_unseq, a.begin(), a.end(), lt);
    hpx::future<It> fe = hpx::parallel::stable_partition(t, a.begin(), a.end(), lt);
    fe = hpx::parallel::partition(t, a.begin(), a.end(), lt);

    pair2 r2 = hpx::parallel::remove_copy_if(p, a.begin(), a.end(), b.begin(), lt);
    i = r2.in(); o1 = r2.out();
    r2 = hpx::parallel::remove_copy(p, a.begin(), a.end(), b.begin(), 7L);
    r2 = hpx::remove_copy(ex::par, a.begin(), a.end(), a.begin(), 7);
    r2 = hpx::remove_copy_if(ex::par, a.begin(), a.end(), b.begin(), fn::equal_to<long>{1});
    hpx::future<pair2> f2 = hpx::parallel::remove_copy_if(t, a.begin(), a.end(), b.begin(), lt);
    f2 = hpx::parallel::remove_copy(t, a.begin(), a.end(), b.begin(), 7L);

    e = hpx::parallel::remove_if(p, a.begin(), a.end(), lt);
    e = hpx::parallel::remove(p, a.begin(), a.end(), 7L);
    e = hpx::remove_if(ex::par, a.begin(), a.end(), lt);
    e = hpx::remove(ex::par, a.begin(), a.end(), 7);
    fe = hpx::parallel::remove_if(t, a.begin(), a.end(), lt);
    fe = hpx::parallel::remove(t, a.begin(), a.end(), 7L);
    (void)i; (void)o1; (void)o2; (void)e; (void)f3; (void)f2;

    static_assert(std::is_same<decltype(hpx::parallel::partition_copy(p, a.begin(), a.end(), b.begin(), c.begin(),
                                                                      lt)), tuple3>::value, "tagged_tuple");
    static_assert(std::is_same<decltype(hpx::parallel::remove_copy(p, a.begin(), a.end(), b.begin(), 7L)),
                               pair2>::value, "tagged_pair");
    static_assert(std::is_same<decltype(hpx::parallel::remove(p, a.begin(), a.end(), 7L)), It>::value, "iterator");
    static_assert(std::is_same<decltype(hpx::parallel::partition(t, a.begin(), a.end(), lt)),
                               hpx::future<It>>::value, "future");
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


LAMBDA = "[](long x) { return x % 3 == 0; }"


@pytest.mark.parametrize("call", [
    f"hpx::parallel::partition_copy(p, a.begin(), a.end(), b.begin(), c.begin(), {LAMBDA});",
    f"hpx::parallel::stable_partition(p, a.begin(), a.end(), {LAMBDA});",
    f"hpx::parallel::partition(p, a.begin(), a.end(), {LAMBDA});",
    f"hpx::parallel::remove_copy_if(p, a.begin(), a.end(), b.begin(), {LAMBDA});",
    f"hpx::parallel::remove_if(p, a.begin(), a.end(), {LAMBDA});",
], ids=["partition_copy", "stable_partition", "partition", "remove_copy_if", "remove_if"])
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


PRED = F.less_than(3)


def _calls(first, last, d1, d2, pred, value=3):
    """Every algorithm of the family on the same arguments."""
    return {
        "partition_copy": lambda: P.partition_copy(ex.par, first, last, d1, d2, pred),
        "stable_partition": lambda: P.stable_partition(ex.par, first, last, pred),
        "partition": lambda: P.partition(ex.par, first, last, pred),
        "remove_copy_if": lambda: P.remove_copy_if(ex.par, first, last, d1, pred),
        "remove_if": lambda: P.remove_if(ex.par, first, last, pred),
        "remove_copy": lambda: P.remove_copy(ex.par, first, last, d1, value),
        "remove": lambda: P.remove(ex.par, first, last, value),
    }


WITH_PRED = ["partition_copy", "stable_partition", "partition", "remove_copy_if", "remove_if"]
ALL = WITH_PRED + ["remove_copy", "remove"]


@pytest.mark.parametrize("name", ALL)
def test_python_non_policy_is_type_error(name):
    a = _it()
    fn = getattr(P, name)
    args = {"partition_copy": (a, a + 16, _it(), _it(), PRED), "remove_copy_if": (a, a + 16, _it(), PRED),
            "remove_copy": (a, a + 16, _it(), 3), "remove": (a, a + 16, 3)}.get(name, (a, a + 16, PRED))
    with pytest.raises(TypeError, match="execution policy"):
        fn("par", *args)


@pytest.mark.parametrize("name", WITH_PRED)
def test_python_non_functor_predicate_is_type_error(name):
    a = _it()
    with pytest.raises(TypeError, match="not an hpx_amd functor"):
        _calls(a, a + 16, _it(), _it(), lambda x: x < 3)[name]()
    with pytest.raises(TypeError, match="not an hpx_amd functor"):
        _calls(a, a + 16, _it(), _it(), F.plus)[name]()  # a binary operator, not a predicate


@pytest.mark.parametrize("name", ["partition_copy", "remove_copy_if", "remove_copy"])
def test_python_mismatched_dtypes_are_type_errors(name):
    a = _it(L.I64)
    with pytest.raises(TypeError, match="source and destination dtypes differ"):
        _calls(a, a + 16, _it(L.I32), _it(L.I64), PRED)[name]()
    if name == "partition_copy":
        with pytest.raises(TypeError, match="source and destination dtypes differ"):
            _calls(a, a + 16, _it(L.I64), _it(L.F64), PRED)[name]()


@pytest.mark.parametrize("name", ALL)
def test_python_host_arrays_are_type_errors(name):
    h = np.zeros(16, dtype=np.int64)
    with pytest.raises(TypeError, match="device iterators"):
        _calls(h, h, _it(), _it(), PRED)[name]()
    if name in ("partition_copy", "remove_copy_if", "remove_copy"):
        a = _it()
        with pytest.raises(TypeError, match="device iterators"):
            _calls(a, a + 16, h, _it(), PRED)[name]()
    if name == "partition_copy":
        a = _it()
        with pytest.raises(TypeError, match="device iterators"):
            _calls(a, a + 16, _it(), h, PRED)[name]()


def test_python_same_destination_twice_is_value_error():
    a, d = _it(), _it()
    with pytest.raises(ValueError, match="must not be the same range"):
        P.partition_copy(ex.par, a, a + 16, d, d, PRED)


def test_c_abi_invalid_arguments():
    lib = L.load()
    bufs = [(ctypes.c_int64 * 8)() for _ in range(3)]
    a, b, c = (ctypes.cast(x, ctypes.c_void_p) for x in bufs)
    count = ctypes.c_uint64()
    cp = ctypes.cast(ctypes.byref(count), ctypes.c_void_p)
    arg = L.scalar_buf(L.I64, 3)
    bad = L.ERROR_INVALID_ARGUMENT
    pc = lib.hpxhip_partition_copy
    assert pc(L.I64, L.P_LT, arg, a, b, c, 8, None, None, None, 0) == bad      # null count
    assert pc(L.I64, L.P_LT, arg, a, None, None, 8, cp, None, None, 0) == bad  # both outputs null
    assert pc(L.I64, L.P_LT, arg, a, b, b, 8, cp, None, None, 0) == bad        # out_true == out_false
    assert pc(L.I64, L.P_LT, arg, a, a, a, 8, cp, None, None, 0) == bad        # both outputs the input
    assert pc(L.I64, L.P_LT, arg, None, b, c, 8, cp, None, None, 0) == bad     # null input
    sp = lib.hpxhip_stable_partition
    assert sp(L.I64, L.P_LT, arg, a, 8, None, None, None, 0) == bad
    assert sp(L.I64, L.P_LT, arg, None, 8, cp, None, None, 0) == bad


@pytest.mark.parametrize("dt", [L.I32, L.U32, L.I64, L.U64, L.F32, L.F64])
def test_scratch_bytes_for_the_new_algorithms(dt):
    lib = L.load()

    def need(algo, n):
        v = ctypes.c_size_t()
        assert lib.hpxhip_scratch_bytes(algo, dt, 0, n, ctypes.byref(v)) == 0
        return v.value
    size = L.DTYPE_SIZE[dt]
    prev = (0, 0)
    for n in (0, 1, 1000, 8192, 8193, 16385, 1 << 20, (1 << 20) + 1, 1 << 30, 1 << 33):
        pc, st = need(L.ALGO_PARTITION_COPY, n), need(L.ALGO_STABLE_PARTITION, n)
        assert pc > 0
        assert st >= pc + n * size  # the tile state plus n elements
        assert pc >= prev[0] and st >= prev[1]  # non-decreasing in n
        prev = (pc, st)
