"""reduce_by_key without a GPU: the C++ mirror compiles with the host
compiler for the std:: functors and rejects closures there, the Python
mirror's argument checks raise before any device call, and the C ABI refuses
a null count."""
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
#include <hpx/include/parallel_reduce.hpp>
#include <functional>
#include <utility>
namespace ex = hpx::parallel::execution;
using kvec = hpx::compute::vector<long>;
using vvec = hpx::compute::vector<double>;
"""


def test_std_functors_compile_with_host_compiler():
    r = _compile(PROLOGUE + """
void f(kvec& k, vvec& v, kvec& ko, vvec& vo) {
    hpx::compute::hip::default_executor exec;
    auto p = ex::par.on(exec);
    std::pair<kvec::iterator, vvec::iterator> r =
        hpx::parallel::reduce_by_key(p, k.begin(), k.end(), v.begin(), ko.begin(), vo.begin(),
                                     std::equal_to<long>(), std::plus<double>());
    r = hpx::parallel::reduce_by_key(ex::seq, k.begin(), k.end(), v.begin(), k.begin(), v.begin());
    r = hpx::reduce_by_key(ex::par, k.begin(), k.end(), v.begin(), ko.begin(), vo.begin(), std::equal_to<>(),
                           std::multiplies<>());
    hpx::future<std::pair<kvec::iterator, vvec::iterator>> fut =
        hpx::parallel::reduce_by_key(ex::par(ex::task).on(exec), k.begin(), k.end(), v.begin(), ko.begin(),
                                     vo.begin());
    (void)fut;
}
""")
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.mark.parametrize("call", [
    "hpx::parallel::reduce_by_key(p, k.begin(), k.end(), v.begin(), ko.begin(), vo.begin(), std::equal_to<>(), "
    "[](double a, double b) { return a + b; });",
    "hpx::parallel::reduce_by_key(p, k.begin(), k.end(), v.begin(), ko.begin(), vo.begin(), "
    "[](long a, long b) { return a / 4 == b / 4; }, std::plus<>());",
], ids=["func", "comp"])
def test_closures_need_hipcc(call):
    r = _compile(PROLOGUE + f"""
void f(kvec& k, vvec& v, kvec& ko, vvec& vo) {{
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


def _its(kdt=L.I64, vdt=L.I64, kodt=None, vodt=None):
    vs = [_NoDeviceVector(d) for d in (kdt, vdt, kdt if kodt is None else kodt, vdt if vodt is None else vodt)]
    k, v, ko, vo = (iterator(x, 0) for x in vs)
    return k, k + 16, v, ko, vo


def test_python_non_policy_is_type_error():
    with pytest.raises(TypeError, match="execution policy"):
        P.reduce_by_key("par", *_its())


def test_python_mismatched_dtypes_are_type_errors():
    with pytest.raises(TypeError, match="key input and output dtypes differ"):
        P.reduce_by_key(ex.par, *_its(kodt=L.I32))
    with pytest.raises(TypeError, match="value input and output dtypes differ"):
        P.reduce_by_key(ex.par, *_its(vodt=L.F64))


def test_python_unknown_comparator_is_type_error():
    with pytest.raises(TypeError):
        P.reduce_by_key(ex.par, *_its(), lambda a, b: a == b)
    with pytest.raises(TypeError):
        P.reduce_by_key(ex.par, *_its(), F.equal_to(3))  # the copy_if predicate, not a key comparator
    with pytest.raises(TypeError):
        P.reduce_by_key(ex.par, *_its(), F.key_equal, lambda a, b: a + b)
    with pytest.raises(TypeError):
        P.reduce_by_key(ex.par, np.zeros(4), np.zeros(4), *_its()[2:])  # host ranges


def test_c_abi_null_count_is_invalid_argument():
    lib = L.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.hpxhip_reduce_by_key(L.I64, L.I64, L.PLUS, p, p, p, p, 8, None, None, None, 0) == \
        L.ERROR_INVALID_ARGUMENT
    count = ctypes.c_uint64()
    cp = ctypes.cast(ctypes.byref(count), ctypes.c_void_p)
    assert lib.hpxhip_reduce_by_key(L.I64, L.I64, L.PLUS, None, p, p, p, 8, cp, None, None, 0) == \
        L.ERROR_INVALID_ARGUMENT
    assert lib.hpxhip_reduce_by_key(L.I64, L.I64, L.PLUS, p, p, p, None, 8, cp, None, None, 0) == \
        L.ERROR_INVALID_ARGUMENT
    need = ctypes.c_size_t()
    assert lib.hpxhip_scratch_bytes(L.ALGO_REDUCE_BY_KEY, L.I64, L.F64, 1 << 20, ctypes.byref(need)) == 0
    assert need.value > 0
