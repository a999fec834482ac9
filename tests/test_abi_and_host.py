"""CPU-side checks: the C-ABI library loads and exports every entry point
include/hpxhip.h declares (no compute calls), the ctypes signature table
covers them, and the host-side API logic (policies, functors, iterators,
argument dispatch) behaves like the reference interface."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hpxhip.h")
LIB = os.path.join(ROOT, "hpx_amd", "libhpxhip.so")


def declared_symbols():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(hpxhip_\w+)\s*\(", src, re.M)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    for must in ["hpxhip_transform_reduce", "hpxhip_scan", "hpxhip_copy_if", "hpxhip_sort", "hpxhip_sort_by_key",
                 "hpxhip_transform_binary", "hpxhip_stencil_heat_step", "hpxhip_stream_add_callback"]:
        assert must in syms
    assert len(syms) >= 40


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "libhpxhip.so not built (run make lib / __graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s(hpxhip_\w+)", out))
    missing = [s for s in declared_symbols() if s not in exported]
    assert not missing, missing


def test_library_is_gfx950_code_object(tmp_path):
    """Every offload bundle in the library's .hip_fatbin targets gfx950.  The
    bundles are compressed (--offload-compress, "CCOB" v3 headers: magic,
    u16 version, u16 method, u64 total size, u64 raw size, u64 hash), so each
    is cut out by its total size and listed by clang-offload-bundler."""
    import struct
    llvm = "/opt/rocm/lib/llvm/bin"
    fb = tmp_path / "fatbin.bin"
    subprocess.run([f"{llvm}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", LIB, str(tmp_path / "lib.so")],
                   check=True, capture_output=True)
    blob = fb.read_bytes()
    if not blob.startswith(b"CCOB"):  # an uncompressed build
        assert b"gfx950" in blob
        return
    off, n = blob.find(b"CCOB"), 0
    while off >= 0:  # one bundle per object file, padded apart
        _ver, _meth, total, _raw, _h = struct.unpack_from("<HHQQQ", blob, off + 4)
        one = tmp_path / f"b{n}.bin"
        one.write_bytes(blob[off:off + total])
        r = subprocess.run([f"{llvm}/clang-offload-bundler", "--list", "--type=o", f"--input={one}"],
                           capture_output=True, text=True, check=True)
        targets = [t for t in r.stdout.split() if t.startswith("hip")]
        assert targets and all(t.endswith("gfx950") for t in targets), r.stdout
        off = blob.find(b"CCOB", off + total)
        n += 1
    assert n == 8, n  # runtime elementwise reduce scan compaction sort merge stencil


def test_ctypes_table_covers_header():
    from hpx_amd import _lib as L
    syms = set(declared_symbols()) - {"hpxhip_error_string"}
    assert syms <= set(L.SIGNATURES), sorted(syms - set(L.SIGNATURES))
    lib = L.load()
    for s in syms:
        getattr(lib, s)


def test_error_strings_and_no_device_behaviour():
    from hpx_amd import _lib as L
    lib = L.load()
    assert lib.hpxhip_abi_version() == 1
    assert b"not supported" in lib.hpxhip_error_string(L.ERROR_UNSUPPORTED)
    assert lib.hpxhip_error_string(L.ERROR_OUT_OF_MEMORY)
    # argument validation happens before any device call
    assert lib.hpxhip_fill(L.F64, None, None, 10, None) == L.ERROR_INVALID_ARGUMENT
    assert lib.hpxhip_scan(L.I64, L.PLUS, 1, 0, None, None, None, None, None, 5, None, None, 0) == L.ERROR_INVALID_ARGUMENT
    assert lib.hpxhip_fill(L.F64, None, None, 0, None) == 0  # empty range: no-op
    # strided walks: span |stride| * (n-1) * size must stay below 2^47 bytes
    import ctypes
    fake = ctypes.c_void_p(1 << 20)
    big = ctypes.c_int64(-(1 << 44))   # e.g. a wrapped unsigned stride
    assert lib.hpxhip_transform_strided(L.I64, L.I64, L.I64, L.U_IDENTITY, None, fake, big, fake, ctypes.c_int64(1),
                                        ctypes.c_uint64(10), None) == L.ERROR_INVALID_ARGUMENT
    assert lib.hpxhip_transform_binary_strided(L.I64, L.I64, L.I64, L.B_ADD, None, fake, ctypes.c_int64(1), fake,
                                               ctypes.c_int64(1), fake, big, ctypes.c_uint64(10),
                                               None) == L.ERROR_INVALID_ARGUMENT


def test_scratch_size_queries():
    import ctypes
    from hpx_amd import _lib as L
    lib = L.load()
    b = ctypes.c_size_t()
    for algo in (L.ALGO_REDUCE, L.ALGO_SCAN, L.ALGO_COPY_IF, L.ALGO_SORT):
        assert lib.hpxhip_scratch_bytes(algo, L.I64, -1, 1 << 20, ctypes.byref(b)) == 0
        assert b.value > 0
    assert lib.hpxhip_scratch_bytes(L.ALGO_SORT, L.U64, -1, 1 << 30, ctypes.byref(b)) == 0
    assert b.value >= (1 << 33)  # alternate key buffer
    assert lib.hpxhip_scratch_bytes(L.ALGO_SORT_BY_KEY, L.U64, L.U32, 1000, ctypes.byref(b)) == 0
    assert lib.hpxhip_scratch_bytes(99, L.I64, -1, 10, ctypes.byref(b)) == L.ERROR_INVALID_ARGUMENT


def test_policies_mirror_reference():
    from hpx_amd import execution as ex
    assert ex.par(ex.task).is_task and not ex.par.is_task
    p = ex.par.on("exec").with_(ex.static_chunk_size(100))
    assert p.executor == "exec" and p.parameters.chunk_size == 100
    with pytest.raises(TypeError):
        ex.par(42)
    assert ex.is_execution_policy(ex.seq) and ex.is_async_execution_policy(ex.seq(ex.task))


def test_functor_semantics():
    from hpx_amd import functional as F
    assert F.triad_step(3.0)(1.0, 2.0) == 7.0
    assert F.multiply_step(2)(5) == 10
    assert F.add_value(5)(1) == 6
    assert F.not_less_than(0)(0) and not F.not_less_than(0)(-1)
    assert F.minimum(3, 2) == 2 and F.maximum(3, 2) == 3
    with pytest.raises(TypeError):
        F.require(lambda x: x, F.Unary, "for_each")


def test_algorithms_reject_host_policies_without_device():
    from hpx_amd import execution as ex, parallel as P
    with pytest.raises(TypeError):
        P.reduce(ex.par, 1, 2)
    with pytest.raises(TypeError):
        P.reduce("not a policy", None, None)


def test_future_composition_without_gpu():
    import hpx_amd as hpx
    a = hpx.make_ready_future(2)
    b = hpx.make_ready_future(3)
    c = hpx.dataflow(lambda x, y: x * y, a, b)
    assert c.get() == 6
    assert [f.get() for f in hpx.when_all(a, b).get()] == [2, 3]
    assert a.then(lambda f: f.get() + 1).get() == 3
    e = hpx.future(thunk=lambda: 1 / 0)
    assert e.has_exception()
    with pytest.raises(ZeroDivisionError):
        e.get()


def test_generate_host_restatement_matches_splitmix_reference_values():
    from oracle import oracle as O
    # splitmix64 reference values (Vigna's splitmix64 with state 0 -> first output)
    z = O.splitmix64(np.array([0], np.uint64))[0]
    assert int(z) == 0xE220A8397B1DCDAF
