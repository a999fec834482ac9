"""The single-pass scan (scan_kernel.hpp, launched from scan.hip) for every
operator, element type, converter and launch path, and the reductions for
every operator, on inputs that stay live to the last element
(tests/scan_inputs.py, pinned by tests/test_scan_inputs_host.py).

Every comparison is bit-exact against the serial left fold of the CPU oracle:
the inputs are chosen so that floating-point results are exact in any
association.  Every scan writes into a buffer laid out as
[canaries | range | canaries], and the WHOLE buffer is compared bytewise with
the expected one, so a store outside [out, out + n) fails the test too.

Launch paths of hpxhip_scan (scan.hip):
  aligned      input and output 16-B aligned: the vector kernel;
  split        the same offset inside 16 B: a one-thread head up to a 1-KiB
               output boundary, the vector kernel behind it;
  shifted      different offsets inside 16 B: the head, then the vector
               kernel reading its input shifted across lanes (SHIFTED);
  elementwise  a pointer that is not element-aligned, or n <= 4 h + 1024:
               the 1024 x 8-round kernel with element loads and stores.

What the padding of a ragged last tile (`i < n ? conv(in[i]) : id` in k_scan)
holds cannot be observed through the scan: the padded elements lie behind
every stored element of the tile in wave, round, lane and element order, so
they feed only outputs that are not stored and the aggregate of the last
tile, which no tile reads.  The identities that do reach stored outputs are
those of the wave scans (invalid DPP source lanes), of wave_shift_right and of
the look-back's missing aggregates.
"""
import ctypes
import functools

import numpy as np
import pytest

import hpx_amd as hpx
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from hpx_amd.compute import device_error_check, dtype_code
import scan_inputs as SI
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 0x5CA7
PAD = 256        # canary elements on each side of the range (a multiple of 1 KiB)
CANARY = 0xA5    # every canary byte
OPS = {"plus": L.PLUS, "multiplies": L.MULTIPLIES, "min": L.MIN, "max": L.MAX, "bit_and": L.BIT_AND,
       "bit_or": L.BIT_OR, "bit_xor": L.BIT_XOR}
FOPS = {"plus": F.plus, "multiplies": F.multiplies, "min": F.minimum, "max": F.maximum, "bit_and": F.bit_and,
        "bit_or": F.bit_or, "bit_xor": F.bit_xor}
CONVS = {"identity": (L.U_IDENTITY, ()), "scale": (L.U_SCALE, (3,)), "square": (L.U_SQUARE, ())}
NON_PLUS = ["min", "max", "multiplies", "bit_and", "bit_or", "bit_xor"]
# path -> (input offset, output offset) in elements, input byte shift
PATHS = {"aligned": (0, 0, 0), "split": (1, 1, 0), "shifted10": (1, 0, 0), "shifted03": (0, 3, 0),
         "elementwise": (0, 0, 1)}
vp = ctypes.c_void_p


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def name(dt):
    return np.dtype(dt).name


def head_of(address, itemsize):
    """The head launch_scan_split cuts off a range whose output starts at
    address: elements to the next 16-B boundary, then to the next 1-KiB one."""
    h = (16 - address % 16) % 16 // itemsize
    v = address + h * itemsize
    return h + (1024 - v % 1024) % 1024 // itemsize


class Frame:
    """A device buffer [PAD canaries | oout | up to cap elements | PAD
    canaries], every byte CANARY, whose range starts out_byte bytes past
    element PAD + oout."""

    def __init__(self, t, dt, cap, oout=0, out_byte=0):
        self.t, self.dt = t, np.dtype(dt)
        isz = self.dt.itemsize
        self.blank = np.full((2 * PAD + oout + cap + 1) * isz, CANARY, np.uint8)
        self.start = (PAD + oout) * isz + out_byte
        self.dev = hpx.vector.from_host(self.blank.view(self.dt), t)
        self.address = self.dev.data() + self.start
        self.h = head_of(self.address, isz) if out_byte == 0 else None

    def scan(self, a, init, op, incl, ref, oin=0, in_byte=0, conv="identity", in_place=False, prefix=None,
             host_init=None, path=None):
        """hpxhip_scan of a into the frame; the whole buffer must then equal
        canaries around ref.  prefix: a value placed in device memory and
        passed as prefix_dev (host_init, a different value, goes in init)."""
        t, dt = self.t, self.dt
        isz, n, code = dt.itemsize, a.size, dtype_code(dt)
        assert a.dtype == dt and ref.dtype == dt and ref.size == n
        want = self.blank.copy()
        want[self.start:self.start + n * isz] = bits(ref)
        if in_place:
            seeded = self.blank.copy()
            seeded[self.start:self.start + n * isz] = bits(a)
            L.call("hpxhip_memcpy_async", vp(self.dev.data()), seeded.ctypes.data_as(vp), seeded.nbytes, L.H2D,
                   t.stream)
            src = self.address
        else:
            raw = np.zeros((oin + n + 2) * isz, np.uint8)
            raw[oin * isz + in_byte:oin * isz + in_byte + n * isz] = bits(a)
            d = hpx.vector.from_host(raw.view(dt), t)
            src = d.data() + oin * isz + in_byte
        if path is not None:  # the addresses really select that launch path (hpxhip_scan, launch_scan_split)
            out, split = self.address, self.h is not None and src % isz == 0 and n > 4 * self.h + 1024
            assert {"aligned": src % 16 == 0 and out % 16 == 0,
                    "split": split and src % 16 == out % 16 != 0,
                    "shifted": split and src % 16 != out % 16,
                    "elementwise": (src % 16 or out % 16) and not split}[path.rstrip("0123")], (path, src, out, n)
        pd = None
        if prefix is not None:
            pv = hpx.vector.from_host(np.array([prefix, 0], dt), t)
            pd = vp(pv.data())
        kind, scalars = CONVS[conv]
        iv = np.array(init if host_init is None else host_init, dt)[()].item()
        L.call("hpxhip_scan", code, OPS[op], 1 if incl else 0, kind, L.scalars_buf(code, scalars),
               L.scalar_buf(code, iv), pd, vp(src), vp(self.address), n, t.stream, None, 0)
        L.call("hpxhip_stream_synchronize", t.stream)
        device_error_check(t.device)
        got = bits(self.dev.to_host())
        if not np.array_equal(got, want):
            pytest.fail(self.explain(got, want, n))

    def explain(self, got, want, n):
        """Where the first differing byte lies: a canary, or an element of
        the range in the coordinates of the aligned kernel."""
        dt, isz = self.dt, self.dt.itemsize
        b = int(np.flatnonzero(got != want)[0])
        nbad = int(np.count_nonzero(got != want))
        if b < self.start or b >= self.start + n * isz:
            side = "before" if b < self.start else "after"
            return f"stray write {side} the range: byte {b - self.start} relative to out, {nbad} bytes differ"
        i = (b - self.start) // isz
        g = SI.Geometry(dt)
        msg = f"first mismatch at element {i} of {n} ({nbad} bytes differ)"
        for what, j in (("as launched aligned", i), (f"behind a head of {self.h}", i - (self.h or 0))):
            if j >= 0:
                k = j % g.E % g.W
                msg += (f"; {what}: group {j // g.E // g.group} tile {j // g.E} wave {j % g.E // g.W} "
                        f"round {k // (64 * g.V)} lane {k // g.V % 64} element {k % g.V}")
        w = want[self.start + i * isz:self.start + (i + 1) * isz].view(dt)[0]
        r = got[self.start + i * isz:self.start + (i + 1) * isz].view(dt)[0]
        return msg + f"; got {r!r}, expected {w!r}"


@functools.lru_cache(maxsize=6)
def case(op, dtname, n, incl, conv="identity", small=False, bound=20):
    """(input, init, oracle scan), computed once and shared by the tests of
    every launch path (read-only)."""
    dt = np.dtype(dtname)
    if small:
        a, init = SI.small_ints(dt, n, SEED)
    elif op == "multiplies" and dt.kind == "f":
        a, init = SI.generate(op, dt, n, SEED, bound=bound)
    else:
        a, init = SI.generate(op, dt, n, SEED)
    ref = O.scan(a, init, incl, op=op, conv=conv, scalars=CONVS[conv][1])
    a.setflags(write=False)
    ref.setflags(write=False)
    return a, init, ref


def run_path(t, op, dt, n, incl, path, **kw):
    oin, oout, in_byte = PATHS[path]
    a, init, ref = case(op, name(dt), n, incl, **kw)
    Frame(t, dt, n, oout).scan(a, init, op, incl, ref, oin=oin, in_byte=in_byte, conv=kw.get("conv", "identity"),
                               path=path)


OP_DT = [(op, dt) for op in NON_PLUS for dt in SI.dtypes_of(op)]


# ------------------------------------------------- operators x types x paths
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("op,dt", OP_DT, ids=[f"{op}-{name(dt)}" for op, dt in OP_DT])
def test_scan_operator_type_path(gpu_target, op, dt, incl, path):
    """33 tiles + 5: crosses a look-back group boundary, ragged last tile."""
    run_path(gpu_target, op, dt, SI.group_crossing_n(dt), incl, path)


@pytest.mark.parametrize("op", NON_PLUS)
def test_scan_operator_in_place(gpu_target, op):
    dt = np.int64
    n = SI.group_crossing_n(dt)
    a, init, ref = case(op, name(dt), n, True)
    Frame(gpu_target, dt, n).scan(a, init, op, True, ref, in_place=True, path="aligned")


# ---------------------------------------------------------- exact float plus
def _plus_sizes(dt):
    E = SI.Geometry(dt).E
    return {"E-1": E - 1, "E": E, "E+1": E + 1, "33E+5": 33 * E + 5, "96E+5": 96 * E + 5}


@pytest.mark.parametrize("path", ["aligned", "shifted10", "shifted03"])
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("size", ["E-1", "E", "E+1", "33E+5", "96E+5"])
@pytest.mark.parametrize("dt", SI.FLOAT_DTYPES, ids=name)
def test_scan_float_plus_exact(gpu_target, dt, size, incl, path):
    """Integers in [-3, 3] and a non-zero init: every partial sum is an exact
    integer (3 n < 2^24 at the largest float32 size, three look-back groups),
    so one dropped or duplicated element anywhere changes the bits."""
    run_path(gpu_target, "plus", dt, _plus_sizes(dt)[size], incl, path)


# ---------------------------------------------------------------- converters
@pytest.mark.parametrize("path", ["aligned", "shifted10"])
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("op", ["plus", "max"])
@pytest.mark.parametrize("dt", [np.int32, np.uint64, np.float32, np.float64], ids=name)
@pytest.mark.parametrize("conv", ["scale", "square"])
def test_transform_scan_converters(gpu_target, conv, dt, op, incl, path):
    """transform_{in,ex}clusive_scan: scale(3) and square of values in
    [-3, 3] (|image| <= 9, 9 n < 2^24 for float32)."""
    run_path(gpu_target, op, dt, SI.group_crossing_n(dt), incl, path, conv=conv, small=True)


# ------------------------------------------ the element-wise kernel, multi-tile
@pytest.mark.parametrize("in_byte,out_byte", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("op", ["plus", "min"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=name)
def test_scan_not_element_aligned(gpu_target, dt, op, incl, in_byte, out_byte):
    """Input and / or output one byte past an element boundary: no head makes
    them 16-B aligned, so the 1024 x 8-round kernel takes the whole range --
    two tiles and a ragged third."""
    n = 2 * SI.Geometry(dt).E8 + 5
    a, init, ref = case(op, name(dt), n, incl)
    Frame(gpu_target, dt, n, 0, out_byte).scan(a, init, op, incl, ref, in_byte=in_byte, path="elementwise")


# ------------------------------------------------------- head-split threshold
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("which", ["1", "h", "4h+1024", "4h+1025"])
@pytest.mark.parametrize("oin,oout", [(1, 1), (0, 1)], ids=["same-offset", "different-offset"])
@pytest.mark.parametrize("op", ["plus", "bit_and"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=name)
def test_scan_head_split_threshold(gpu_target, dt, op, oin, oout, which, incl):
    """launch_scan_split hands ranges of up to 4 h + 1024 elements to the
    element-wise kernel and splits longer ones: both sides of that switch, a
    single element, and a range that ends with the head."""
    isz = np.dtype(dt).itemsize
    frame = Frame(gpu_target, dt, 4 * (1024 // isz + 16 // isz) + 1025, oout)
    h = frame.h
    assert 0 < h <= 1024 // isz + 16 // isz
    n = {"1": 1, "h": h, "4h+1024": 4 * h + 1024, "4h+1025": 4 * h + 1025}[which]
    a, init = SI.generate(op, dt, n, SEED)
    kernel = "elementwise" if which != "4h+1025" else "split" if oin == oout else "shifted"
    frame.scan(a, init, op, incl, O.scan(a, init, incl, op=op), oin=oin, path=kernel)


# ------------------------------------------------------ SHIFTED: the full edge
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("m", ["E+V-1", "E+V", "E+V+1", "2E", "2E+V-1", "2E+V"])
@pytest.mark.parametrize("op", ["plus", "min"])
@pytest.mark.parametrize("dt,oin,oout", [(np.int64, 1, 0), (np.int32, 3, 1)], ids=["int64-1-0", "int32-3-1"])
def test_scan_shifted_full_edge(gpu_target, dt, oin, oout, op, m, incl):
    """A shifted tile is read with vector loads only if one more vector lies
    behind it (tile_base + E + V <= n): m elements behind the head put a
    complete last tile on both sides of that condition."""
    g = SI.Geometry(dt)
    E, V = g.E, g.V
    m = {"E+V-1": E + V - 1, "E+V": E + V, "E+V+1": E + V + 1, "2E": 2 * E, "2E+V-1": 2 * E + V - 1,
         "2E+V": 2 * E + V}[m]
    frame = Frame(gpu_target, dt, m + 1024, oout)
    n = frame.h + m
    assert n > 4 * frame.h + 1024  # the split applies
    a, init = SI.generate(op, dt, n, SEED)
    frame.scan(a, init, op, incl, O.scan(a, init, incl, op=op), oin=oin, path="shifted")


# ------------------------------------------------------------------ prefix_dev
@pytest.mark.parametrize("path", ["aligned", "split", "shifted10"])
@pytest.mark.parametrize("incl", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("op", ["plus", "multiplies"])
@pytest.mark.parametrize("dt", [np.int64, np.float64], ids=name)
def test_scan_prefix_dev_overrides_init(gpu_target, dt, op, incl, path):
    """prefix_dev set and init set to a different value: the scan is seeded
    with the device value -- by tile 0 of the vector kernel, or by the split
    head, whose carry then seeds the rest."""
    oin, oout, _ = PATHS[path]
    n = SI.group_crossing_n(dt)
    a, init, ref = case(op, name(dt), n, incl)
    wrong = np.dtype(dt).type(7)
    assert wrong != init
    Frame(gpu_target, dt, n, oout).scan(a, init, op, incl, ref, oin=oin, prefix=init, host_init=wrong,
                                   path=path)


# ------------------------------------------------------- reduce, live inputs
@functools.lru_cache(maxsize=4)
def reduce_case(op, dtname, n, conv):
    dt = np.dtype(dtname)
    # bound 5: the reduction tree folds up to ten sub-ranges per partial
    # (test_scan_inputs_host.py::test_float_products_stay_in_range)
    a, init = SI.generate(op, dt, n, SEED, bound=5) if (op == "multiplies" and dt.kind == "f") else \
        SI.generate(op, dt, n, SEED)
    return a, init, O.transform_reduce(a, init, op, conv, CONVS[conv][1])


# reduce for every operator; transform_reduce with scale(3) for the selecting
# ones, whose inputs stay exact and live under it
REDUCE_CASES = [(op, dt, conv) for op in ["min", "max", "bit_and", "bit_or", "multiplies"] for dt in SI.dtypes_of(op)
                for conv in (["identity", "scale"] if op in ("min", "max") else ["identity"])]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("size", ["2 blocks + 5", "40 x 16384 + 3"])
@pytest.mark.parametrize("op,dt,conv", REDUCE_CASES, ids=[f"{op}-{name(dt)}-{c}" for op, dt, c in REDUCE_CASES])
def test_reduce_live_inputs(gpu_target, op, dt, conv, size, off):
    """reduce / transform_reduce of inputs whose result is neither 0 nor the
    identity and which a spurious 0 operand changes: a block of the
    reduction is 8192 16-B vectors."""
    V = 16 // np.dtype(dt).itemsize
    n = {"2 blocks + 5": 2 * 16384 * (V // 2) + 5, "40 x 16384 + 3": 40 * 16384 + 3}[size]
    a, init, want = reduce_case(op, name(dt), n, conv)
    pol = ex.par.on(hpx.default_executor(gpu_target))
    d = hpx.vector.from_host(np.concatenate([np.zeros(off, dt), a]), gpu_target)
    if conv == "identity":
        got = P.reduce(pol, d.begin() + off, d.end(), init, FOPS[op])
    else:
        got = P.transform_reduce(pol, d.begin() + off, d.end(), init, FOPS[op], F.multiply_step(3))
    assert bits(np.array([got], dt)).tobytes() == bits(np.array([want], dt)).tobytes(), (got, want)
