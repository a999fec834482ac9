"""The onesweep LSD of the sort (sort.hip: k_sort_plan -> k_onesweep per live
byte -> k_copy_gated, or as the segmented LSD -> k_seg_copy) through the C
ABI, for every key type, order, value width and set of live bytes, at the
edges of its tiles and waves, over absent digits, and for the one key that
decides a byte's liveness.  The inputs are those of tests/sort_lsd_inputs.py;
tests/test_sort_lsd_inputs_host.py proves without a GPU that each has the
live bytes, parity, duplicates and digit census its test names here.

Every sort runs in frames [256 canary elements | offset | range | 256 canary
elements] for the keys and for the values, and the WHOLE frames are compared
bytewise with canaries around the numpy reference (a stable argsort of the
ordered bits), so a stray store fails the test as a wrong key does.  A
mismatch is reported in the coordinates of k_onesweep: tile (8192 keys or
4096 pairs), wave (1024 consecutive elements), round and lane."""
import ctypes
import functools

import numpy as np
import pytest

import hpx_amd as hpx
import sort_lsd_inputs as SL
import sort_plan_model as M
from hpx_amd import _lib as L
from hpx_amd.compute import device_error_check, dtype_code

pytestmark = pytest.mark.gpu

PAD = 256       # canary elements on each side of a range
CANARY = 0x5C   # every canary byte (no builder's key or value is made of it)
vp = ctypes.c_void_p


def name(dt):
    return "keys" if dt is None else np.dtype(dt).name


def order_id(desc):
    return "greater" if desc else "less"


def raw(x):
    return np.ascontiguousarray(x).view(np.uint8)


class Frame:
    """A device buffer [PAD canaries | off elements | n elements | PAD
    canaries] of dt, every byte CANARY but the range, which holds a."""

    def __init__(self, t, a, off=0):
        self.dt, self.n = a.dtype, a.size
        isz = self.dt.itemsize
        self.blank = np.full((2 * PAD + off + self.n) * isz, CANARY, np.uint8)
        self.start = (PAD + off) * isz
        self.dev = hpx.vector.from_host(self.filled(a).view(np.uint32), t)
        self.address = self.dev.data() + self.start

    def filled(self, a):
        assert a.dtype == self.dt and a.size == self.n
        want = self.blank.copy()
        want[self.start:self.start + a.nbytes] = raw(a)
        return want

    def mismatch(self, want, what, tile):
        """None, or where the frame first differs from canaries around `want`."""
        got, exp = raw(self.dev.to_host()), self.filled(want)
        if np.array_equal(got, exp):
            return None
        isz = self.dt.itemsize
        bad = np.flatnonzero(got != exp)
        b = int(bad[0])
        if b < self.start or b >= self.start + self.n * isz:
            side = "before" if b < self.start else "after"
            return (f"{what}: a canary was overwritten {side} the range, byte {b - self.start} relative to its "
                    f"start ({bad.size} bytes differ)")
        i = (b - self.start) // isz
        nel = np.unique((bad - self.start) // isz).size
        j, k = i % tile, i % SL.WAVE_BLOCK
        U = SL.utype(self.dt)
        g = got[self.start + i * isz:self.start + (i + 1) * isz].view(U)[0]
        w = exp[self.start + i * isz:self.start + (i + 1) * isz].view(U)[0]
        return (f"{what}: first mismatch at element {i} of {self.n} (not a canary; {nel} elements differ): tile "
                f"{i // tile} wave {j // SL.WAVE_BLOCK} round {k // 64} lane {k % 64}; got bits {int(g):#x}, "
                f"expected {int(w):#x}")

    def free(self):
        self.dev.free()


def values_for(vdt, n, seed=0x7A1):
    """Full-range random bits of the value type's width."""
    vdt = np.dtype(vdt)
    U = SL.utype(vdt)
    return np.random.default_rng(seed).integers(0, (1 << (8 * vdt.itemsize)) - 1, n, dtype=U, endpoint=True).view(vdt)


def run_sort(t, k, v, desc, want_k, want_v, koff=0, voff=0, scratch=None, scratch_bytes=0, refused=None):
    """hpxhip_sort / hpxhip_sort_by_key of k (and v) inside frames; the whole
    frames must then equal canaries around want_k (want_v).  refused: the
    error status the call must return instead of sorting."""
    tile = SL.tile_of(None if v is None else v.dtype)
    fk = Frame(t, k, koff)
    fv = None if v is None else Frame(t, v, voff)
    try:
        sp = vp(scratch) if scratch else None
        try:
            if v is None:
                L.call("hpxhip_sort", dtype_code(k.dtype), vp(fk.address), k.size, 1 if desc else 0, t.stream, sp,
                       scratch_bytes)
            else:
                L.call("hpxhip_sort_by_key", dtype_code(k.dtype), dtype_code(v.dtype), vp(fk.address),
                       vp(fv.address), k.size, 1 if desc else 0, t.stream, sp, scratch_bytes)
            assert refused is None, "the call was not refused"
        except L.HpxHipError as e:
            if refused is None or e.status != refused:
                raise
        L.call("hpxhip_stream_synchronize", t.stream)
        device_error_check(t.device)
        msgs = [fk.mismatch(want_k, "keys", tile)] + ([fv.mismatch(want_v, "values", tile)] if fv else [])
        msgs = [m for m in msgs if m]
        if msgs:
            pytest.fail("; ".join(msgs))
    finally:
        fk.free()
        if fv:
            fv.free()


def check(t, k, vdt, desc, koff=0, voff=0, v=None, **kw):
    """Sort k (with random values of vdt, or with v) and compare with the reference."""
    if v is None and vdt is not None:
        v = values_for(vdt, k.size)
    if v is None:
        run_sort(t, k, None, desc, SL.reference_sort(k, desc), None, koff, **kw)
    else:
        wk, wv = SL.reference_sort_by_key(k, v, desc)
        run_sort(t, k, v, desc, wk, wv, koff, voff, **kw)


# ------------------------------------------------------------- a. the matrix
MATRIX = SL.matrix_cases()


@pytest.mark.parametrize("dt,vdt,desc,mask,n", MATRIX,
                         ids=[f"{name(dt)}-{name(vdt)}-{order_id(desc)}-{SL.mask_id(mask)}"
                              for dt, vdt, desc, mask, _ in MATRIX])
def test_lsd_matrix(gpu_target, dt, vdt, desc, mask, n):
    """Every key type x {keys, 4-byte values, 8-byte values} x order x set of
    live bytes at 3 tiles + 5: no pass (all keys equal), one pass on the
    lowest or the top byte, two adjacent passes, an odd number of passes with
    dead bytes between them (the sort ends in the alternate buffer:
    k_copy_gated for keys and values), every byte, and for 64-bit keys five
    bytes with gaps.  Three quarters of the keys have equal partners, so the
    values show whether every pass is stable."""
    check(gpu_target, SL.by_mask(dt, desc, n, mask, SL.mask_seed(mask)), vdt, desc)


@pytest.mark.parametrize("vdt", [np.float32, np.float64], ids=name)
def test_values_move_bitwise(gpu_target, vdt):
    """Float values made of NaN patterns of both signs and many payloads: the
    values are moved as bits."""
    n = 3 * SL.TILE["pairs"] + 5
    k = SL.by_mask(np.int32, False, n, (0, 2, 3), SL.mask_seed((0, 2, 3)))
    v = SL.specials(vdt, n, seed=11)
    check(gpu_target, k, vdt, False, v=v)


# ------------------------------------------------ b. tile and wave edges
EDGES = SL.edge_cases()


@pytest.mark.parametrize("dt,vdt,mask,n", EDGES,
                         ids=[f"{name(dt)}-{name(vdt)}-{SL.mask_id(mask)}-{n}" for dt, vdt, mask, n in EDGES])
def test_lsd_tile_and_wave_edges(gpu_target, dt, vdt, mask, n):
    """2 and 3 elements, a lane round (64), a wave's 1024 elements, the
    case's own tile and two tiles, each one short, exact and one over."""
    check(gpu_target, SL.by_mask(dt, False, n, mask, SL.mask_seed(mask)), vdt, False)


# ------------------------------------------------------------ c. sub-ranges
SUB_RANGES = [(dt, wv, off, vmis) for dt in (np.int32, np.int64) for wv in (False, True) for off in (1, 3)
              for vmis in ((False, True) if wv else (False,))]


@pytest.mark.parametrize("dt,with_values,off,vmis", SUB_RANGES,
                         ids=[f"{name(dt)}-{'pairs' if wv else 'keys'}-{off}"
                              f"{'-values-' + ('misaligned' if vm else 'aligned') if wv else ''}"
                              for dt, wv, off, vm in SUB_RANGES])
def test_lsd_sub_ranges(gpu_target, dt, with_values, off, vmis):
    """Ranges that start 1 and 3 elements past a 16-B boundary (the keys, and
    the values with them or not): 2 tiles + 5, every byte live, and the
    elements in front of the range are canaries like those behind it."""
    vdt = None if not with_values else (np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64)
    n = 2 * SL.tile_of(vdt) + 5
    mask = tuple(range(np.dtype(dt).itemsize))
    check(gpu_target, SL.by_mask(dt, False, n, mask, SL.mask_seed(mask)), vdt, False, koff=off,
          voff=off if vmis else 0)


# ------------------------------------------------------------- d. look-back
@pytest.mark.parametrize("with_values", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("dt", [np.uint64, np.uint32], ids=name)
@pytest.mark.parametrize("variant", ["gap", "one_per_tile"])
def test_lookback_over_absent_digits(gpu_target, variant, dt, with_values):
    """11 tiles + 3 with one live byte.  'gap': digit 0x5A occurs in tile 0
    and in the ragged last tile only, so its look-back walks over ten
    aggregates of zero -- more than two rounds of LBB = 4 granules -- before it
    finds tile 0's prefix.  'one_per_tile': every tile holds one digit of its
    own, so every look-back ends at the first tile with nothing but zeros on
    the way.  64-bit keys take their tile ids from the counter, 32-bit keys
    from blockIdx."""
    vdt = np.uint64 if with_values else None
    check(gpu_target, SL.absent_digit(dt, False, 11, SL.tile_of(vdt), variant), vdt, False)


@pytest.mark.parametrize("reverse", [False, True], ids=["sorted", "reversed"])
@pytest.mark.parametrize("with_values", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("dt", [np.uint64, np.uint32], ids=name)
def test_lsd_sorted_and_reversed_input(gpu_target, dt, with_values, reverse):
    """Every byte live, the input already sorted or sorted the other way
    round: in the top byte's pass every tile holds a few adjacent digits only."""
    vdt = np.uint64 if with_values else None
    P = np.dtype(dt).itemsize
    mask = tuple(range(P))
    k = np.sort(SL.by_mask(dt, False, 11 * SL.tile_of(vdt) + 3, mask, SL.mask_seed(mask)))
    check(gpu_target, k[::-1].copy() if reverse else k, vdt, False)


# ------------------------------------------------------ e. the liveness word
@pytest.mark.parametrize("with_values", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("desc", [False, True], ids=order_id)
@pytest.mark.parametrize("pos", ["0", "T-1", "T", "n-1"])
@pytest.mark.parametrize("dt", [np.uint64, np.float32], ids=name)
def test_lone_key_keeps_its_byte_live(gpu_target, dt, pos, desc, with_values):
    """All keys equal but one, which differs in the top byte: the byte is
    live only if the OR / AND count (k_hist) sees that key -- the first
    element, the last of a tile, the first of the next, the last of the
    ragged tile.  A byte judged dead skips the only pass and leaves the key
    where it was; the one pass that runs ends in the alternate buffer."""
    vdt = np.uint64 if with_values else None
    T = SL.tile_of(vdt)
    n = 2 * T + 5
    p = {"0": 0, "T-1": T - 1, "T": T, "n-1": n - 1}[pos]
    v = np.arange(n, dtype=np.uint64) if with_values else None
    check(gpu_target, SL.lone_key(dt, desc, n, p), vdt, desc, v=v)


# ----------------------------------------------------------------- f. floats
@pytest.mark.parametrize("with_values", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("desc", [False, True], ids=order_id)
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=name)
def test_float_specials_total_order(gpu_target, dt, desc, with_values):
    """+-0, +-Inf, denormals, quiet and signalling NaNs of both signs and
    several payloads, ordinary values, in the IEEE total order of
    ordered_bits (negative NaNs first, -0 before +0, positive NaNs last),
    compared as bits.  The values are the input index: equal bit patterns
    must keep their input order."""
    vdt = np.uint64 if with_values else None
    n = SL.tile_of(vdt) + 7
    v = np.arange(n, dtype=np.uint64) if with_values else None
    check(gpu_target, SL.specials(dt, n), vdt, desc, v=v)


# ------------------------------------------------- g. caller-owned scratch
@pytest.mark.parametrize("dt,vdt", [(np.uint64, np.uint64), (np.int32, None)], ids=["uint64-uint64", "int32-keys"])
def test_caller_scratch_of_exactly_the_queried_size(gpu_target, dt, vdt):
    """A scratch buffer of exactly hpxhip_scratch_bytes() followed by 4 KiB
    of canary: the sort is right and the canary intact; one byte less is
    refused and leaves the keys (and values) as they were."""
    t = gpu_target
    n = 3 * SL.tile_of(vdt) + 5
    mask = tuple(range(np.dtype(dt).itemsize))
    k = SL.by_mask(dt, False, n, mask, SL.mask_seed(mask))
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_SORT if vdt is None else L.ALGO_SORT_BY_KEY, dtype_code(dt),
           -1 if vdt is None else dtype_code(vdt), n, ctypes.byref(need))
    assert need.value > 0
    tail = 4096
    size = (need.value + 3) // 4 * 4 + tail
    host = np.full(size, CANARY, np.uint8)
    scratch = hpx.vector.from_host(host.view(np.uint32), t)
    try:
        check(t, k, vdt, False, scratch=scratch.data(), scratch_bytes=need.value)
        after = raw(scratch.to_host())
        stray = np.flatnonzero(after[need.value:] != CANARY)
        assert stray.size == 0, f"store {int(stray[0])} bytes past the queried scratch size ({stray.size} bytes)"
        # one byte less: an error status, and the frames hold the input as it was
        v = None if vdt is None else values_for(vdt, n)
        run_sort(t, k, v, False, k, v, scratch=scratch.data(), scratch_bytes=need.value - 1,
                 refused=L.ERROR_INVALID_ARGUMENT)
    finally:
        scratch.free()


# ------------------------------------------------------ h. the last plain LSD
@pytest.mark.parametrize("dt,vdt", [(np.uint64, None), (np.uint32, np.uint32)], ids=["uint64-keys", "uint32-uint32"])
def test_largest_plain_lsd(gpu_target, dt, vdt):
    """2^22 - 1 elements, one below the hybrid's threshold: 512 key tiles or
    1024 pair tiles, every byte live."""
    mask = tuple(range(np.dtype(dt).itemsize))
    check(gpu_target, SL.by_mask(dt, False, M.K_HYBRID_MIN - 1, mask, SL.mask_seed(mask)), vdt, False)


# ------------------------------------- i. odd pass counts at hybrid size
@functools.lru_cache(maxsize=1)
def hybrid_reference(case):
    """(keys, values, sorted keys, sorted values) of one 2^22-key input,
    shared read-only by its forms, with and without values."""
    k = M.keys_from_ordered(SL.hybrid_input(case), SL.HYBRID_INPUTS[case])
    v = values_for(np.uint64, k.size) if case != "u64-byte0" else np.arange(k.size, dtype=np.uint64)
    out = (k, v) + SL.reference_sort_by_key(k, v)
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize("form", SL.HYBRID_FORMS, ids=["default", "form16"])
@pytest.mark.parametrize("with_values", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("case", list(SL.HYBRID_INPUTS))
def test_segmented_lsd_ends_in_the_alternate_buffer(gpu_target, monkeypatch, case, with_values, form):
    """2^22 keys whose finishing LSD runs an odd number of passes under
    every form (asserted on the host,
    test_hybrid_inputs_run_an_odd_number_of_lsd_passes), so k_seg_copy<U> and
    k_seg_copy<VAL> must bring the segment back: one 30000-key bucket -- over
    every segment capacity -- with five (u64) or three (u32) live bytes under
    its prefix; 256 oversized buckets, more than the finish keeps, so the
    whole array goes through the LSD over its seven live bytes; and a planned
    LSD over one live byte (nl = 1 < 3) that runs as
    a one-segment segmented LSD.  The stable sort's keys are the plain sort's,
    so one reference serves both."""
    if form == 18:
        monkeypatch.delenv("HPXHIP_SORT_HYBRID", raising=False)
    else:
        monkeypatch.setenv("HPXHIP_SORT_HYBRID", str(form))
    k, v, wk, wv = hybrid_reference(case)
    if with_values:
        run_sort(gpu_target, k, v, False, wk, wv)
    else:
        run_sort(gpu_target, k, None, False, wk, None)
