"""Without a GPU: every input of tests/test_gpu_sort_lsd.py has the
properties its test relies on -- the live bytes k_sort_plan will find, the
parity of their number (C_COPY), equal keys everywhere, the per-tile digit
census of the look-back inputs, the pass count of the hybrid-sized cases --
and the numpy reference the GPU tests compare with agrees bit for bit with
the oracle's sort and stable sort_by_key."""
import numpy as np
import pytest

import sort_lsd_inputs as SL
import sort_plan_model as M
from oracle import oracle as O


def name(dt):
    return "keys" if dt is None else np.dtype(dt).name


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def index_values(n, vdt=np.uint64):
    return np.arange(n, dtype=vdt)


# ----------------------------------------------------- ordered bits, inverse
@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", SL.KEY_DTYPES, ids=name)
def test_ordered_bits_round_trip_and_order(dt, desc):
    """The inverse round-trips on full-range random bits (and, for floats, on
    the specials), integers agree with sort_plan_model, and the ordered bits
    order finite values as the type's own comparison does."""
    dt = np.dtype(dt)
    U = SL.utype(dt)
    raw = np.random.default_rng(7).integers(0, (1 << (8 * dt.itemsize)) - 1, 4099, dtype=U, endpoint=True)
    pats = [raw] + ([SL.special_patterns(dt)] if dt.kind == "f" else [])
    for bits in pats:
        k = bits.view(dt)
        o = SL.ordered_bits(k, desc)
        assert o.dtype == U
        assert same_bits(SL.keys_from_ordered(o, dt, desc), k)
        assert same_bits(SL.ordered_bits(SL.keys_from_ordered(bits, dt, desc), desc), bits)
        assert np.array_equal(SL.ordered_bits(k, not desc), ~o)
        if dt.kind != "f":
            assert np.array_equal(o, M.ordered_bits(k, desc))
    k = raw.view(dt)
    k = k[np.isfinite(k)] if dt.kind == "f" else k
    o = SL.ordered_bits(k, False).astype(object)
    a, b = k[:-1], k[1:]
    assert np.array_equal(a < b, o[:-1] < o[1:])


def test_specials_hold_what_the_float_test_needs():
    for dt in (np.float32, np.float64):
        p = SL.special_patterns(dt).view(dt)
        raw = p.view(SL.utype(dt))
        quiet = 1 << (np.finfo(dt).nmant - 1)
        for neg in (False, True):
            s = np.signbit(p) == neg
            assert (s & (p == 0)).sum() == 1 and (s & np.isinf(p)).sum() == 1
            nan = s & np.isnan(p)
            assert (nan & ((raw & quiet) != 0)).sum() >= 3 and (nan & ((raw & quiet) == 0)).sum() >= 3
            den = s & (p != 0) & (np.abs(p) < np.finfo(dt).tiny)
            assert den.sum() == 2
        assert np.unique(raw).size == raw.size
        k = SL.specials(dt, SL.TILE["keys"] + 7)
        assert np.array_equal(np.unique(k.view(raw.dtype)), np.unique(raw))


# ------------------------------------------------------------ (a) the matrix
def test_matrix_live_bytes_parity_and_duplicates():
    """Every (dtype, order, mask, n) of the matrix: the live bytes are the
    mask, copy_back is its parity, and at least half the keys have an equal
    partner (at most n // 4 distinct values)."""
    cases = SL.matrix_cases()
    assert len(cases) == 3 * 2 * (3 * 6 + 3 * 7)
    odd = 0
    for dt, vdt, desc, mask, n in cases:
        assert n == 3 * SL.tile_of(vdt) + 5
        k = SL.by_mask(dt, desc, n, mask, SL.mask_seed(mask))
        assert k.dtype == np.dtype(dt) and k.size == n
        assert SL.live_bytes(k, desc) == sorted(mask), (dt, desc, mask)
        assert SL.copy_back(k, desc) == len(mask) & 1
        odd += len(mask) & 1
        o = SL.ordered_bits(k, desc)
        for p in range(o.dtype.itemsize):  # the bytes outside the mask hold the non-zero constant
            if p not in mask:
                assert (((o >> o.dtype.type(8 * p)) & o.dtype.type(0xFF)) == SL.CONST).all()
        if mask:
            _, inv, cnt = np.unique(o, return_inverse=True, return_counts=True)
            assert cnt.size <= n // 4
            assert (cnt[inv] >= 2).sum() * 2 >= n
            assert not same_bits(SL.reference_sort(k, desc), k)
        else:
            assert np.unique(o).size == 1
    assert odd == 3 * 2 * (3 * 3 + 3 * 4)  # {0}, {P-1}, {0,2,P-1}, and {1,3,4,6,7}


def test_same_digits_for_every_type_and_order():
    """One (mask, n, seed) gives the same ordered bits for every type of a
    width and for both orders."""
    for P, dts in ((4, (np.uint32, np.int32, np.float32)), (8, (np.uint64, np.int64, np.float64))):
        mask = (0, 2, P - 1)
        ref = None
        for dt in dts:
            for desc in (False, True):
                o = SL.ordered_bits(SL.by_mask(dt, desc, 12293, mask, 1), desc)
                ref = o if ref is None else ref
                assert np.array_equal(o, ref)


# ------------------------------------------------------------- (b) the edges
def test_edge_cases_live_bytes():
    for dt, vdt, mask, n in SL.edge_cases():
        k = SL.by_mask(dt, False, n, mask, SL.mask_seed(mask))
        assert k.size == n and SL.live_bytes(k) == sorted(mask), (dt, mask, n)
    T = SL.TILE["keys"]
    assert SL.edge_sizes(T) == [2, 3, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385]
    assert SL.WAVE_BLOCK * 8 == SL.TILE["keys"] and SL.WAVE_BLOCK * 4 == SL.TILE["pairs"]


# ------------------------------------------------------------- (e) lone key
@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", [np.uint64, np.float32], ids=name)
def test_lone_key(dt, desc):
    for T in SL.TILE.values():
        n = 2 * T + 5
        for pos in (0, T - 1, T, n - 1):
            k = SL.lone_key(dt, desc, n, pos)
            P = np.dtype(dt).itemsize
            assert SL.live_bytes(k, desc) == [P - 1] and SL.copy_back(k, desc) == 1
            o = SL.ordered_bits(k, desc)
            vals, cnt = np.unique(o, return_counts=True)
            assert sorted(cnt.tolist()) == [1, n - 1]
            assert o[pos] == vals[cnt == 1][0]
            r = SL.reference_sort(k, desc)
            assert not same_bits(r, k)  # a skipped pass would leave the input, which is not the answer
            where = int(np.flatnonzero(SL.ordered_bits(r, desc) == o[pos])[0])
            assert where == (n - 1 if pos < n // 2 else 0)


# ---------------------------------------------------------- (d) absent digits
@pytest.mark.parametrize("dt,kind", [(np.uint64, "keys"), (np.uint64, "pairs"), (np.uint32, "keys"),
                                      (np.uint32, "pairs")])
def test_absent_digit_census(dt, kind):
    T, tiles = SL.TILE[kind], 11
    n = tiles * T + 3
    k = SL.absent_digit(dt, False, tiles, T, "gap")
    assert k.size == n and SL.live_bytes(k) == [0]
    d = (SL.ordered_bits(k) & SL.utype(dt)(0xFF)).astype(np.int64)
    per_tile = [np.unique(d[t * T:(t + 1) * T]).tolist() for t in range(tiles + 1)]
    assert per_tile[0] == [0x00, SL.GAP_DIGIT, SL.FILL_DIGIT, 0xFF]
    assert all(p == [SL.FILL_DIGIT] for p in per_tile[1:tiles])
    assert d[tiles * T:].tolist() == [SL.GAP_DIGIT, SL.FILL_DIGIT, SL.GAP_DIGIT]
    assert tiles - 1 > 2 * SL.LBB  # tiles between the two occurrences of 0x5A

    k = SL.absent_digit(dt, False, tiles, T, "one_per_tile")
    assert k.size == n and SL.live_bytes(k) == [0]
    d = (SL.ordered_bits(k) & SL.utype(dt)(0xFF)).astype(np.int64)
    per_tile = [np.unique(d[t * T:(t + 1) * T]).tolist() for t in range(tiles + 1)]
    assert per_tile == [[SL.tile_digit(t)] for t in range(tiles + 1)]
    assert len({p[0] for p in per_tile}) == tiles + 1
    assert not same_bits(SL.reference_sort(k), k)


# ----------------------------------------------- the reference vs the oracle
def _oracle_agrees(k, desc, vdts=(np.uint32, np.uint64)):
    assert same_bits(SL.reference_sort(k, desc), O.sort(k, desc))
    for vdt in vdts:
        v = index_values(k.size, vdt)
        rk, rv = SL.reference_sort_by_key(k, v, desc)
        ok, ov = O.sort_by_key(k, v, desc)
        assert same_bits(rk, ok) and same_bits(rv, ov)


@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
@pytest.mark.parametrize("dt", SL.KEY_DTYPES, ids=name)
def test_reference_agrees_with_the_oracle_on_by_mask(dt, desc):
    n = 3 * SL.TILE["pairs"] + 5
    for mask in SL.masks(np.dtype(dt).itemsize):
        _oracle_agrees(SL.by_mask(dt, desc, n, mask, SL.mask_seed(mask)), desc)


@pytest.mark.parametrize("desc", [False, True], ids=["less", "greater"])
def test_reference_agrees_with_the_oracle_on_the_other_builders(desc):
    T = SL.TILE["pairs"]
    for dt in (np.uint64, np.float32):
        for pos in (0, T):
            _oracle_agrees(SL.lone_key(dt, desc, 2 * T + 5, pos), desc)
    for dt in (np.uint64, np.uint32):
        for variant in ("gap", "one_per_tile"):
            _oracle_agrees(SL.absent_digit(dt, desc, 11, T, variant), desc)
    for dt in (np.float32, np.float64):
        _oracle_agrees(SL.specials(dt, SL.TILE["keys"] + 7), desc)
        _oracle_agrees(SL.specials(dt, T + 7), desc)


# ------------------------------------------------- (i) the hybrid-sized cases
@pytest.mark.parametrize("case", list(SL.HYBRID_INPUTS))
def test_hybrid_inputs_run_an_odd_number_of_lsd_passes(case):
    """Whatever form plans them, the LSD that finishes these sorts runs an
    odd number of passes and so ends in the alternate buffer (k_seg_copy):
    one oversized bucket (30000 keys in one cell of the top 18 bits, which is
    one bucket under every form) with five (u64) or three (u32) live bytes
    under its prefix; 256 oversized buckets, which send the whole array
    through the LSD over its seven live bytes; or a planned one-byte LSD
    (nl = 1 < 3)."""
    u = SL.hybrid_input(case)
    assert u.size == 1 << 22 and u.dtype == SL.HYBRID_INPUTS[case]
    bits = 8 * u.dtype.itemsize
    live = SL.live_bytes(u)
    if case == "u64-byte0":
        assert live == [0]
    elif case == "u64-many":
        assert live == [1, 2, 3, 4, 5, 6, 7]
        top = np.bincount((u >> np.uint64(56)).astype(np.int64), minlength=256)
        assert top.min() > SL.K_CAP17 and np.array_equal((u >> np.uint64(56)) ^ np.uint64(0x5A), (u >> np.uint64(48)) & np.uint64(0xFF))
        low = u & np.uint64((1 << 56) - 1)  # before the top byte's pass the keys are not yet in order
        assert not np.array_equal(u[np.argsort(low, kind="stable")], np.sort(u))
    else:
        assert live == ([2, 3, 4, 5, 6, 7] if bits == 64 else [0, 1, 2, 3])
        cells = np.bincount((u >> u.dtype.type(bits - 18)).astype(np.int64), minlength=1 << 18)
        cell = SL.hot_cell(bits, (0, 1) if bits == 64 else ())[1]
        assert int(cells.argmax()) == cell and SL.HOT_KEYS <= cells[cell] < SL.HOT_KEYS + 100
        assert SL.HOT_KEYS > SL.K_CAP16 and np.delete(cells, cell).max() < 100
    for has_val in (False, True):
        for form in SL.HYBRID_FORMS:
            passes = SL.hybrid_lsd_passes(u, has_val, form)
            assert len(passes) & 1, (case, has_val, form, passes)
            if case == "u64-many":
                assert passes == live  # the whole-array fallback
            elif case != "u64-byte0":
                assert passes == ([2, 3, 4, 5, 6] if bits == 64 else [0, 1, 2])
    k = M.keys_from_ordered(u, u.dtype)
    assert same_bits(SL.reference_sort(k), O.sort(k))
    if case == "u64-byte0":  # 256 distinct keys: the values' order is all stability
        rk, rv = SL.reference_sort_by_key(k, index_values(k.size))
        ok, ov = O.sort_by_key(k, index_values(k.size))
        assert same_bits(rk, ok) and same_bits(rv, ov)
