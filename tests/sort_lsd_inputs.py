"""Inputs and the plain-numpy reference of the LSD tests of the sort
(tests/test_gpu_sort_lsd.py; pinned without a GPU by
tests/test_sort_lsd_inputs_host.py).

The onesweep LSD (sort.hip run_sort: k_sort_plan -> k_onesweep per live byte
-> k_copy_gated / k_seg_copy) is steered by the keys' ORDERED bits alone: a
byte p is sorted iff the OR and the AND of the ordered keys differ in it, the
passes ping-pong between the keys and the alternate buffer, and an odd number
of them ends in the alternate buffer (C_COPY).  So the builders here work in
the ordered-bit domain and map back to keys of the wanted type and order:
one (mask, n, seed) gives the same digits, pass by pass, for u64 / i64 / f64
and for less / greater.

The integer halves of ordered_bits / keys_from_ordered are those of
tests/sort_plan_model.py (not restated here); this module adds the floats."""
import functools

import numpy as np

import sort_plan_model as M

TILE = {"keys": 8192, "pairs": 4096}  # sort.hip tile_shape<HAS_VAL>::tile = threads * items: 512 x 16, 256 x 16
WAVE_BLOCK = 1024                     # sort_kernel.hpp k_onesweep: wbase = tile_base + wave * (TILE / WAVES)
LBB = 4                               # sort.hip tile_shape::lbb: granules a digit's thread loads per look-back step
CONST = 0xA5                          # every byte outside a mask
KEY_DTYPES = (np.uint32, np.int32, np.float32, np.uint64, np.int64, np.float64)


def utype(dt):
    return M._utype(8 * np.dtype(dt).itemsize)


def ordered_bits(a, desc=False):
    """common.hpp ordered_bits<T, DESC> for all six key types."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return M.ordered_bits(a, desc)
    U = utype(a.dtype)
    raw = a.view(U)
    sign = U(1 << (8 * a.dtype.itemsize - 1))
    u = np.where((raw & sign) != 0, ~raw, raw | sign)
    return ~u if desc else u


def keys_from_ordered(u, dt, desc=False):
    """ordered_bits<T, DESC>::inverse: the keys of type dt whose ordered bits are u."""
    dt = np.dtype(dt)
    if dt.kind != "f":
        return M.keys_from_ordered(u, dt, desc)
    U = utype(dt)
    assert u.dtype == U
    o = ~u if desc else u
    sign = U(1 << (8 * dt.itemsize - 1))
    return np.where((o & sign) != 0, o ^ sign, ~o).view(dt)


def live_bytes(a, desc=False):
    """The bytes k_sort_plan sorts: p with ((OR ^ AND) >> 8 p) & 0xff != 0
    over the ordered bits, least significant first."""
    o = ordered_bits(a, desc)
    diff = int(np.bitwise_or.reduce(o)) ^ int(np.bitwise_and.reduce(o))
    return [p for p in range(o.dtype.itemsize) if (diff >> (8 * p)) & 0xFF]


def copy_back(a, desc=False):
    """C_COPY = nl & 1: an odd number of passes ends in the alternate buffer."""
    return len(live_bytes(a, desc)) & 1


def _order(k, desc):
    return np.argsort(ordered_bits(k, desc), kind="stable")


def reference_sort(k, desc=False):
    """Stable argsort of the ordered bits (keys move as bit patterns, so NaN
    payloads survive)."""
    k = np.ascontiguousarray(k)
    return k.view(utype(k.dtype))[_order(k, desc)].view(k.dtype)


def reference_sort_by_key(k, v, desc=False):
    """Ties keep their input order in both orders, as the oracle's
    std::stable_sort on the ordered bits does."""
    k, v = np.ascontiguousarray(k), np.ascontiguousarray(v)
    idx = _order(k, desc)
    return k.view(utype(k.dtype))[idx].view(k.dtype), v.view(utype(v.dtype))[idx].view(v.dtype)


def _finish(u, dt, desc):
    k = keys_from_ordered(u, dt, desc)
    if np.dtype(dt).kind == "f":
        assert np.isfinite(k).all(), "builder keys are finite"
    k.setflags(write=False)
    return k


def _const(dt):
    """Every byte CONST."""
    return int.from_bytes(bytes([CONST]) * np.dtype(dt).itemsize, "little")


# --------------------------------------------------------------- the builders
@functools.lru_cache(maxsize=64)
def _ordered_by_mask(P, n, mask, seed):
    U = M._utype(8 * P)
    rng = np.random.default_rng(seed)
    m = max(2, n // 4)
    pool = np.zeros(m, U)
    for p in range(P):
        if p in mask:
            b = rng.integers(0, 256, m, dtype=U)
            if p == P - 1:
                b = U(1) + b % U(254)  # 1..254: see by_mask
            # the first two pool values differ in every bit of the byte, so it is live at any n >= 2
            b[1] = b[0] ^ U(0xFF)
        else:
            b = np.full(m, CONST, U)
        pool |= b << U(8 * p)
    u = pool[rng.integers(0, m, n)]
    i = rng.choice(n, 2, replace=False)
    u[i[0]], u[i[1]] = pool[0], pool[1]
    u.setflags(write=False)
    return u


def by_mask(dt, desc, n, mask, seed):
    """n >= 2 keys whose ordered bytes named by `mask` are random and whose
    other bytes are CONST: live_bytes == sorted(mask).  The keys are drawn
    from a pool of max(2, n // 4) values, so at most n // 4 keys (n >= 8) are
    without an equal partner.

    Floats stay finite: the top ordered byte is CONST (exponent bits 0100101x
    in either order) or random in 1..254 -- an all-ones exponent needs the
    top ordered byte 0x00 or 0xFF.  The integer types take the same bytes, so
    every type of a width sorts the same digits."""
    dt = np.dtype(dt)
    mask = frozenset(mask)
    assert n >= 2 and all(0 <= p < dt.itemsize for p in mask)
    return _finish(_ordered_by_mask(dt.itemsize, n, mask, seed), dt, desc)


def lone_key(dt, desc, n, pos):
    """All keys equal except the key at pos, which differs in the top ordered
    byte only -- that byte is live only if the OR / AND count sees that one
    key.  The lone key is the largest for pos in the first half and the
    smallest otherwise, so the sorted range always differs from the input."""
    dt = np.dtype(dt)
    U = utype(dt)
    u = np.full(n, _const(dt), U)
    top = 8 * (dt.itemsize - 1)
    u[pos] = (int(u[pos]) & ((1 << top) - 1)) | ((0xC3 if pos < n // 2 else 0x3C) << top)
    return _finish(u, dt, desc)


GAP_DIGIT, FILL_DIGIT = 0x5A, 0xC3


def tile_digit(t):
    """absent_digit 'one_per_tile': tile t's only digit (distinct for t < 256, not monotone)."""
    return (GAP_DIGIT + 37 * t) & 0xFF


def absent_digit(dt, desc, tiles, tile, variant="gap", seed=3):
    """tiles * tile + 3 keys with one live byte, byte 0.
    'gap': digit 0x5A occurs in tile 0 (mixed with 0xC3, 0x00 and 0xFF) and in
    the last, ragged tile (0x5A, 0xC3, 0x5A) only; every tile between holds the
    single digit 0xC3, so the look-back of 0x5A in the last tile walks over
    tiles - 1 aggregates of zero.
    'one_per_tile': tile t holds the single digit tile_digit(t)."""
    dt = np.dtype(dt)
    n = tiles * tile + 3
    d = np.full(n, FILL_DIGIT, np.int64)
    if variant == "gap":
        rng = np.random.default_rng(seed)
        d[:tile] = np.array([GAP_DIGIT, FILL_DIGIT, 0x00, 0xFF])[rng.integers(0, 4, tile)]
        d[n - 3:] = [GAP_DIGIT, FILL_DIGIT, GAP_DIGIT]
    else:
        assert variant == "one_per_tile"
        d[:] = [tile_digit(t) for t in range(tiles + 1) for _ in range(tile)][:n]
    u = (np.full(n, _const(dt) & ~0xFF, np.uint64) | d.astype(np.uint64)).astype(utype(dt))
    return _finish(u, dt, desc)


def special_patterns(dt):
    """Raw bit patterns of the float specials, each once."""
    dt = np.dtype(dt)
    assert dt.kind == "f"
    bits = 8 * dt.itemsize
    mant = np.finfo(dt).nmant
    sign, exp_all, quiet = 1 << (bits - 1), ((1 << (bits - 1 - mant)) - 1) << mant, 1 << (mant - 1)
    pos = [0, exp_all,                      # 0, Inf
           (1 << mant) - 1, 1]              # the largest and the smallest denormal
    pos += [exp_all | quiet | p for p in (0, 1, 0x12345, quiet - 1)]   # quiet NaNs
    pos += [exp_all | p for p in (1, 2, quiet >> 1, quiet - 1)]        # signalling NaNs
    fi = np.finfo(dt)
    ordinary = np.array([1.0, 3.14159, 2.5e-3, fi.max, fi.tiny, 0.5, 1.5, 1e10, 123456.0], dt).view(utype(dt))
    pos += [int(x) for x in ordinary]
    return np.array(pos + [p | sign for p in pos], utype(dt))


def specials(dt, n, seed=5):
    """The special patterns repeated to n keys, in a fixed random order."""
    pat = special_patterns(dt)
    k = np.resize(pat, n)[np.random.default_rng(seed).permutation(n)].view(np.dtype(dt))
    k.setflags(write=False)
    return k


# ------------------------------------------- hybrid-sized inputs (2^22 keys)
N_HYBRID = 1 << 22
HOT_KEYS = 30000          # over every segment capacity (the largest: 1024 x 18 = 18432)
K_CAP_KV2, K_CAP17, K_CAP16 = 4608, 9216, 18432  # sort.hip kCapKV2 (= kCap18), kCap17 (= kCapKV), kCap16


@functools.lru_cache(maxsize=4)
def hot_cell(bits, dead, n=N_HYBRID, seed=1):
    """Ordered bits: uniform keys, HOT_KEYS of them moved into one cell of the
    top 18 bits (one bucket under every hybrid form), the bytes in `dead`
    CONST.  Returns (u, cell)."""
    U = M._utype(bits)
    rng = np.random.default_rng(seed)
    u = rng.integers(0, (1 << bits) - 1, n, dtype=U, endpoint=True)
    cell = (0x1234 << 2) | 1
    pos = rng.choice(n, HOT_KEYS, replace=False)
    u[pos] = (U(cell) << U(bits - 18)) | (u[pos] & U((1 << (bits - 18)) - 1))
    for p in dead:
        u = (u & ~(U(0xFF) << U(8 * p))) | (U(CONST) << U(8 * p))
    u.setflags(write=False)
    return u, cell


@functools.lru_cache(maxsize=1)
def many_oversized(n=N_HYBRID, seed=2):
    """Ordered 64-bit keys whose byte 6 is byte 7 ^ 0x5A (byte 7 random; not
    byte 7 itself, or the keys would be in order before the last pass and a
    lost copy-back would not show), bytes 1..5 random and byte 0 CONST: the marginal histograms are uniform, but every
    bucket of every plan holds all 2^14 keys of its top byte -- 256 oversized
    buckets, more than the 64 the segmented finish keeps."""
    rng = np.random.default_rng(seed)
    top = rng.integers(0, 256, n, dtype=np.uint64)
    u = (top << np.uint64(56)) | ((top ^ np.uint64(0x5A)) << np.uint64(48)) | (rng.integers(0, 1 << 40, n, dtype=np.uint64) << np.uint64(8)) \
        | np.uint64(CONST)
    u.setflags(write=False)
    return u


def plan16(u, has_val):
    """sort.hip k_sort_plan's 16-bit branch (prefix passes on the two top
    live bytes): pairs try 512 x 9 segments (C_SEGD), then 1024 x 9; keys 512 x
    18 (C_SEGA), then 1024 x 18 with b2 = 8."""
    n, P = int(u.size), u.dtype.itemsize
    diff = int(np.bitwise_or.reduce(u)) ^ int(np.bitwise_and.reduce(u))
    live = [p for p in range(P - 1, -1, -1) if (diff >> (8 * p)) & 0xFF]
    assert len(live) >= 3
    d1 = ((u >> u.dtype.type(8 * live[0])) & u.dtype.type(0xFF)).astype(np.int64)
    d2 = ((u >> u.dtype.type(8 * live[1])) & u.dtype.type(0xFF)).astype(np.int64)
    m_top = float(np.bincount(d1, minlength=256).max())
    h2 = np.bincount(d2, minlength=256)
    tries = [(cap, b2) for cap in ((K_CAP_KV2, K_CAP17) if has_val else (K_CAP17,)) for b2 in range(1, 9)]
    if not has_val:
        tries.append((K_CAP16, 8))
    for cap, b2 in tries:
        if M.fits(m_top * float(h2.reshape(-1, 1 << (8 - b2)).sum(axis=1).max()) / n, cap):
            sizes = np.bincount((d1 << b2) | (d2 >> (8 - b2)), minlength=256 << b2)
            return {"b2": b2, "s2": 8 * live[1] + 8 - b2, "cap": cap, "oversized": int((sizes > cap).sum()),
                    "max_bucket": int(sizes.max())}
    raise AssertionError("no 16-bit plan: the input leaves the modelled branch")


def hybrid_lsd_passes(u, has_val, form):
    """The bytes the LSD of a hybrid-sized sort of ordered bits u runs over,
    under HPXHIP_SORT_HYBRID = form (18: the default; pairs always plan the
    16-bit form): every live byte when fewer than three are live (the planned
    one-segment LSD), else the live bytes under the bucket prefix
    (k_sort_fallback: 8 p < s2) of the 1..64 oversized buckets, or every live
    byte again when more buckets than that are oversized."""
    bits = 8 * u.dtype.itemsize
    diff = int(np.bitwise_or.reduce(u)) ^ int(np.bitwise_and.reduce(u))
    live = [p for p in range(bits // 8) if (diff >> (8 * p)) & 0xFF]
    if len(live) < 3:
        return live
    if form == 18 and not has_val:
        p = M.plan18(u)
        s2 = bits - 18 + 9 - p["b2"]
    else:
        p = plan16(u, has_val)
        s2 = p["s2"]
    assert p["oversized"] >= 1, "an oversized bucket sends the sort to the LSD"
    if p["oversized"] > M.K_MAX_BIG:  # more than the segmented finish keeps: the whole array, every live byte
        return live
    return [d for d in live if 8 * d < s2]


# ----------------------------------------------- the cases of the GPU tests
# Read by tests/test_gpu_sort_lsd.py and by tests/test_sort_lsd_inputs_host.py,
# which asserts every case's live bytes and parity from the same builder call.
SEED = 0x50F7
VALUE_KINDS = (None, np.uint32, np.uint64)  # keys only, 4-byte values, 8-byte values


def tile_of(vdt):
    return TILE["keys" if vdt is None else "pairs"]


def masks(P):
    """(a): none, the lowest byte, the top byte, two adjacent bytes, an odd
    non-adjacent set, every byte; 64-bit keys also five bytes with gaps."""
    m = [(), (0,), (P - 1,), (0, 1), (0, 2, P - 1), tuple(range(P))]
    return m + [(1, 3, 4, 6, 7)] if P == 8 else m


def mask_seed(mask):
    return SEED + sum(1 << p for p in mask)


def mask_id(mask):
    return "mask" + ("".join(str(p) for p in mask) or "-")


def matrix_cases():
    """(a): (key dtype, value dtype or None, desc, mask, n = 3 tiles + 5)."""
    return [(dt, vdt, desc, mask, 3 * tile_of(vdt) + 5) for dt in KEY_DTYPES for vdt in VALUE_KINDS
            for desc in (False, True) for mask in masks(np.dtype(dt).itemsize)]


EDGE_KINDS = ((np.uint64, None), (np.int32, None), (np.uint64, np.uint64), (np.uint32, np.uint32))


def edge_sizes(T):
    return [2, 3, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 2 * T, 2 * T + 1]


def edge_cases():
    """(b): (key dtype, value dtype, mask, n) at the wave and tile edges."""
    out = []
    for dt, vdt in EDGE_KINDS:
        P = np.dtype(dt).itemsize
        for mask in (tuple(range(P)), (0, 2, P - 1)):
            out += [(dt, vdt, mask, n) for n in edge_sizes(tile_of(vdt))]
    return out


# (i): (name, ordered-bits builder, key dtype); every one 2^22 keys
def hybrid_input(name):
    if name == "u64-hot":    # bytes 0 and 1 dead, 2..7 random, one 30000-key cell
        return hot_cell(64, (0, 1))[0]
    if name == "u32-hot":    # every byte random, one 30000-key cell
        return hot_cell(32, ())[0]
    if name == "u64-many":   # byte 6 a function of byte 7, byte 0 dead: 256 buckets of 2^14 keys under every plan
        return many_oversized()
    assert name == "u64-byte0"
    return _ordered_by_mask(8, N_HYBRID, frozenset({0}), SEED)


HYBRID_INPUTS = {"u64-hot": np.uint64, "u32-hot": np.uint32, "u64-many": np.uint64, "u64-byte0": np.uint64}
HYBRID_FORMS = (18, 16)  # HPXHIP_SORT_HYBRID unset (the default form) and = 16
