"""Host restatement of the sort planner's 18-bit branch, and the inputs of
the padded-pass edge tests.

The keys-only sort plans itself on the device (sort.hip k_sort_plan) and
offers no read-back of the plan, so a test cannot ask which path an input
took.  This module restates, in plain numpy, the part of the planner that
decides it -- the default form (HPXHIP_SORT_HYBRID unset: mode 18), keys
only, 2^22 <= n < 2^32, the two top bytes live and at least three live
bytes:

* thist / xhist: the histograms of the top 9 bits and of the 9-bit field
  under them (k_hist_tiles);
* joint[field >> 6][top9] (8 field regions x 512 digits, read as float);
* mtop = max thist, mg[b2] = the largest group of 2^(9 - b2) field bins;
* per field width b2 = 1..9: est = mtop * mg[b2] / n; the first b2 with
  fits(est, 4608) (est + 5 sqrt(est) <= 4608) is planned, except that a b2
  whose joint histogram shows more than kMaxBig = 64 cells over the segment
  (jover) is skipped (`futile`);
* cap = min(4608, (int(est + 7 sqrt(est) + 1) + 63) & ~63) and the padded
  second pass iff (512 << b2) * cap <= pad_keys = min(n + n/4 + 4608,
  2^18 * 4608) (make_layout).

plan18() takes the keys' ORDERED bits (ordered_bits(): sign flip for signed
keys, complement for std::greater) and returns the plan with the exact
bucket sizes, so a test can state -- and tests/test_sort_plan_model_host.py
asserts without a GPU -- which kernels its input reaches: the padded pass or
the look-back pass, buckets of 0, 1 and 2 keys, a slot overflow (a bucket
over cap: the look-back fallback), buckets over the 4608-key segment (the
oversized-bucket finish).

The builders below work in the ordered-bit domain and map back to keys of
the wanted type and order (keys_from_ordered), so one (n, width, seed) gives
the same buckets for u64 / i64 and for less / greater."""
import functools
import math

import numpy as np

K_CAP18 = 4608          # sort.hip kCap18 = kPadSlotMax: 512 threads x 9 keys
K_MAX_BIG = 64          # sort_kernel.hpp kMaxBig
K_MAX_BUCKETS = 1 << 18
K_HYBRID_MIN = 1 << 22


def _utype(bits):
    return np.uint64 if bits == 64 else np.uint32


def ordered_bits(h, desc=False):
    """common.hpp ordered_bits<T, DESC> for integer keys."""
    h = np.ascontiguousarray(h)
    assert h.dtype.kind in "iu" and h.dtype.itemsize in (4, 8)
    bits = 8 * h.dtype.itemsize
    U = _utype(bits)
    u = h.view(U).copy()
    if h.dtype.kind == "i":
        u ^= U(1 << (bits - 1))
    return ~u if desc else u


def keys_from_ordered(u, dt, desc=False):
    """ordered_bits<T, DESC>::inverse: the keys of type dt whose ordered bits are u."""
    dt = np.dtype(dt)
    bits = 8 * dt.itemsize
    U = _utype(bits)
    assert u.dtype == U
    k = ~u if desc else u.copy()
    if dt.kind == "i":
        k ^= U(1 << (bits - 1))
    return k.view(dt)


def fits(est, cap):
    return est + 5.0 * math.sqrt(est) <= cap


def plan18(u, est_scale=1.0):
    """The plan of sort.hip k_sort_plan's 18-bit branch for ordered bits u.
    est_scale multiplies every bucket estimate (the host test's margin probe)."""
    n = int(u.size)
    bits = 8 * u.dtype.itemsize
    passes = bits // 8
    assert u.dtype == _utype(bits)
    assert K_HYBRID_MIN <= n < (1 << 32), "takes_pre18: a hybrid-sized sort with 32-bit offsets"
    diff = int(np.bitwise_or.reduce(u)) ^ int(np.bitwise_and.reduce(u))
    live = [p for p in range(passes - 1, -1, -1) if (diff >> (8 * p)) & 0xFF]
    assert len(live) >= 3 and live[0] == passes - 1 and live[1] == passes - 2, "top two bytes live, nl >= 3"

    # cnt[top9][field]: everything the planner reads is a marginal of it
    cell = (u >> u.dtype.type(bits - 18)).astype(np.int64)
    cnt = np.bincount(cell, minlength=1 << 18).reshape(512, 512)
    thist = cnt.sum(axis=1)
    xhist = cnt.sum(axis=0)
    joint = cnt.reshape(512, 8, 64).sum(axis=2).T.astype(np.float32).astype(np.float64)  # [region][top9]
    mtop = float(thist.max())
    dn = float(n)
    pad_keys = min(n + n // 4 + K_CAP18, K_MAX_BUCKETS * K_CAP18)

    futile = False
    for b2 in range(1, 10):
        g = 1 << (9 - b2)
        mg = float(xhist.reshape(-1, g).sum(axis=1).max())
        est = mtop * mg / dn * est_scale
        if b2 <= 3:
            r = 1 << (3 - b2)
            jover = int((joint.reshape(8 // r, r, 512).sum(axis=1) > float(K_CAP18)).sum())
        else:
            jover = int((joint > float(K_CAP18) * float(1 << (b2 - 3))).sum())
        if not fits(est, K_CAP18):
            continue
        if jover > K_MAX_BIG:
            futile = True
            continue
        nb = 512 << b2
        cap = min(K_CAP18, (int(est + 7.0 * math.sqrt(est) + 1.0) + 63) & ~63)
        sizes = cnt.reshape(512, 1 << b2, g).sum(axis=2).ravel()  # bucket = top9 << b2 | field >> (9 - b2)
        s2 = bits - 18 + 9 - b2
        return {
            "n": n, "bits": bits, "b2": b2, "est": est, "cap": cap, "nb": nb, "pad_keys": pad_keys,
            "slots": nb * cap, "padded": nb * cap <= pad_keys, "sizes": sizes,
            "max_bucket": int(sizes.max()),
            "overflow": bool((sizes > cap).any()),
            "oversized": int((sizes > K_CAP18).sum()),
            "fit_margin": K_CAP18 - (est + 5.0 * math.sqrt(est)),
            "top_single": (diff & ((1 << s2) - 1)).bit_length(),
            "skipped_futile": futile,
        }
    raise AssertionError("no field width fits: the input leaves the modelled 18-bit branch")


def census(plan):
    """Ids of the buckets of one and two keys, and the number of empty ones."""
    s = plan["sizes"]
    return {"empty": int((s == 0).sum()), "one": np.flatnonzero(s == 1).tolist(),
            "two": np.flatnonzero(s == 2).tolist()}


def bucket_id(plan, key_bits):
    """Bucket of one ordered key under the plan."""
    bits, b2 = plan["bits"], plan["b2"]
    return ((key_bits >> (bits - 9)) << b2) | ((key_bits >> (bits - 18 + 9 - b2)) & ((1 << b2) - 1))


# ------------------------------------------------------------------ inputs
# All return ordered bits (uint64 / uint32); keys_from_ordered maps them to
# the key type and order of a test case.  functools.cache: the GPU tests and
# the host test share one copy per (n, bits, seed) and leave it unchanged.
EMPTIED6 = (0, 1, 255, 256, 300, 511)


def _uniform(rng, n, bits):
    return rng.integers(0, (1 << bits) - 1, n, dtype=_utype(bits), endpoint=True)


def _empty_digits(rng, u, bits, digits):
    """Move every key whose top-9 digit is in `digits` to a random other digit."""
    U = u.dtype.type
    sh = U(bits - 9)
    allowed = np.setdiff1d(np.arange(512), np.asarray(digits)).astype(u.dtype)
    sel = np.isin(u >> sh, np.asarray(digits, dtype=u.dtype))
    low = U((1 << (bits - 9)) - 1)
    u[sel] = (allowed[rng.integers(0, allowed.size, int(sel.sum()))] << sh) | (u[sel] & low)


@functools.cache
def sparse_padded(n, bits, seed, extra=0):
    """Case (a) (and, with `extra`, case (b)): uniform keys with the top-9
    digits EMPTIED6 emptied, then planted, at random positions:
      key 0 and the all-ones key (first / last bucket: one key each, sorted
      positions 0 and n - 1), two keys of digit 255 differing in bit 0 only and
      two equal keys of digit 256 (two buckets of two keys), two keys of digit
      300 in different halves of the field (two more buckets of one key).
    A whole digit is empty but for the planted keys, so the planted buckets
    are what they are for every field width b2.  extra > 0: that many more
    keys in one (top-9 digit, 4-bit field) cell -- its bucket overflows its
    slot.  Returns (u, planted) with planted = dict of the planted ordered keys."""
    rng = np.random.default_rng(seed)
    U = _utype(bits)
    u = _uniform(rng, n, bits)
    _empty_digits(rng, u, bits, EMPTIED6)
    pos = rng.choice(n, 8 + extra, replace=False)
    top = bits - 9
    low = lambda: int(rng.integers(0, 1 << (top - 1)))  # noqa: E731  (bits under the field's top bit)
    p255 = (255 << top) | (low() & ~1)
    p256 = (256 << top) | low()
    p300 = (300 << top) | low()
    planted = {"zero": 0, "ones": (1 << bits) - 1, "pair255": (p255, p255 | 1), "pair256": (p256, p256),
               "split300": (p300, p300 | (1 << (top - 1)))}
    vals = [planted["zero"], planted["ones"], *planted["pair255"], *planted["pair256"], *planted["split300"]]
    if extra:
        allowed = np.setdiff1d(np.arange(512), np.asarray(EMPTIED6))
        cell = (int(allowed[rng.integers(0, allowed.size)]) << 4) | int(rng.integers(0, 16))
        planted["cell"] = cell
        u[pos[8:]] = U(cell << (bits - 13)) | rng.integers(0, 1 << (bits - 13), extra, dtype=U)
    u[pos[:8]] = np.array(vals, dtype=U)
    u.setflags(write=False)
    return u, planted


@functools.cache
def sparse16_padded(n, bits, seed):
    """Case (a), second variant: 16 top-9 digits (0, 511 and 14 drawn ones)
    emptied, each then given ONE key with a random field: 16 buckets of one
    key.  Returns (u, the 16 planted ordered keys)."""
    rng = np.random.default_rng(seed)
    U = _utype(bits)
    u = _uniform(rng, n, bits)
    digits = np.concatenate(([0, 511], rng.choice(np.arange(1, 511), 14, replace=False)))
    _empty_digits(rng, u, bits, digits)
    keys = [(int(d) << (bits - 9)) | int(rng.integers(0, 1 << (bits - 9))) for d in digits]
    u[rng.choice(n, 16, replace=False)] = np.array(keys, dtype=U)
    u.setflags(write=False)
    return u, tuple(keys)


@functools.cache
def sparse_unpadded(n, bits, seed):
    """Case (c): uniform ordered keys in [0, 0.8 * 2^bits) plus the all-ones
    key.  A fifth of the top-9 digits is empty, which raises the largest
    digit's share and with it the slot estimate past the padded pass's
    budget: the 18-bit form with the look-back pass and k_bucket_bounds."""
    rng = np.random.default_rng(seed)
    U = _utype(bits)
    u = rng.integers(0, (8 << bits) // 10, n, dtype=U)
    u[int(rng.integers(0, n))] = U((1 << bits) - 1)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=1)  # 48 M keys: one width held at a time
def thin_field_part(n, bits, seed, part=9, keep=40):
    """Case (d): uniform keys, then field part `part` of 32 (the top 5 bits of
    the 9-bit field) reduced to `keep` keys; the others move to a random
    other part and keep their lower bits.  With b2 = 5 a tile of the padded
    pass that starts in part 8 reaches part 10, whose keys -- two parts past
    the tile's first key -- take k_pad_scatter's one-by-one branch."""
    rng = np.random.default_rng(seed)
    U = _utype(bits)
    u = _uniform(rng, n, bits)
    sh = bits - 14  # the field's top 5 bits
    idx = np.flatnonzero(((u >> U(sh)) & U(31)) == U(part))
    move = idx[rng.permutation(idx.size)[keep:]]
    others = np.setdiff1d(np.arange(32), [part]).astype(U)
    u[move] = (u[move] & ~U(31 << sh)) | (others[rng.integers(0, 31, move.size)] << U(sh))
    u.setflags(write=False)
    return u


@functools.cache
def uniform(n, bits, seed):
    u = _uniform(np.random.default_rng(seed), n, bits)
    u.setflags(write=False)
    return u


def bits_of(built):
    """The ordered bits of a builder's result (some return (u, planted))."""
    return built[0] if isinstance(built, tuple) else built


@functools.cache
def plan_of(builder, args):
    """plan18 of the input of a (builder, args) case, computed once per input."""
    return plan18(bits_of(builder(*args)))


# The inputs of tests/test_gpu_sort_padded_edges.py, as (builder, args): the
# GPU tests and tests/test_sort_plan_model_host.py read the same lists, so
# every GPU case's path is asserted on the host from the same builder and seed.
N_SMALL, N_WIDE, N_THIN = 1 << 22, 3 << 22, 48 << 20
CASES_A = [(sparse_padded, (n, bits, 1)) for n in (N_SMALL, N_WIDE) for bits in (64, 32)]
CASES_A16 = [(sparse16_padded, (n, bits, 1)) for n in (N_SMALL, N_WIDE) for bits in (64, 32)]
# (b): the seeds whose cell lands in a bucket that the 1500 extra keys also
# take over the 4608-key segment (the host test asserts it)
CASES_B = [(sparse_padded, (N_WIDE, 64, 3, 1500)), (sparse_padded, (N_WIDE, 32, 4, 1500))]
CASES_C = [(sparse_unpadded, (N_SMALL, bits, 1)) for bits in (64, 32)]
CASES_D = [(thin_field_part, (N_THIN, bits, 1)) for bits in (64, 32)]


def cases_e(bits):
    """(e): four sorts on one scratch; the first two plan different b2 / nb."""
    first = (sparse_padded, (N_SMALL, bits, 1))
    return [first, (sparse_padded, (N_WIDE, bits, 1)), (uniform, (N_SMALL, bits, 1)), first]


def case_id(case):
    builder, args = case
    return builder.__name__ + "-" + "-".join(str(a) for a in args)
