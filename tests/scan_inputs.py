"""Inputs that keep a scan or reduction live from the first element to the last.

A scan test only sees what its input lets through.  Small random integers
make `min`, `max`, `bit_and`, `bit_or` and `multiplies` reach a constant
within a dozen elements, and that constant is absorbing: an operand that
should not be there (the 0 a padded lane or an out-of-range element supplies
where the operator's identity is not 0) leaves it unchanged.  The generators
here are built so that

  * every element changes every later output, or -- for the selecting
    operators `min` / `max` -- new extremes keep arriving to the end;
  * the result is never 0 and never the operator's identity, and no element at
    a position where the kernel changes path (`edge_positions`) is 0 or the
    identity;
  * floating-point results are exact in ANY association (small integers for
    `plus`, signed powers of two with a bounded running exponent for
    `multiplies`, plain selection for `min` / `max`), so a GPU result is
    compared bit for bit with the serial left fold.

No generator produces a NaN: `op_min` / `op_max` (`(b < a) ? b : a`) are not
associative with NaN operands, so there is no association-independent answer
to compare with.

tests/test_scan_inputs_host.py pins these properties with the CPU oracle
alone; tests/test_gpu_scan_operators.py runs the kernels on them.

Each generator is `(dt, n, seed) -> (array, init)`.
"""
import numpy as np

# Tile geometry of the scan kernel: k_scan in
# include/hpxhip/kernels/scan_kernel.hpp (tile_elems, rounds_for, kScanGroup)
# as launched by hpx_amd/csrc/scan.hip (threads_for, launch_scan):
#   aligned / shifted   8-byte types   512 threads x 16 rounds
#                       4-byte ints    512 threads x 16 rounds
#                       float32       1024 threads x 12 rounds
#   element-wise        every type    1024 threads x  8 rounds
# Each lane holds one 16-B vector (V elements) per round; a wave owns a
# contiguous block of the tile and walks it in rounds of 64 lanes.
LOOKBACK_GROUP = 32  # tiles per group of the fixed-association look-back
_SHAPES = {  # (itemsize, is float) -> (threads, rounds) of the aligned kernel
    (8, False): (512, 16), (8, True): (512, 16), (4, False): (512, 16), (4, True): (1024, 12),
}
_ELEMENTWISE_SHAPE = (1024, 8)


class Geometry:
    """V, E (aligned tile), E8 (element-wise tile), W (a wave's block of the
    aligned tile) in elements of dtype dt."""

    def __init__(self, dt):
        dt = np.dtype(dt)
        threads, rounds = _SHAPES[(dt.itemsize, dt.kind == "f")]
        self.V = 16 // dt.itemsize
        self.threads = threads
        self.E = threads * rounds * self.V
        self.E8 = _ELEMENTWISE_SHAPE[0] * _ELEMENTWISE_SHAPE[1] * self.V
        self.W = self.E // (threads // 64)
        self.group = LOOKBACK_GROUP


def edge_positions(dt, n):
    """The indices at which the aligned kernel changes lane, round, wave, tile
    or look-back group, inside [0, n), sorted."""
    g = Geometry(dt)
    V, W, E, G = g.V, g.W, g.E, g.group
    cand = {0, 1, V - 1, V, 64 * V - 1, 64 * V, W - 1, W, E - 1, E, E + 1, G * E - 1, G * E, G * E + 1, n - 1}
    return sorted(p for p in cand if 0 <= p < n)


def group_crossing_n(dt):
    """33 tiles + 5: crosses a look-back group boundary, ragged last tile."""
    return 33 * Geometry(dt).E + 5


def identity(op, dt):
    """The operator's identity as the kernels define it (common.hpp)."""
    dt = np.dtype(dt)
    if op in ("plus", "bit_or", "bit_xor"):
        return dt.type(0)
    if op == "multiplies":
        return dt.type(1)
    if op == "bit_and":
        return np.array(-1).astype(dt)[()] if dt.kind == "i" else dt.type(np.iinfo(dt).max)
    if dt.kind == "f":
        return dt.type(np.inf if op == "min" else -np.inf)
    info = np.iinfo(dt)
    return dt.type(info.max if op == "min" else info.min)


def _full_range(rng, dt, n):
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def _exact_int_limit(dt):
    return 2 ** 24 if np.dtype(dt) == np.float32 else 2 ** 53


def gen_plus(dt, n, seed):
    """Floats: integers in [-3, 3] (non-zero at the edge positions), init 2;
    3 (n + 1) below 2^24 / 2^53, so every partial sum of every sub-range is
    an exactly representable integer.  Integers: full-range random values
    (wrapping sums: every element changes every later output)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    if dt.kind != "f":
        a = _full_range(rng, dt, n)
        a[edge_positions(dt, n)] |= dt.type(1)
        return a, dt.type(_full_range(rng, dt, 1)[0] | dt.type(1))
    assert 3 * (n + 1) < _exact_int_limit(dt), "partial sums must stay exact"
    v = rng.integers(-3, 3, n, endpoint=True)
    e = np.asarray(edge_positions(dt, n))
    v[e] = np.where(v[e] == 0, 1, v[e])
    return v.astype(dt), dt.type(2)


def small_ints(dt, n, seed):
    """Integers in [-3, 3] cast to dt (wrapping for unsigned types): the
    input of the converter tests, whose scale(3) / square images stay within
    9 in magnitude (9 n below 2^24 for the float32 sizes used)."""
    dt = np.dtype(dt)
    v = np.random.default_rng(seed).integers(-3, 3, n, endpoint=True)
    if dt.kind == "f":
        assert 9 * (n + 3) < _exact_int_limit(dt)
    return v.astype(np.int64).astype(dt), (dt.type(-20) if dt.kind in "if" else dt.type(0))


def gen_bit_xor(dt, n, seed):
    """Full-range random values, non-zero at the edge positions."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    a = _full_range(rng, dt, n)
    a[edge_positions(dt, n)] |= dt.type(1)
    return a, _full_range(rng, dt, 1)[0]


def gen_multiplies(dt, n, seed, bound=20):
    """Integers: full-range random odd values.  Odd values are invertible
    mod 2^w, so every element changes every later output and the product is
    never 0; init odd and not 1; no edge element is 1.
    Floats: +-2^s, s in {-1, 0, 1}; the exponent of the running product is a
    random walk reflected into [-bound, bound], so every sub-range product is
    a power of two within 2^(+-2 bound): exact in any association.  Signs are
    random, negative at the edge positions (no edge element is 1)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    edges = np.asarray(edge_positions(dt, n))
    if dt.kind != "f":
        a = _full_range(rng, dt, n) | dt.type(1)
        a[edges] = np.where(a[edges] == 1, dt.type(3), a[edges])
        init = _full_range(rng, dt, 1)[0] | dt.type(1)
        return a, (dt.type(3) if init == 1 else init)
    free = np.cumsum(rng.integers(-1, 1, n, endpoint=True))
    # fold the free walk into [-bound, bound] (a triangle wave of period
    # 4 bound has slope +-1, so the steps stay in {-1, 0, 1})
    y = (free + bound) % (4 * bound)
    run = np.where(y > 2 * bound, 4 * bound - y, y) - bound
    assert run.min() >= -bound and run.max() <= bound
    s = np.diff(run, prepend=0)
    assert s.min() >= -1 and s.max() <= 1
    sign = rng.integers(0, 1, n, endpoint=True) * 2 - 1
    sign[edges] = -1
    return (sign * np.exp2(s.astype(np.float64))).astype(dt), dt.type(-0.5)


def gen_min(dt, n, seed):
    """Strictly positive values with a downward drift and noise wider than
    the drift: C - 3 i + U[0, 1000), init C + 500.  New minima occur
    throughout (not at every element: the noise hides most), each edge
    position holds a strict new minimum, and the result is never 0 or the
    identity.  Float types hold the same integers (below 2^24)."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    c = 3 * n + 64  # the edge positions step at most 15 below the drift
    a = c - 3 * np.arange(n, dtype=np.int64) + rng.integers(0, 1000, n)
    init = c + 500
    before = np.minimum.accumulate(np.concatenate([[init], a[:-1]]))  # min(init, a[:p])
    low = init
    for p in edge_positions(dt, n):
        low = min(low, int(before[p])) - 1
        a[p] = low
    assert a.min() > 0 and init + 1000 < _exact_int_limit(dt if dt.kind == "f" else np.float64)
    return a.astype(dt), dt.type(init)


def gen_max(dt, n, seed):
    """The mirror image of gen_min: strictly negative and rising for signed
    and float types; for unsigned types rising from 1 (1 + 3 i + U[0, 1000),
    init 1), each edge position a strict new maximum."""
    dt = np.dtype(dt)
    if dt.kind != "u":
        a, init = gen_min(dt, n, seed)
        return -a, dt.type(-init)
    rng = np.random.default_rng(seed)
    a = 1 + 3 * np.arange(n, dtype=np.int64) + rng.integers(0, 1000, n)
    init = 1
    before = np.maximum.accumulate(np.concatenate([[init], a[:-1]]))
    high = init
    for p in edge_positions(dt, n):
        high = max(high, int(before[p])) + 1
        a[p] = high
    assert a.max() <= np.iinfo(dt).max
    return a.astype(dt), dt.type(init)


def _bit_positions(dt, n, seed):
    """At most w - 1 distinct positions: the edge positions, then random fill."""
    dt = np.dtype(dt)
    w = 8 * dt.itemsize
    pos = edge_positions(dt, n)[:w - 1]
    rng = np.random.default_rng(seed)
    want = min(w - 1, n)
    taken = set(pos)
    while len(pos) < want:
        p = int(rng.integers(0, n))
        if p not in taken:
            taken.add(p)
            pos.append(p)
    bits = rng.permutation(w)[:len(pos)]
    return np.asarray(pos, np.int64), (np.uint64(1) << bits.astype(np.uint64))


def gen_bit_or(dt, n, seed):
    """init and elements 0; each chosen position (the edge positions, then
    random fill, at most w - 1) sets one distinct bit."""
    dt = np.dtype(dt)
    pos, bit = _bit_positions(dt, n, seed)
    u = np.zeros(n, np.uint64)
    u[pos] = bit
    return u.astype(np.dtype(f"u{dt.itemsize}")).view(dt), dt.type(0)


def gen_bit_and(dt, n, seed):
    """The complement: init and elements all-ones, each chosen position
    clears one distinct bit; at most w - 1 of them, so the result is never 0."""
    a, _ = gen_bit_or(dt, n, seed)
    return ~a, identity("bit_and", dt)


GENERATORS = {"plus": gen_plus, "multiplies": gen_multiplies, "min": gen_min, "max": gen_max,
              "bit_and": gen_bit_and, "bit_or": gen_bit_or, "bit_xor": gen_bit_xor}
INT_DTYPES = [np.int32, np.uint32, np.int64, np.uint64]
FLOAT_DTYPES = [np.float32, np.float64]


def dtypes_of(op):
    """The element types an operator is built for (bit operators: integers)."""
    return INT_DTYPES + ([] if op.startswith("bit_") else FLOAT_DTYPES)


def generate(op, dt, n, seed=0x5CA7, **kw):
    a, init = GENERATORS[op](np.dtype(dt), n, seed, **kw)
    assert a.dtype == np.dtype(dt) and a.size == n
    return a, init
