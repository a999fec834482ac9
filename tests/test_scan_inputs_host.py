"""The scan input generators (tests/scan_inputs.py), pinned with the CPU oracle
alone: a GPU test is only as good as its input, so each property the GPU
tests rely on is asserted here for every (operator, dtype) at the size they
use, 33 tiles + 5.

  exactness    the oracle's native-dtype left fold equals, bit for bit, a
               fold in Python integers (wrapped to the width) or in
               np.longdouble, cast back: no rounding happens in any
               association, so the GPU tree can be compared bitwise.
  liveness     plus / multiplies / xor / min / max: every aligned
               256-element block of the inclusive output contains a change;
               and / or: the output changes at every edge position.
  sensitivity  at every edge position p: the element replaced by 0, or by
               the operator's identity where that is not 0, changes the
               output; one extra 0 operand folded in just before p changes
               the final value (min, signed / float max, and, multiplies).

How far a replaced element can show: for plus, multiplies and the bit
operators, and for a 0 that lies beyond every value (min; signed / float
max), every output from p to the end differs.  A selecting operator fed its
identity (or unsigned max fed 0) skips the element: the outputs differ from p
on -- so the element at p has to be a strict new extreme -- but only until a
later extreme takes over, which it must if the scan is to stay live.  There
the check is that the first differing index is exactly p.
"""
import numpy as np
import pytest

import scan_inputs as SI
from oracle import oracle as O

SEED = 0x5CA7
CASES = [(op, dt) for op in SI.GENERATORS for dt in SI.dtypes_of(op)]


# ------------------------------------------------------------ wide reference
def _wrap(v, dt):
    w = 8 * dt.itemsize
    v &= (1 << w) - 1
    return v - (1 << w) if dt.kind == "i" and v >> (w - 1) else v


def wide_fold(op, a, init):
    """Inclusive left fold of a from init, in Python integers wrapped to the
    width of a.dtype, or in np.longdouble; cast back to a.dtype."""
    dt = a.dtype
    if dt.kind == "f":
        uf = {"plus": np.add, "multiplies": np.multiply, "min": np.minimum, "max": np.maximum}[op]
        x = np.concatenate([[np.longdouble(init)], a.astype(np.longdouble)])
        return uf.accumulate(x)[1:].astype(dt)
    f = {"plus": lambda x, y: _wrap(x + y, dt), "multiplies": lambda x, y: _wrap(x * y, dt),
         "min": lambda x, y: y if y < x else x, "max": lambda x, y: y if x < y else x,
         "bit_and": lambda x, y: x & y, "bit_or": lambda x, y: x | y, "bit_xor": lambda x, y: x ^ y}[op]
    x = np.concatenate([np.array([int(init)], object), a.astype(object)])
    return np.frompyfunc(f, 2, 1).accumulate(x, dtype=object)[1:].astype(dt)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ------------------------------------------------------------------ checks
def is_exact(op, a, init, ref):
    return np.array_equal(bits(ref), bits(wide_fold(op, a, init)))


def is_live(op, a, init, ref):
    changed = np.concatenate([[a.dtype.type(init)], ref[:-1]]) != ref
    if op in ("bit_and", "bit_or"):
        return bool(changed[SI.edge_positions(a.dtype, a.size)].all())
    full = a.size // 256 * 256
    return bool(changed[:full].reshape(-1, 256).any(axis=1).all() and (full == a.size or changed[full:].any()))


def _selects(op, dt, value_is_identity):
    """Whether the replaced element is merely skipped (see the module docstring)."""
    if op not in ("min", "max"):
        return False
    return value_is_identity or (op == "max" and dt.kind == "u")


def replaced_shows(op, a, init, ref, p, value, value_is_identity):
    b = a.copy()
    b[p] = value
    d = O.scan(b, init, True, op=op) != ref
    if d[:p].any() or not d[p]:
        return False
    return True if _selects(op, a.dtype, value_is_identity) else bool(d[p:].all())


def spurious_zero_shows(op, a, init, ref, p):
    return O.transform_reduce(np.insert(a, p, 0), init, op) != ref[-1]


def zero_is_absorbing_or_beyond(op, dt):
    return op in ("min", "bit_and", "multiplies") or (op == "max" and dt.kind != "u")


def failures(op, a, init):
    """The names of the properties the input (a, init) does not have."""
    dt = a.dtype
    ref = O.scan(a, init, True, op=op)
    bad = []
    if not is_exact(op, a, init, ref):
        bad.append("exactness")
    if not is_live(op, a, init, ref):
        bad.append("liveness")
    ident = SI.identity(op, dt)
    for p in SI.edge_positions(dt, a.size):
        if not replaced_shows(op, a, init, ref, p, 0, ident == 0):
            bad.append(f"zero at {p}")
        if ident != 0 and not replaced_shows(op, a, init, ref, p, ident, True):
            bad.append(f"identity at {p}")
        if zero_is_absorbing_or_beyond(op, dt) and not spurious_zero_shows(op, a, init, ref, p):
            bad.append(f"spurious zero before {p}")
    return bad


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("op,dt", CASES, ids=[f"{op}-{np.dtype(dt).name}" for op, dt in CASES])
def test_generator_is_exact_live_and_sensitive(op, dt):
    n = SI.group_crossing_n(dt)
    a, init = SI.generate(op, dt, n, SEED)
    assert not np.isnan(a).any() if a.dtype.kind == "f" else True
    ref = O.scan(a, init, True, op=op)
    assert ref[-1] != 0 and ref[-1] != SI.identity(op, dt)
    assert failures(op, a, init) == []


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("bound", [20, 5])
def test_float_products_stay_in_range(dt, bound):
    """+-2^s with the running exponent inside [-bound, bound]: every
    sub-range product is within 2^(+-2 bound).  The reduction tree folds up
    to ten sub-ranges per partial (a thread's eight strided vectors, head and
    tail), so its inputs take bound = 5: 2^(+-100) is inside float32."""
    a, init = SI.generate("multiplies", dt, SI.group_crossing_n(dt), SEED, bound=bound)
    e = np.log2(np.abs(a.astype(np.float64)))
    assert set(np.unique(e)) <= {-1.0, 0.0, 1.0}
    run = np.cumsum(e)
    assert run.min() >= -bound and run.max() <= bound
    assert (a < 0).any() and (a > 0).any()


def test_small_sizes_keep_the_properties():
    """The head-split tests run the generators at a handful of elements."""
    for op, dt in [("bit_and", np.int32), ("bit_and", np.int64), ("plus", np.int32), ("min", np.int64)]:
        for n in (1, 3, 127, 1532, 2037):
            a, init = SI.generate(op, dt, n, SEED)
            assert failures(op, a, init) == [], (op, dt, n)


def test_old_small_range_input_is_dead_for_min():
    """The input of test_scan_other_ops (300001 int64 values in [-7, 7], init
    3) under min: the output is -7 from index 4 on, so almost nothing of the
    range is checked, and -7 absorbs a spurious 0.  This is why the
    generators exist."""
    a = np.random.default_rng(12).integers(-7, 7, 300001, dtype=np.int64, endpoint=True)
    ref = O.scan(a, 3, True, op="min")
    assert (ref[4:] == -7).all() and (ref[:4] != -7).all()
    bad = failures("min", a, 3)
    assert "liveness" in bad
    edges = SI.edge_positions(np.int64, a.size)
    assert all(f"spurious zero before {p}" in bad for p in edges)
    assert all(f"zero at {p}" in bad for p in edges if p >= 4)
