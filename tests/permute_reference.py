"""NumPy reference of reverse, rotate, swap_ranges, replace(_if) and
adjacent_difference for the tests (not a test itself).  Every result has the
input's dtype; comparisons are bitwise (`same`), so -0.0 / 0.0 and NaN
payloads count."""
import numpy as np

from hpx_amd import _lib as L

ALL_DT = [np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]


def same(a, b) -> bool:
    """Bitwise equality of two arrays of one dtype and length."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def reverse(a):
    return np.ascontiguousarray(a[::-1])


def rotate(a, mid):
    """Left rotation: a[mid] becomes element 0."""
    return np.roll(a, -mid) if len(a) else a.copy()


def pred_mask(a, kind, arg):
    """hpxhip_pred `kind` of every element against `arg` (copy_if's meaning)."""
    arg = a.dtype.type(arg)
    with np.errstate(invalid="ignore"):
        if kind == L.P_LT:
            return a < arg
        if kind == L.P_LE:
            return a <= arg
        if kind == L.P_GT:
            return a > arg
        if kind == L.P_GE:
            return a >= arg
        if kind == L.P_EQ:
            return a == arg
        if kind == L.P_NE:
            return a != arg
        if kind == L.P_NOT_LT:
            return ~(a < arg)
        if kind == L.P_BITS:
            return (a & arg) != 0
    raise ValueError(kind)


def replace_if(a, kind, arg, new):
    """np.where keeps the bits of both sources."""
    return np.where(pred_mask(a, kind, arg), a.dtype.type(new), a).astype(a.dtype, copy=False)


def replace(a, old, new):
    return replace_if(a, L.P_EQ, old, new)


def adjacent_difference(a, kind=L.B_SUB):
    """out[0] = a[0], out[i] = op(a[i], a[i-1]) in a's own dtype (integers
    wrap; floats: one IEEE operation)."""
    out = a.copy()
    if len(a) < 2:
        return out
    x, y = a[1:], a[:-1]
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == L.B_SUB:
            out[1:] = x - y
        elif kind == L.B_ADD:
            out[1:] = x + y
        elif kind == L.B_MUL:
            out[1:] = x * y
        elif kind == L.B_MIN:
            out[1:] = np.where(y < x, y, x)
        elif kind == L.B_MAX:
            out[1:] = np.where(x < y, y, x)
        else:
            raise ValueError(kind)
    return out


def sample(dt, n, seed=0):
    """n elements of dtype dt: small values with repeats (so predicates hit),
    a few extremes (so differences wrap), signed zeros for floats."""
    rng = np.random.default_rng(seed + 1000003 * n + np.dtype(dt).num)
    dt = np.dtype(dt)
    if dt.kind == "f":
        a = rng.integers(-6, 7, n).astype(dt) / dt.type(4)
        if n > 3:
            a[rng.integers(0, n, max(1, n // 16))] = dt.type(-0.0)
            a[rng.integers(0, n, max(1, n // 16))] = dt.type(0.0)
        return a
    info = np.iinfo(dt)
    lo = -6 if info.min < 0 else 0
    a = rng.integers(lo, 13, n).astype(dt)
    if n > 3:
        a[rng.integers(0, n, max(1, n // 16))] = info.max
        a[rng.integers(0, n, max(1, n // 16))] = info.min
    return a
