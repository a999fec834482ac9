"""Host reference for the set operations (set_union, set_intersection,
set_difference, set_symmetric_difference, includes) with the device's key
order: vectorised numpy over the ordered-bits view of the keys (integers as
std::less, floats in IEEE total order, descending inverted -- ordered_bits in
include/hpxhip/kernels/common.hpp).

The rank rule (std::set_* on multisets): for a value v with cntA / cntB
equivalent elements in range 1 / 2 and an element's rank k inside its own
range's run of v,

    union                 range 1: always       range 2: k >= cntA
    intersection          range 1: k < cntB     range 2: never
    difference            range 1: k >= cntB    range 2: never
    symmetric difference  range 1: k >= cntB    range 2: k >= cntA

and the kept elements leave in the order of the stable merge (range 1 first
on ties).  tests/test_set_operations_host.py pins this against a literal
two-pointer transcription of the std loops.
"""
import numpy as np

UNION, INTERSECTION, DIFFERENCE, SYMMETRIC_DIFFERENCE = range(4)
OPS = {"set_union": UNION, "set_intersection": INTERSECTION, "set_difference": DIFFERENCE,
       "set_symmetric_difference": SYMMETRIC_DIFFERENCE}


def ordered_bits(a, descending=False):
    """Unsigned keys whose < is the device's key order on a."""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)
    sign = u.dtype.type(1 << (8 * a.dtype.itemsize - 1))
    if a.dtype.kind == "f":
        k = np.where(u & sign, ~u, u | sign)
    elif a.dtype.kind == "i":
        k = u ^ sign
    else:
        k = u.copy()
    return ~k if descending else k


def sort_keys(a, descending=False):
    """a sorted in the device's key order (bitwise: -0.0 before +0.0, NaNs at
    the ends by sign and payload)."""
    a = np.ascontiguousarray(a)
    return a[np.argsort(ordered_bits(a, descending), kind="stable")]


def keep_masks(op, a, b, descending=False):
    """-> (keep_a, keep_b, pos_a, pos_b): which elements of the sorted ranges
    the operation keeps, and every element's place in the stable merge."""
    ka, kb = ordered_bits(a, descending), ordered_bits(b, descending)
    lb_aa, ub_aa = np.searchsorted(ka, ka, "left"), np.searchsorted(ka, ka, "right")
    lb_ba, ub_ba = np.searchsorted(kb, ka, "left"), np.searchsorted(kb, ka, "right")   # a's values in b
    lb_bb, ub_bb = np.searchsorted(kb, kb, "left"), np.searchsorted(kb, kb, "right")
    lb_ab, ub_ab = np.searchsorted(ka, kb, "left"), np.searchsorted(ka, kb, "right")   # b's values in a
    rank_a, cnt_b = np.arange(a.size) - lb_aa, ub_ba - lb_ba
    rank_b, cnt_a = np.arange(b.size) - lb_bb, ub_ab - lb_ab
    del ub_aa, ub_bb
    if op == UNION:
        keep_a, keep_b = np.ones(a.size, bool), rank_b >= cnt_a
    elif op == INTERSECTION:
        keep_a, keep_b = rank_a < cnt_b, np.zeros(b.size, bool)
    elif op == DIFFERENCE:
        keep_a, keep_b = rank_a >= cnt_b, np.zeros(b.size, bool)
    elif op == SYMMETRIC_DIFFERENCE:
        keep_a, keep_b = rank_a >= cnt_b, rank_b >= cnt_a
    else:
        raise ValueError(op)
    # the stable merge: b-elements before an a-element are those strictly
    # before it, a-elements before a b-element those not after it
    return keep_a, keep_b, np.arange(a.size) + lb_ba, np.arange(b.size) + ub_ab


def set_operation(op, a, b, descending=False, with_source=False):
    """The kept elements in output order (bitwise copies of the inputs'); with
    with_source also the range (0 / 1) each came from."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    keep_a, keep_b, pos_a, pos_b = keep_masks(op, a, b, descending)
    merged = np.empty(a.size + b.size, dtype=a.dtype)
    keep = np.zeros(a.size + b.size, bool)
    src = np.zeros(a.size + b.size, np.uint8)
    merged[pos_a], merged[pos_b] = a, b
    keep[pos_a], keep[pos_b] = keep_a, keep_b
    src[pos_b] = 1
    return (merged[keep], src[keep]) if with_source else merged[keep]


def includes(a, b, descending=False):
    """std::includes(a, b): set_difference(b, a) keeps nothing."""
    keep_b = keep_masks(DIFFERENCE, b, a, descending)[0]
    return not keep_b.any()
