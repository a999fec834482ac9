#!/usr/bin/env python3
"""The set operations against hpxhip_merge on the same inputs.

Times, alternating in one process at 2^logn + 2^logn sorted uint64 keys
(A = the even numbers, B = the odd numbers: no common keys, interleaved one by
one, so every merge tile holds both ranges):

  merge                   hpxhip_merge(A, B), the yardstick
  set_union disjoint      hpxhip_set_operation(UNION, A, B): the merge's bytes
  set_union identical     UNION(A, A): every key of range 2 is dropped
  set_intersection disj.  INTERSECTION(A, B): read-only, nothing is kept
  set_difference disj.    DIFFERENCE(A, B): all of A is kept
  includes                DIFFERENCE(A, A) counted without an output (true)

HIP events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).

Byte model (uint64): the inputs read once, the kept elements written once.
GB/s and the share of the 8 TB/s HBM peak are on that model.

    python scripts/ubench/set_ops.py [--logn 27] [--reps 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import hpx_amd as hpx  # noqa: E402
from hpx_amd import _lib as L  # noqa: E402

PEAK = 8.0e12
vp = ctypes.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=27)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = 1 << a.logn
    t = hpx.target(0)
    s = t.stream
    even = np.arange(n, dtype=np.uint64) * np.uint64(2)
    A = hpx.vector.from_host(even, t)
    even += np.uint64(1)
    B = hpx.vector.from_host(even, t)
    del even
    out = hpx.vector(2 * n, dtype=np.uint64, tgt=t)
    count = hpx.vector(2, dtype=np.uint64, tgt=t)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))

    def merge():
        L.call("hpxhip_merge", L.U64, vp(A.data()), n, vp(B.data()), n, vp(out.data()), 0, s, None, 0)

    def set_op(op, x, y, dest=True):
        def run():
            L.call("hpxhip_set_operation", L.U64, op, vp(x.data()), n, vp(y.data()), n,
                   vp(out.data()) if dest else None, 0, vp(count.data()), s, None, 0)
        return run

    # name, call, expected count (None: no count), bytes on the model
    shapes = [("merge", merge, None, 32 * n),
              ("set_union disjoint", set_op(L.SET_UNION, A, B), 2 * n, 32 * n),
              ("set_union identical", set_op(L.SET_UNION, A, A), n, 24 * n),
              ("set_intersection disjoint", set_op(L.SET_INTERSECTION, A, B), 0, 16 * n),
              ("set_difference disjoint", set_op(L.SET_DIFFERENCE, A, B), n, 24 * n),
              ("includes (identical)", set_op(L.SET_DIFFERENCE, A, A, dest=False), 0, 16 * n)]

    def timed(fn):
        L.call("hpxhip_event_record", e0, s)
        fn()
        L.call("hpxhip_event_record", e1, s)
        L.call("hpxhip_event_synchronize", e1)
        ms = ctypes.c_float()
        L.call("hpxhip_event_elapsed_ms", e0, e1, ctypes.byref(ms))
        return ms.value

    for _ in range(a.warmup):
        for _, fn, _, _ in shapes:
            timed(fn)
    # what the kernels report: the counts, and the ends of the union
    w = hpx.vector(8, dtype=np.uint64, tgt=t)
    for name, fn, want, _ in shapes:
        fn()
        L.call("hpxhip_stream_synchronize", s)
        if want is not None:
            assert int(count.to_host()[0]) == want, name
        if name in ("merge", "set_union disjoint"):
            L.call("hpxhip_copy", L.U64, vp(out.data()), vp(w.data()), 4, s)
            L.call("hpxhip_copy", L.U64, vp(out.data() + 8 * (2 * n - 4)), vp(w.data() + 32), 4, s)
            L.call("hpxhip_stream_synchronize", s)
            got = w.to_host()
            assert np.array_equal(got, np.r_[0:4, 2 * n - 4:2 * n].astype(np.uint64)), (name, got)

    ms = {name: [] for name, _, _, _ in shapes}
    for _ in range(a.reps):  # alternating: every shape once per repetition
        for name, fn, _, _ in shapes:
            ms[name].append(timed(fn))
    hpx.compute.device_error_check(t.device)
    mrg = statistics.median(ms["merge"])
    print(f"n1 = n2 = 2^{a.logn} uint64 (evens, odds); {a.reps} repetitions, median [min, max] ms")
    rows = {}
    for name, _, _, nbytes in shapes:
        med = statistics.median(ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        rows[name] = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                      "bytes": nbytes, "GBps": round(gbs, 1), "peak_share": round(gbs * 1e9 / PEAK, 3),
                      "vs_merge": round(med / mrg, 3)}
        print(f"{name:28s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms  {gbs:7.1f} GB/s  "
              f"{100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {med / mrg:5.3f} x merge")
    print(json.dumps({"bench": "set_ops", "logn": a.logn, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
