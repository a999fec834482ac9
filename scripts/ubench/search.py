#!/usr/bin/env python3
"""The search family against transform_reduce, and find_if's early exit.

Times, alternating in one process at 2^logn int64 (random values in
[1, 2^40], generated on the device; four negative marks planted at 0, n/1024,
n/8 and n/2, each a value of its own, so that find(value) hits exactly there):

  transform_reduce   hpxhip_transform_reduce(plus, identity), the yardstick
  count_if 50%       hpxhip_count_if(x < 2^39): the reduce kernel itself
  find_if no hit     hpxhip_find_if(x == 0): a full scan of k_find_first
  equal              hpxhip_mismatch of the range and a copy: twice the bytes
  min_element        hpxhip_minmax_element(MIN)
  minmax_element     hpxhip_minmax_element(MINMAX), one pass
  find hit at k      hpxhip_find_if(x == mark), k = 0, n/1024, n/8, n/2
  find empty range   hpxhip_find_if with n = 0: the launch floor

HIP events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).  Every full-scan shape is
reported per byte read against transform_reduce from the same run, whose
[min, max] is the noise figure: a ratio's median is inside or outside it.
GB/s and the share of the 8 TB/s HBM peak are on 8 B per element and input.

    python scripts/ubench/search.py [--logn 28] [--reps 20] [--warmup 3]
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
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = 1 << a.logn
    t = hpx.target(0)
    s = t.stream
    x = hpx.vector(n, dtype=np.int64, tgt=t)
    y = hpx.vector(n, dtype=np.int64, tgt=t)
    L.call("hpxhip_generate", L.I64, L.GEN_RANGE, 2026, 1, 1 << 40, vp(x.data()), n, s)
    marks = {0: -1, n // 1024: -2, n // 8: -3, n // 2: -4}
    for k, v in marks.items():
        L.call("hpxhip_memcpy_async", vp(x.data() + 8 * k), L.scalar_buf(L.I64, v), 8, L.H2D, s)
        L.call("hpxhip_stream_synchronize", s)
    L.call("hpxhip_copy", L.I64, vp(x.data()), vp(y.data()), n, s)
    out = hpx.vector(2, dtype=np.uint64, tgt=t)
    acc = hpx.vector(1, dtype=np.int64, tgt=t)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))
    zero, half = L.scalar_buf(L.I64, 0), L.scalar_buf(L.I64, 1 << 39)
    xs, ys, o = vp(x.data()), vp(y.data()), vp(out.data())

    def find(value, count=n):
        arg = L.scalar_buf(L.I64, value)
        return lambda: L.call("hpxhip_find_if", L.I64, L.P_EQ, arg, 0, xs, count, o, s)

    # name -> (call, bytes read by a full scan or None, expected out[0] or None)
    shapes = {
        "transform_reduce": (lambda: L.call("hpxhip_transform_reduce", L.I64, L.I64, L.PLUS, L.U_IDENTITY, None, zero,
                                            xs, n, vp(acc.data()), s, None, 0), 8 * n, None),
        "count_if 50%": (lambda: L.call("hpxhip_count_if", L.I64, L.P_LT, half, xs, n, o, s, None, 0), 8 * n, None),
        "find_if no hit": (find(0), 8 * n, n),
        "equal": (lambda: L.call("hpxhip_mismatch", L.I64, xs, ys, n, o, s), 16 * n, n),
        "min_element": (lambda: L.call("hpxhip_minmax_element", L.I64, L.X_MIN, 0, xs, n, o, s, None, 0), 8 * n,
                        n // 2),
        "minmax_element": (lambda: L.call("hpxhip_minmax_element", L.I64, L.X_MINMAX, 0, xs, n, o, s, None, 0),
                           8 * n, n // 2),
    }
    for k, v in marks.items():
        shapes[f"find hit at {k}"] = (find(v), None, k)
    shapes["find empty range"] = (find(0, 0), None, 0)

    def timed(fn):
        L.call("hpxhip_event_record", e0, s)
        fn()
        L.call("hpxhip_event_record", e1, s)
        L.call("hpxhip_event_synchronize", e1)
        ms = ctypes.c_float()
        L.call("hpxhip_event_elapsed_ms", e0, e1, ctypes.byref(ms))
        return ms.value

    for _ in range(a.warmup):
        for fn, _, _ in shapes.values():
            timed(fn)
    for name, (fn, _, want) in shapes.items():  # what the kernels report
        if want is not None:
            fn()
            L.call("hpxhip_stream_synchronize", s)
            got = int(out.to_host()[0])
            assert got == want, (name, got, want)
    ms = {name: [] for name in shapes}
    for _ in range(a.reps):  # alternating: every shape once per repetition
        for name, (fn, _, _) in shapes.items():
            ms[name].append(timed(fn))
    hpx.compute.device_error_check(t.device)

    ref = ms["transform_reduce"]
    ref_med = statistics.median(ref)
    per_byte = ref_med / (8 * n)
    spread = (min(ref) / ref_med, max(ref) / ref_med)
    print(f"n = 2^{a.logn} int64; {a.reps} repetitions, median [min, max] ms")
    rows = {}
    for name, (_, nbytes, _) in shapes.items():
        med = statistics.median(ms[name])
        row = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4)}
        line = f"{name:24s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms"
        if nbytes:
            gbs = nbytes / (med * 1e-3) / 1e9
            ratio = med / nbytes / per_byte
            row.update({"bytes": nbytes, "GBps": round(gbs, 1), "peak_share": round(gbs * 1e9 / PEAK, 3),
                        "per_byte_vs_transform_reduce": round(ratio, 3),
                        "inside_spread": spread[0] <= ratio <= spread[1]})
            line += (f"  {gbs:7.1f} GB/s  {100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {ratio:5.3f} x transform_reduce "
                     f"per byte ({'inside' if spread[0] <= ratio <= spread[1] else 'outside'} its spread)")
        else:
            row["vs_no_hit"] = round(med / statistics.median(ms["find_if no hit"]), 4)
            line += f"  {row['vs_no_hit']:6.4f} x find_if no hit"
        rows[name] = row
        print(line)
    print(f"transform_reduce's spread: [{spread[0]:.3f}, {spread[1]:.3f}] of its median")
    print(json.dumps({"search_ubench": {"logn": a.logn, "reps": a.reps, "rows": rows}}))


if __name__ == "__main__":
    main()
