#!/usr/bin/env python3
"""reverse, rotate, swap_ranges, replace_if and adjacent_difference against
the elementwise kernels with the same bytes per element.

Times, alternating in one process at 2^logn elements of each dtype:

  copy                    hpxhip_copy, the out-of-place yardstick (s + s bytes)
  for_each                hpxhip_for_each (x + 1), the in-place yardstick
  reverse_copy            ... and with in / out offset by one element
  rotate_copy             mid = n/2 and mid = 1
  replace_if              copying and in place (x < 0 -> 0, nothing replaced)
  adjacent_difference
  reverse                 n and n - 1: both classes of the mirrored windows'
                          alignment for 8-byte types (16-B back side /
                          element-wide back side), two of four for 4-byte types
  swap_ranges             against two copies; ... and offset by one element
  rotate                  against two reverse calls
  rot_copy+copy           the rotate that is not shipped: rotate_copy into a
                          second buffer and a copy back (same bytes as rotate)

HIP events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).  The ratio is per byte
against the shape's yardstick.

    python scripts/ubench/permute.py [--logn 28] [--reps 20] [--warmup 3] [--dtypes int64,float32]
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
from hpx_amd.compute import dtype_code  # noqa: E402

PEAK = 8.0e12
vp = ctypes.c_void_p


def bench(dt, logn, reps, warmup):
    n = 1 << logn
    es = np.dtype(dt).itemsize
    code = dtype_code(np.dtype(dt))
    t = hpx.target(0)
    s = t.stream
    x = hpx.vector(n + 4, dtype=dt, tgt=t)
    y = hpx.vector(n + 4, dtype=dt, tgt=t)
    L.call("hpxhip_generate", code, L.GEN_RANGE if np.dtype(dt).kind != "f" else L.GEN_UNIT, 7, 0, 1 << 20,
           vp(x.data()), n + 4, s)
    L.call("hpxhip_generate", code, L.GEN_RANGE if np.dtype(dt).kind != "f" else L.GEN_UNIT, 8, 0, 1 << 20,
           vp(y.data()), n + 4, s)
    X, Y = x.data(), y.data()
    one = L.scalars_buf(code, (1,))
    zero = L.scalar_buf(code, 0)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))

    def copy(src=X, dst=Y, m=n):
        return lambda: L.call("hpxhip_copy", code, vp(src), vp(dst), m, s)

    def two(f, g):
        def run():
            f()
            g()
        return run

    rw = 2 * es * n  # s read + s written per element
    # name, call, bytes on the model, yardstick
    shapes = [
        ("copy", copy(), rw, "copy"),
        ("for_each", lambda: L.call("hpxhip_for_each", code, L.U_ADD_SCALAR, one, vp(X), n, s), rw, "for_each"),
        ("reverse_copy", lambda: L.call("hpxhip_reverse_copy", code, vp(X), vp(Y), n, s), rw, "copy"),
        ("reverse_copy in+1", lambda: L.call("hpxhip_reverse_copy", code, vp(X + es), vp(Y), n, s), rw, "copy"),
        ("rotate_copy mid=n/2", lambda: L.call("hpxhip_rotate_copy", code, vp(X), n // 2, n, vp(Y), s), rw, "copy"),
        ("rotate_copy mid=1", lambda: L.call("hpxhip_rotate_copy", code, vp(X), 1, n, vp(Y), s), rw, "copy"),
        ("replace_if copy", lambda: L.call("hpxhip_replace_if", code, L.P_LT, zero, zero, vp(X), vp(Y), n, s), rw,
         "copy"),
        ("replace_if in place", lambda: L.call("hpxhip_replace_if", code, L.P_LT, zero, zero, vp(X), vp(X), n, s), rw,
         "for_each"),
        ("adjacent_difference", lambda: L.call("hpxhip_adjacent_difference", code, L.B_SUB, None, vp(X), vp(Y), n, s),
         rw, "copy"),
        ("reverse n", lambda: L.call("hpxhip_reverse", code, vp(X), n, s), rw, "for_each"),
        ("reverse n-1", lambda: L.call("hpxhip_reverse", code, vp(X), n - 1, s), rw, "for_each"),
        ("two copies", two(copy(X, Y), copy(Y, X)), 2 * rw, "two copies"),
        ("swap_ranges", lambda: L.call("hpxhip_swap_ranges", code, vp(X), vp(Y), n, s), 2 * rw, "two copies"),
        ("swap_ranges a+1", lambda: L.call("hpxhip_swap_ranges", code, vp(X + es), vp(Y), n, s), 2 * rw,
         "two copies"),
        ("two reverses", two(lambda: L.call("hpxhip_reverse", code, vp(X), n, s),
                             lambda: L.call("hpxhip_reverse", code, vp(X), n, s)), 2 * rw, "two reverses"),
        ("rotate mid=n/2", lambda: L.call("hpxhip_rotate", code, vp(X), n // 2, n, s), 2 * rw, "two reverses"),
        ("rotate mid=1", lambda: L.call("hpxhip_rotate", code, vp(X), 1, n, s), 2 * rw, "two reverses"),
        # the variant that is not shipped: rotate_copy into a second buffer, then a copy back
        ("rot_copy+copy mid=n/2", two(lambda: L.call("hpxhip_rotate_copy", code, vp(X), n // 2, n, vp(Y), s),
                                      copy(Y, X)), 2 * rw, "two reverses"),
        ("rot_copy+copy mid=1", two(lambda: L.call("hpxhip_rotate_copy", code, vp(X), 1, n, vp(Y), s), copy(Y, X)),
         2 * rw, "two reverses"),
    ]

    def timed(fn):
        L.call("hpxhip_event_record", e0, s)
        fn()
        L.call("hpxhip_event_record", e1, s)
        L.call("hpxhip_event_synchronize", e1)
        ms = ctypes.c_float()
        L.call("hpxhip_event_elapsed_ms", e0, e1, ctypes.byref(ms))
        return ms.value

    for _ in range(warmup):
        for _, fn, _, _ in shapes:
            timed(fn)
    ms = {name: [] for name, _, _, _ in shapes}
    for _ in range(reps):  # alternating: every shape once per repetition
        for name, fn, _, _ in shapes:
            ms[name].append(timed(fn))
    hpx.compute.device_error_check(t.device)
    print(f"n = 2^{logn} {np.dtype(dt).name}; {reps} repetitions, median [min, max] ms")
    rows = {}
    per_byte = {name: statistics.median(ms[name]) / nbytes for name, _, nbytes, _ in shapes}
    for name, _, nbytes, yard in shapes:
        med = statistics.median(ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        ratio = per_byte[name] / per_byte[yard]
        rows[name] = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                      "bytes": nbytes, "GBps": round(gbs, 1), "yardstick": yard, "ratio": round(ratio, 3)}
        print(f"{name:22s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms  {gbs:7.1f} GB/s  "
              f"{100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {ratio:5.3f} x {yard}")
    print(json.dumps({"bench": "permute", "dtype": np.dtype(dt).name, "logn": logn, "reps": reps, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="int64,float32")
    a = ap.parse_args()
    for name in a.dtypes.split(","):
        bench(np.dtype(name).type, a.logn, a.reps, a.warmup)


if __name__ == "__main__":
    main()
