#!/usr/bin/env python3
"""reduce_by_key against the two shipped kernels whose structure it fuses.

Times hpxhip_reduce_by_key (int64 keys, int64 values, plus) on three inputs
-- the reference recipe (run lengths uniform in 1..256, mean 128.5), all
keys distinct, all keys equal -- and, alternating with it in the same
process, inclusive_scan of int64 and copy_if of int64 at 50 % hits.  HIP
events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).

Byte model: reduce_by_key reads 16 B per element and writes 16 B per run;
the scan moves 16 B per element; copy_if reads 8 B per element and writes
8 B per hit.  GB/s and the share of the 8 TB/s HBM peak are on that model.

    python scripts/ubench/reduce_by_key.py [--logn 28] [--reps 20] [--warmup 3]
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
    rng = np.random.default_rng(2026)

    lens = rng.integers(1, 257, n // 100 + 16)
    while lens.sum() < n:
        lens = np.concatenate((lens, rng.integers(1, 257, n // 100 + 16)))
    recipe = np.repeat(np.arange(lens.size, dtype=np.int64), lens)[:n]
    runs = {"recipe": int(np.count_nonzero(recipe[1:] != recipe[:-1])) + 1, "distinct": n, "equal": 1}
    keys = {"recipe": hpx.vector.from_host(recipe, t),
            "distinct": hpx.vector.from_host(np.arange(n, dtype=np.int64), t),
            "equal": hpx.vector.from_host(np.full(n, 7, dtype=np.int64), t)}
    del recipe
    vals_h = rng.integers(-256, 256, n, endpoint=True).astype(np.int64)
    vals = hpx.vector.from_host(vals_h, t)
    hits = int(np.count_nonzero(vals_h >= 1))  # ~50 % (256 of 513 values)
    del vals_h
    ko = hpx.vector(n, dtype=np.int64, tgt=t)
    vo = hpx.vector(n, dtype=np.int64, tgt=t)
    count = hpx.vector(2, dtype=np.uint64, tgt=t)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))
    zero, one = L.scalar_buf(L.I64, 0), L.scalar_buf(L.I64, 1)

    def rbk(kind):
        L.call("hpxhip_reduce_by_key", L.I64, L.I64, L.PLUS, vp(keys[kind].data()), vp(vals.data()), vp(ko.data()),
               vp(vo.data()), n, vp(count.data()), s, None, 0)

    def scan():
        L.call("hpxhip_scan", L.I64, L.PLUS, 1, L.U_IDENTITY, None, zero, None, vp(vals.data()), vp(vo.data()), n, s,
               None, 0)

    def copy_if():
        L.call("hpxhip_copy_if", L.I64, L.P_GE, one, vp(vals.data()), vp(vo.data()), n, vp(count.data()), s, None, 0)

    shapes = [("reduce_by_key recipe", lambda: rbk("recipe"), 16 * n + 16 * runs["recipe"]),
              ("inclusive_scan", scan, 16 * n),
              ("reduce_by_key distinct", lambda: rbk("distinct"), 16 * n + 16 * runs["distinct"]),
              ("copy_if 50%", copy_if, 8 * n + 8 * hits),
              ("reduce_by_key equal", lambda: rbk("equal"), 16 * n + 16 * runs["equal"])]

    def timed(fn):
        L.call("hpxhip_event_record", e0, s)
        fn()
        L.call("hpxhip_event_record", e1, s)
        L.call("hpxhip_event_synchronize", e1)
        ms = ctypes.c_float()
        L.call("hpxhip_event_elapsed_ms", e0, e1, ctypes.byref(ms))
        return ms.value

    for _ in range(a.warmup):
        for _, fn, _ in shapes:
            timed(fn)
    # the run counts the kernel reports
    for kind in ("recipe", "distinct", "equal"):
        rbk(kind)
        L.call("hpxhip_stream_synchronize", s)
        got = int(count.to_host()[0])
        assert got == runs[kind], (kind, got, runs[kind])
    ms = {name: [] for name, _, _ in shapes}
    for _ in range(a.reps):  # alternating: every shape once per repetition
        for name, fn, _ in shapes:
            ms[name].append(timed(fn))
    hpx.compute.device_error_check(t.device)
    scan_med = statistics.median(ms["inclusive_scan"])
    print(f"n = 2^{a.logn} int64 keys / int64 values, plus; {a.reps} repetitions, median [min, max] ms")
    out = {}
    for name, _, nbytes in shapes:
        med = statistics.median(ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        out[name] = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                     "bytes": nbytes, "GBps": round(gbs, 1), "peak_share": round(gbs * 1e9 / PEAK, 3),
                     "vs_scan": round(med / scan_med, 3)}
        print(f"{name:24s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms  {gbs:7.1f} GB/s  "
              f"{100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {med / scan_med:5.3f} x scan")
    exp = scan_med * (16 * n + 16 * runs["recipe"]) / (16 * n)
    print(f"recipe: runs = {runs['recipe']}, scan time x (bytes moved / scan bytes) = {exp:.4f} ms")
    print(json.dumps({"reduce_by_key_ubench": {"logn": a.logn, "reps": a.reps, "runs": runs, "rows": out}}))


if __name__ == "__main__":
    main()
