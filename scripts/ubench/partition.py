#!/usr/bin/env python3
"""The two-sided compaction kernel against copy_if and copy.

Times, alternating in one process at 2^logn int64 with about 50 % accepted
(x >= 1 over values uniform in [-256, 256]):

  partition_copy     hpxhip_partition_copy, two separate outputs
  remove_if          hpxhip_partition_copy with out_false == in, no out_true
  stable_partition   hpxhip_stable_partition, in place
  copy_if            hpxhip_copy_if (the one-sided kernel)
  copy               hpxhip_copy (the same 16 B per element as partition_copy)

HIP events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).  The in-place shapes
run on a vector that is partitioned after the first call; the kernel does the
same work on it (the count stays, the accepted elements are then in front).
To keep the acceptance pattern random for them, the input is copied back
before every in-place call, outside the timed span.

Byte model (int64): partition_copy 8 B read + 8 B written per element;
remove_if 8 B read + 8 B per kept element; stable_partition the
partition_copy bytes + 16 B per rejected element; copy_if 8 B read + 8 B per
hit; copy 16 B per element.  GB/s and the share of the 8 TB/s HBM peak are on
that model.

    python scripts/ubench/partition.py [--logn 28] [--reps 20] [--warmup 3]
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
    vals_h = np.random.default_rng(2026).integers(-256, 256, n, endpoint=True).astype(np.int64)
    hits = int(np.count_nonzero(vals_h >= 1))  # ~50 % (256 of 513 values)
    vals = hpx.vector.from_host(vals_h, t)
    first_hits = vals_h[vals_h >= 1][:4].copy()
    first_rest = vals_h[vals_h < 1][:4].copy()
    del vals_h
    work = hpx.vector(n, dtype=np.int64, tgt=t)   # the in-place shapes' range
    ot = hpx.vector(n, dtype=np.int64, tgt=t)
    of = hpx.vector(n, dtype=np.int64, tgt=t)
    count = hpx.vector(2, dtype=np.uint64, tgt=t)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))
    one = L.scalar_buf(L.I64, 1)

    def restore():
        L.call("hpxhip_copy", L.I64, vp(vals.data()), vp(work.data()), n, s)

    def partition_copy():
        L.call("hpxhip_partition_copy", L.I64, L.P_GE, one, vp(vals.data()), vp(ot.data()), vp(of.data()), n,
               vp(count.data()), s, None, 0)

    def remove_if():
        L.call("hpxhip_partition_copy", L.I64, L.P_GE, one, vp(work.data()), None, vp(work.data()), n,
               vp(count.data()), s, None, 0)

    def stable_partition():
        L.call("hpxhip_stable_partition", L.I64, L.P_GE, one, vp(work.data()), n, vp(count.data()), s, None, 0)

    def copy_if():
        L.call("hpxhip_copy_if", L.I64, L.P_GE, one, vp(vals.data()), vp(ot.data()), n, vp(count.data()), s, None, 0)

    def copy():
        L.call("hpxhip_copy", L.I64, vp(vals.data()), vp(ot.data()), n, s)

    rest = n - hits
    shapes = [("partition_copy 50%", partition_copy, None, 16 * n),
              ("copy_if 50%", copy_if, None, 8 * n + 8 * hits),
              ("remove_if 50% in place", remove_if, restore, 8 * n + 8 * rest),
              ("copy", copy, None, 16 * n),
              ("stable_partition 50%", stable_partition, restore, 16 * n + 16 * rest)]

    def timed(fn, before):
        if before:
            before()
        L.call("hpxhip_event_record", e0, s)
        fn()
        L.call("hpxhip_event_record", e1, s)
        L.call("hpxhip_event_synchronize", e1)
        ms = ctypes.c_float()
        L.call("hpxhip_event_elapsed_ms", e0, e1, ctypes.byref(ms))
        return ms.value

    for _ in range(a.warmup):
        for _, fn, before, _ in shapes:
            timed(fn, before)
    # what the kernels report
    partition_copy()
    L.call("hpxhip_stream_synchronize", s)
    assert int(count.to_host()[0]) == hits
    restore()
    stable_partition()
    L.call("hpxhip_stream_synchronize", s)
    assert int(count.to_host()[0]) == hits
    w = hpx.vector(8, dtype=np.int64, tgt=t)
    L.call("hpxhip_copy", L.I64, vp(work.data()), vp(w.data()), 4, s)
    L.call("hpxhip_copy", L.I64, vp(work.data() + 8 * hits), vp(w.data() + 32), 4, s)
    L.call("hpxhip_stream_synchronize", s)
    got = w.to_host()
    assert np.array_equal(got[:4], first_hits) and np.array_equal(got[4:], first_rest), got

    ms = {name: [] for name, _, _, _ in shapes}
    for _ in range(a.reps):  # alternating: every shape once per repetition
        for name, fn, before, _ in shapes:
            ms[name].append(timed(fn, before))
    hpx.compute.device_error_check(t.device)
    cif = statistics.median(ms["copy_if 50%"])
    cpy = statistics.median(ms["copy"])
    print(f"n = 2^{a.logn} int64, x >= 1 ({hits} of {n} accepted); {a.reps} repetitions, median [min, max] ms")
    out = {}
    for name, _, _, nbytes in shapes:
        med = statistics.median(ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        out[name] = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                     "bytes": nbytes, "GBps": round(gbs, 1), "peak_share": round(gbs * 1e9 / PEAK, 3),
                     "vs_copy_if": round(med / cif, 3), "vs_copy": round(med / cpy, 3)}
        print(f"{name:24s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms  {gbs:7.1f} GB/s  "
              f"{100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {med / cif:5.3f} x copy_if  {med / cpy:5.3f} x copy")
    model = 16 * n / (8 * n + 8 * hits)
    print(f"byte model: partition_copy / copy_if = {model:.3f}, measured "
          f"{statistics.median(ms['partition_copy 50%']) / cif:.3f}")
    print(json.dumps({"partition_ubench": {"logn": a.logn, "reps": a.reps, "hits": hits, "rows": out}}))


if __name__ == "__main__":
    main()
