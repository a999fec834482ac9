#!/usr/bin/env python3
"""unique_copy and unique against copy_if at the same keep rate, and copy.

Times, alternating in one process at 2^logn int64.  The input is the running
sum of random bits, so about half of the elements start a run, in a random
pattern; copy_if runs on a 0/1 vector with exactly the same pattern (x >= 1
where unique keeps the element), so both write the same positions' worth:

  unique_copy        hpxhip_unique_copy, a separate output
  unique in place    hpxhip_unique_copy with out == in
  copy_if            hpxhip_copy_if (the same kernel with a unary predicate)
  copy               hpxhip_copy, for scale

HIP events around each call, every shape warmed up, the median of --reps
repetitions (min and max give the run-to-run spread).  The in-place shape
runs on a vector that is restored from the input before every call, outside
the timed span.

Byte model (int64): unique_copy, unique and copy_if 8 B read + 8 B per kept
element; copy 16 B per element.  GB/s and the share of the 8 TB/s HBM peak
are on that model.  copy_if's [min, max] is the noise figure of the run:
unique_copy's median is inside or outside it.

    python scripts/ubench/unique.py [--logn 28] [--reps 20] [--warmup 3]
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
    step = np.random.default_rng(2026).integers(0, 2, n).astype(np.int64)
    step[0] = 1  # the first element is always kept
    kept = int(step.sum())
    sel = hpx.vector.from_host(step, t)         # copy_if's input: 1 where unique keeps the element
    vals_h = np.cumsum(step)
    del step
    vals = hpx.vector.from_host(vals_h, t)
    assert kept == int(vals_h[-1])              # the kept elements are 1, 2, ..., kept
    del vals_h
    work = hpx.vector(n, dtype=np.int64, tgt=t)  # the in-place shape's range
    out = hpx.vector(n, dtype=np.int64, tgt=t)
    count = hpx.vector(2, dtype=np.uint64, tgt=t)
    e0, e1 = vp(), vp()
    L.call("hpxhip_event_create", ctypes.byref(e0))
    L.call("hpxhip_event_create", ctypes.byref(e1))
    one = L.scalar_buf(L.I64, 1)

    def restore():
        L.call("hpxhip_copy", L.I64, vp(vals.data()), vp(work.data()), n, s)

    def unique_copy():
        L.call("hpxhip_unique_copy", L.I64, L.Q_EQUAL, None, vp(vals.data()), vp(out.data()), n, vp(count.data()), s,
               None, 0)

    def unique():
        L.call("hpxhip_unique_copy", L.I64, L.Q_EQUAL, None, vp(work.data()), vp(work.data()), n, vp(count.data()), s,
               None, 0)

    def copy_if():
        L.call("hpxhip_copy_if", L.I64, L.P_GE, one, vp(sel.data()), vp(out.data()), n, vp(count.data()), s, None, 0)

    def copy():
        L.call("hpxhip_copy", L.I64, vp(vals.data()), vp(out.data()), n, s)

    shapes = [("unique_copy 50%", unique_copy, None, 8 * n + 8 * kept),
              ("unique 50% in place", unique, restore, 8 * n + 8 * kept),
              ("copy_if 50%", copy_if, None, 8 * n + 8 * kept),
              ("copy", copy, None, 16 * n)]

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
    # what the kernels report: the count, and the kept elements 1, 2, 3, ...
    w = hpx.vector(8, dtype=np.int64, tgt=t)
    for fn, dst, before in ((copy_if, None, None), (unique_copy, out, None), (unique, work, restore)):
        if before:
            before()
        fn()
        L.call("hpxhip_stream_synchronize", s)
        assert int(count.to_host()[0]) == kept, fn.__name__
        if dst is not None:
            L.call("hpxhip_copy", L.I64, vp(dst.data()), vp(w.data()), 4, s)
            L.call("hpxhip_copy", L.I64, vp(dst.data() + 8 * (kept - 4)), vp(w.data() + 32), 4, s)
            L.call("hpxhip_stream_synchronize", s)
            got = w.to_host()
            assert np.array_equal(got, np.r_[1:5, kept - 3:kept + 1]), (fn.__name__, got)

    ms = {name: [] for name, _, _, _ in shapes}
    for _ in range(a.reps):  # alternating: every shape once per repetition
        for name, fn, before, _ in shapes:
            ms[name].append(timed(fn, before))
    hpx.compute.device_error_check(t.device)
    cif = statistics.median(ms["copy_if 50%"])
    cpy = statistics.median(ms["copy"])
    print(f"n = 2^{a.logn} int64, running sum of random bits ({kept} of {n} kept); {a.reps} repetitions, "
          "median [min, max] ms")
    rows = {}
    for name, _, _, nbytes in shapes:
        med = statistics.median(ms[name])
        gbs = nbytes / (med * 1e-3) / 1e9
        rows[name] = {"ms": round(med, 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                      "bytes": nbytes, "GBps": round(gbs, 1), "peak_share": round(gbs * 1e9 / PEAK, 3),
                      "vs_copy_if": round(med / cif, 3), "vs_copy": round(med / cpy, 3)}
        print(f"{name:24s} {med:8.4f} [{min(ms[name]):.4f}, {max(ms[name]):.4f}] ms  {gbs:7.1f} GB/s  "
              f"{100 * gbs * 1e9 / PEAK:5.1f} % of 8 TB/s  {med / cif:5.3f} x copy_if  {med / cpy:5.3f} x copy")
    lo, hi = min(ms["copy_if 50%"]), max(ms["copy_if 50%"])
    uc = statistics.median(ms["unique_copy 50%"])
    print(f"unique_copy's median {uc:.4f} ms is {'inside' if lo <= uc <= hi else 'outside'} copy_if's "
          f"[min, max] = [{lo:.4f}, {hi:.4f}] ms; unique_copy / copy_if = {uc / cif:.3f}")
    print(json.dumps({"unique_ubench": {"logn": a.logn, "reps": a.reps, "kept": kept, "rows": rows}}))


if __name__ == "__main__":
    main()
