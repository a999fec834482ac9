"""bench.py --dump-outputs on one MI355X: the files hold what the last timed
step returned (triad's a, the scan's y, the reduce's sum), as float64, the
sampled windows of dump_windows where the arrays are larger than the sample,
identical from run to run; and a plain run reports the step alone (`--full`
adds the extras)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(gpu_target, argv):
    import bench
    from hpx_amd import segmented as S
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        bench.main(argv, comm_tgt=(S.LocalComm(gpu_target), gpu_target))
    lines = [ln for ln in out.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.parametrize("logn", [16, 22])   # whole arrays; sampled windows (2^22 > 2^21)
def test_dump_outputs_match_the_oracle(gpu_target, tmp_path, logn):
    import bench
    from oracle import oracle as O
    n = 1 << logn
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(gpu_target, ["--steps", "2", "--warmup", "1", "--logn", str(logn), "--dump-outputs", d1])
    _run(gpu_target, ["--steps", "3", "--warmup", "0", "--logn", str(logn), "--dump-outputs", d2])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "extras" not in line and "cpu_baseline" not in line and line["roofline"]["traffic"] is None
    assert sorted(os.listdir(d1)) == ["inclusive_scan.npy", "transform_reduce.npy", "triad.npy"]
    idx = np.concatenate([np.arange(lo, lo + c) for lo, c in bench.dump_windows(n)])
    assert (len(idx) == n) == (logn == 16)
    b, c = O.generate(np.float64, "unit", n, 1), O.generate(np.float64, "unit", n, 2)
    x = O.generate(np.int64, "range", n, 0x5EED, -(1 << 20), 1 << 20)
    want = {"triad": O.transform_binary(b, c, "triad", (3.0,))[idx],
            "inclusive_scan": O.scan(x, 0, True)[idx].astype(np.float64),
            "transform_reduce": np.array([O.transform_reduce(x, 0)], np.float64)}
    for name, w in want.items():
        got = np.load(os.path.join(d1, name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, w), name
        assert np.array_equal(got, np.load(os.path.join(d2, name + ".npy"))), name
