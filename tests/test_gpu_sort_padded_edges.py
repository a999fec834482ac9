"""Edges of the keys-only sort's default plan, the 18-bit form with the
padded second prefix pass (sort.hip; k_pad_scatter -> k_pad_bounds ->
k_bucket_sort reading each bucket from its slot): in that plan k_bucket_sort
is the only step that moves a bucket from its slot in the padded buffer to
its place in the keys, so every way out of it must write the bucket first.

 a. buckets of ONE key (and of two) in the padded pass: before the fix the
    `m < 2` return left the key in its slot -- keys[b] kept a stale key, one
    key lost and another duplicated;
 b. the same sparse input with a slot overflow: the look-back fallback
    (C_PAD cleared) plus the oversized-bucket finish;
 c. sparse and not padded: the look-back pass and k_bucket_bounds;
 d. the one-by-one bin of k_pad_scatter (keys two field parts past their
    tile's first key), which no uniform field reaches;
 e. four sorts of different plans on one scratch (slot counters reused).
(f, all-equal buckets, needs 2^29 keys: tests/test_gpu_fullsize.py.)

The planner runs on the device and has no read-back, so every case first
asserts the verdict of its host restatement (tests/sort_plan_model.py) for
its own input -- tests/test_sort_plan_model_host.py proves the same verdicts,
with margins, without a GPU -- and then compares P.sort element for element
with the oracle's sort (O.sort on the ordered bits, once per input, mapped to
each key type and order; the host test checks that mapping against O.sort of
the keys themselves).  A mismatch reports how many keys were lost."""
import ctypes
import functools

import numpy as np
import pytest

import hpx_amd as hpx
import sort_plan_model as M
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEY_TYPES = {64: (np.uint64, np.int64), 32: (np.uint32, np.int32)}


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


@pytest.fixture(autouse=True)
def default_form(monkeypatch):
    monkeypatch.delenv("HPXHIP_SORT_HYBRID", raising=False)


@functools.lru_cache(maxsize=2)
def sorted_bits(builder, args):
    """The oracle's sort of a case's ordered bits: one per input, shared by
    its key types and orders, never written to."""
    out = O.sort(M.bits_of(builder(*args)))
    out.setflags(write=False)
    return out


def lost_keys(got, exp):
    """(lost, spurious): keys of exp missing from got and keys of got not in
    exp, counted with multiplicity."""
    U = M._utype(8 * got.dtype.itemsize)
    both, inv = np.unique(np.concatenate([got.view(U), exp.view(U)]), return_inverse=True)
    cg = np.bincount(inv[:got.size], minlength=both.size)
    ce = np.bincount(inv[got.size:], minlength=both.size)
    return int(np.clip(ce - cg, 0, None).sum()), int(np.clip(cg - ce, 0, None).sum())


def assert_sorted_like_oracle(got, exp):
    bad = np.flatnonzero(got != exp)
    if bad.size:
        lost, spurious = lost_keys(got, exp)
        pytest.fail(f"{bad.size} of {got.size} positions differ (first at {int(bad[0])}): "
                    f"{lost} keys lost, {spurious} keys that were not in the input or are duplicated")


def run_case(pol, tgt, case, dt, desc, scratch=None):
    builder, args = case
    h = M.keys_from_ordered(M.bits_of(builder(*args)), dt, desc)
    exp = M.keys_from_ordered(sorted_bits(builder, args), dt, desc)
    v = hpx.vector.from_host(h, tgt)
    if scratch is None:
        P.sort(pol, v.begin(), v.end(), F.greater if desc else F.less)
    else:
        L.call("hpxhip_sort", v.dtype, ctypes.c_void_p(v.data()), h.size, 1 if desc else 0, tgt.stream,
               ctypes.c_void_p(scratch.data()), 8 * scratch.size())
        tgt.synchronize()
    got = v.to_host()
    v.free()
    assert_sorted_like_oracle(got, exp)


def typed(cases):
    """cases x the key types of their width x both orders."""
    return [pytest.param(c, dt, desc, id=f"{M.case_id(c)}-{np.dtype(dt).name}-{'greater' if desc else 'less'}")
            for c in cases for dt in KEY_TYPES[c[1][1]] for desc in (False, True)]


@pytest.mark.parametrize("case,dt,desc", typed(M.CASES_A))
def test_one_key_buckets_in_the_padded_pass(pol, gpu_target, case, dt, desc):
    """(a) the top-9 digits {0, 1, 255, 256, 300, 511} emptied, then: key 0
    and the all-ones key (the first and last bucket hold one key: sorted
    positions 0 and n - 1), two buckets of two keys (keys differing in bit 0;
    equal keys), two more one-key buckets (digit 300, both field halves).
    Before the fix: 4 keys lost at every size, type and order (the four
    one-key buckets stayed in their slots)."""
    p = M.plan_of(*case)
    c = M.census(p)
    assert p["padded"] and not p["overflow"] and p["oversized"] == 0
    assert len(c["one"]) == 4 and c["one"][0] == 0 and c["one"][-1] == p["nb"] - 1 and len(c["two"]) == 2
    run_case(pol, gpu_target, case, dt, desc)


@pytest.mark.parametrize("case,dt,desc", typed(M.CASES_A16))
def test_sixteen_one_key_buckets_in_the_padded_pass(pol, gpu_target, case, dt, desc):
    """(a), second variant: 16 emptied top-9 digits (0 and 511 among them),
    each holding one key in a random field group -- about as many as the slot
    budget allows (every emptied digit raises the largest digit's share and
    with it every slot).  Before the fix: 16 keys lost."""
    p = M.plan_of(*case)
    c = M.census(p)
    assert p["padded"] and not p["overflow"] and len(c["one"]) == 16 and c["empty"] == 16 * (1 << p["b2"]) - 16
    run_case(pol, gpu_target, case, dt, desc)


@pytest.mark.parametrize("case,dt,desc", typed(M.CASES_B))
def test_sparse_buckets_with_slot_overflow(pol, gpu_target, case, dt, desc):
    """(b) the input of (a) plus 1500 keys in one (top-9, 4-bit field) cell:
    still planned padded, but that bucket overflows its slot -- k_pad_check
    clears C_PAD, the look-back pass runs from the same input and the segment
    sort reads the keys in place (one-key buckets need no copy there) -- and,
    over 4608 keys, takes the oversized-bucket finish."""
    p = M.plan_of(*case)
    c = M.census(p)
    assert p["padded"] and p["overflow"] and p["oversized"] == 1 and p["cap"] < p["max_bucket"]
    assert len(c["one"]) == 4 and len(c["two"]) == 2
    run_case(pol, gpu_target, case, dt, desc)


@pytest.mark.parametrize("case,dt,desc", typed(M.CASES_C))
def test_sparse_buckets_not_padded(pol, gpu_target, case, dt, desc):
    """(c) uniform keys in the lower 80 % of the range plus the all-ones key:
    the 18-bit form WITHOUT the padded pass (the slots would not fit), bounds
    from k_bucket_bounds over ~408 empty buckets and one of a single key."""
    p = M.plan_of(*case)
    c = M.census(p)
    assert not p["padded"] and p["b2"] == 2 and c["empty"] == 408 and c["one"] == [p["nb"] - 1]
    run_case(pol, gpu_target, case, dt, desc)


@pytest.mark.parametrize("case", M.CASES_D, ids=M.case_id)
def test_one_by_one_bin_of_the_padded_scatter(pol, gpu_target, case):
    """(d) 48 * 2^20 keys whose field part 9 (of 32) holds 40 keys, between
    parts of 1.5 M: b2 = 5, and the tile across parts 8 | 9 | 10 sends its
    part-10 keys through k_pad_scatter's one-by-one branch (lb == NL) -- the
    smallest n at which the branch is reachable: it needs b2 >= 5, tiles do
    not cross the 64-digit field regions.  Part 9's 40 keys are also ~38
    one-key buckets: before the fix 38 (u64) and 36 (u32) keys were lost
    here, all of them part-9 keys -- the one-by-one branch itself was right.
    (unsigned keys, std::less.)"""
    p = M.plan_of(*case)
    assert p["padded"] and p["b2"] == 5 and not p["overflow"] and p["oversized"] == 0
    part9 = p["sizes"].reshape(512, 32)[:, 9]
    assert int(part9.sum()) == 40
    run_case(pol, gpu_target, case, KEY_TYPES[case[1][1]][0], False)


@pytest.mark.parametrize("bits,desc", [(64, False), (32, True)])
def test_slot_counters_reused_on_one_scratch(pol, gpu_target, bits, desc):
    """(e) four sorts through one caller-provided scratch, each checked: the
    2^22 input of (a), the 3 * 2^22 one (another b2, nb and slot capacity: the
    layout moves, the slot counters and slots hold the previous sort's
    leftovers), plain uniform 2^22 keys, and the first again."""
    cases = M.cases_e(bits)
    plans = [M.plan_of(*c) for c in cases]
    assert all(p["padded"] and not p["overflow"] for p in plans)
    assert plans[0]["nb"] != plans[1]["nb"] and plans[0]["cap"] != plans[1]["cap"]
    dt = KEY_TYPES[bits][0]
    need = ctypes.c_size_t()
    L.call("hpxhip_scratch_bytes", L.ALGO_SORT, L.U64 if bits == 64 else L.U32, -1, M.N_WIDE, ctypes.byref(need))
    scratch = hpx.vector((need.value + 7) // 8, dtype=np.uint64, tgt=gpu_target)
    for c in cases:
        run_case(pol, gpu_target, c, dt, desc, scratch)
    scratch.free()
