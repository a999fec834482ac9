"""Host proof of the paths the padded-pass edge tests take (no GPU).

tests/test_gpu_sort_padded_edges.py sorts inputs built to reach the two
places where a bucket of the padded second prefix pass leaves its slot
without the full segment sort (one key; all keys equal), the one-by-one bin
of k_pad_scatter, the look-back fallback after a slot overflow and the
un-padded 18-bit pass.  Which of these an input reaches is decided by the
device-side planner, which has no read-back; tests/sort_plan_model.py
restates it.  Here, for every one of those inputs (same builder, same seed),
the model's verdict is asserted: the path, b2, the census of buckets of 0, 1
and 2 keys and where they lie, slot overflow and oversized buckets -- and
that each decision has margin: b2 and the path stay when every bucket
estimate is scaled by 0.99 and by 1.01, so the model need not match the
device's floating point to the last bit to be right about the path.

n = 2^22 sits on the b2 = 1 / 2 boundary (padded either way): there only
`padded` is asserted under scaling, and the census is stated relative to the
b2 the model gives."""
import numpy as np
import pytest

import sort_plan_model as M
from oracle import oracle as O


def scaled(case):
    builder, args = case
    u = M.bits_of(builder(*args))
    return [M.plan18(u, s) for s in (0.99, 1.01)]


def assert_margin(case, plan, b2_too=True):
    for p in scaled(case):
        assert p["padded"] == plan["padded"]
        if b2_too:
            assert (p["b2"], p["nb"]) == (plan["b2"], plan["nb"])


def test_model_on_a_hand_computed_input():
    """2^22 keys, 16 per (top-9, field) cell, every lower bit live: every
    statistic has a closed form.  mtop = 2^13, mg[1] = 2^21, est = 2^13 * 2^21
    / 2^22 = 4096; 4096 + 5 * 64 = 4416 <= 4608 so b2 = 1; cap = (4096 + 448 +
    1 + 63) & ~63 = 4608; 1024 * 4608 <= 2^22 * 1.25 + 4608: padded."""
    i = np.arange(1 << 22, dtype=np.uint64)
    u = ((i >> np.uint64(4)) << np.uint64(46)) | ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(18))
    p = M.plan18(u)
    assert (p["b2"], p["est"], p["cap"], p["nb"], p["padded"]) == (1, 4096.0, 4608, 1024, True)
    assert p["pad_keys"] == (1 << 22) + (1 << 20) + 4608
    assert (p["sizes"] == 4096).all() and p["max_bucket"] == 4096
    assert not p["overflow"] and p["oversized"] == 0 and p["top_single"] == 64 - 10
    assert abs(p["fit_margin"] - 192.0) < 1e-9
    # uniform top-9 digits, the field one of {0, 2}, nothing below: field
    # groups of 4 or more bins hold every key (est = 8192: no fit), pairs of
    # bins half of them (b2 = 8, est = 4096); the buckets are 4096 equal keys
    # and no bit under s2 varies (top_single = 0); 2^17 slots do not fit
    u = ((i >> np.uint64(13)) << np.uint64(55)) | ((i & np.uint64(1)) << np.uint64(47))
    p = M.plan18(u)
    assert (p["b2"], p["est"], p["cap"], p["nb"], p["padded"]) == (8, 4096.0, 4608, 1 << 17, False)
    assert p["top_single"] == 0 and p["max_bucket"] == 4096 and int((p["sizes"] == 4096).sum()) == 1024


def test_preconditions_are_asserted():
    u = np.arange(1 << 22, dtype=np.uint64)  # top bytes dead
    with pytest.raises(AssertionError):
        M.plan18(u)
    with pytest.raises(AssertionError):
        M.plan18(np.zeros(1 << 20, np.uint64))  # below the hybrid's size


@pytest.mark.parametrize("dt", [np.uint64, np.int64, np.uint32, np.int32])
@pytest.mark.parametrize("desc", [False, True])
def test_ordered_bits_round_trip_and_order(dt, desc):
    """keys_from_ordered inverts ordered_bits, and ascending ordered bits are
    the oracle's order of the keys: the GPU tests take their expected output
    as keys_from_ordered(O.sort(u))."""
    bits = 8 * np.dtype(dt).itemsize
    u = np.random.default_rng(bits + desc).integers(0, (1 << bits) - 1, 100003, dtype=M._utype(bits), endpoint=True)
    u[:4] = [0, (1 << bits) - 1, 1 << (bits - 1), (1 << (bits - 1)) - 1]
    h = M.keys_from_ordered(u, dt, desc)
    assert h.dtype == np.dtype(dt)
    np.testing.assert_array_equal(M.ordered_bits(h, desc), u)
    np.testing.assert_array_equal(M.keys_from_ordered(O.sort(u), dt, desc), O.sort(h, desc))


@pytest.mark.parametrize("case", M.CASES_A, ids=M.case_id)
def test_case_a_one_key_buckets_take_the_padded_pass(case):
    (n, bits, _seed) = case[1]
    u, planted = case[0](*case[1])
    p = M.plan_of(*case)
    assert p["padded"] and not p["overflow"] and p["oversized"] == 0
    assert p["max_bucket"] < p["cap"]
    if n == M.N_WIDE:
        assert (p["b2"], p["nb"]) == (3, 4096)
        assert p["fit_margin"] > 1000 and p["slots"] < 0.95 * p["pad_keys"]
    assert_margin(case, p, b2_too=n == M.N_WIDE)
    c = M.census(p)
    nb, b2 = p["nb"], p["b2"]
    one = sorted([0, nb - 1, M.bucket_id(p, planted["split300"][0]), M.bucket_id(p, planted["split300"][1])])
    # index 0, the two field halves of digit 300, index n - 1
    assert one[0] == 0 and one[3] == nb - 1 and one[2] == one[1] | (1 << (b2 - 1))
    assert 300 << b2 <= one[1] < (300 << b2) + (1 << (b2 - 1))
    assert c["one"] == one
    two = [M.bucket_id(p, planted["pair255"][0]), M.bucket_id(p, planted["pair256"][0])]
    assert c["two"] == two and 255 << b2 <= two[0] < 256 << b2 <= two[1] < 257 << b2
    assert M.bucket_id(p, planted["pair255"][1]) == two[0]
    assert c["empty"] == 6 * (1 << b2) - 6  # the six emptied digits but the planted buckets
    # sorted positions of the planted ends
    assert int(u.min()) == 0 and int(u.max()) == (1 << bits) - 1
    assert int((u == 0).sum()) == 1 and int((u == u.dtype.type((1 << bits) - 1)).sum()) == 1


@pytest.mark.parametrize("case", M.CASES_A16, ids=M.case_id)
def test_case_a16_sixteen_one_key_buckets(case):
    _u, keys = case[0](*case[1])
    p = M.plan_of(*case)
    assert p["padded"] and not p["overflow"] and p["oversized"] == 0
    assert p["b2"] == (3 if case[1][0] == M.N_WIDE else 2)
    assert_margin(case, p)
    c = M.census(p)
    assert c["one"] == sorted(M.bucket_id(p, k) for k in keys) and len(set(c["one"])) == 16
    assert c["one"][0] < 1 << p["b2"] and c["one"][-1] >= 511 << p["b2"]  # digits 0 and 511
    assert c["two"] == [] and c["empty"] == 16 * (1 << p["b2"]) - 16


@pytest.mark.parametrize("case", M.CASES_B, ids=M.case_id)
def test_case_b_slot_overflow_and_oversized_bucket(case):
    _u, planted = case[0](*case[1])
    p = M.plan_of(*case)
    # planned padded; one bucket over its slot (the look-back fallback) and
    # over the 4608-key segment (the oversized-bucket finish)
    assert p["padded"] and (p["b2"], p["nb"]) == (3, 4096)
    assert p["overflow"] and p["oversized"] == 1
    assert int((p["sizes"] > p["cap"]).sum()) == 1
    assert int(np.argmax(p["sizes"])) == planted["cell"] >> 1  # (top-9, 4-bit field) -> 3-bit bucket
    assert M.K_CAP18 < p["max_bucket"] < 4800 and p["cap"] < M.K_CAP18
    assert_margin(case, p)
    c = M.census(p)
    assert len(c["one"]) == 4 and len(c["two"]) == 2 and c["empty"] == 6 * 8 - 6


@pytest.mark.parametrize("case", M.CASES_C, ids=M.case_id)
def test_case_c_sparse_and_not_padded(case):
    p = M.plan_of(*case)
    assert not p["padded"] and (p["b2"], p["nb"]) == (2, 2048)
    assert p["slots"] > 1.1 * p["pad_keys"]  # 6.2 M slots wanted, 5.25 M there
    assert not (p["sizes"] > M.K_CAP18).any()
    assert_margin(case, p)
    c = M.census(p)
    # top-9 digits 410..510 are empty (0.8 * 512 = 409.6), 511 holds the sentinel alone
    assert c["empty"] == 101 * 4 + 3 + 1 and c["one"] == [2047] and c["two"] == []
    assert not p["sizes"][410 << 2:2047].any()


@pytest.mark.parametrize("case", M.CASES_D, ids=M.case_id)
def test_case_d_reaches_the_one_by_one_bin(case):
    (_n, bits, _seed) = case[1]
    u = case[0](*case[1])
    p = M.plan_of(*case)
    assert p["padded"] and (p["b2"], p["nb"]) == (5, 16384)
    assert not p["overflow"] and p["oversized"] == 0 and p["max_bucket"] < p["cap"]
    assert p["fit_margin"] > 1000 and p["slots"] < 0.96 * p["pad_keys"]
    assert_margin(case, p)
    # the padded pass reads the keys in field order, in 8 regions of 64 field
    # digits, in 8192-key tiles from each region's start.  Region 2 starts
    # with field part 8 (of 32); part 9 holds 40 keys, so the tile that holds
    # them starts in part 8 and ends in part 10 (two parts past its first key:
    # the one-by-one bin) iff part 8 does not end within 40 keys of a tile end
    part = ((u >> u.dtype.type(bits - 14)) & u.dtype.type(31)).astype(np.int64)
    per_part = np.bincount(part, minlength=32)
    assert per_part[9] == 40 and per_part.min() == 40 and np.sort(per_part)[1] > 1 << 20
    r = int(per_part[8]) % 8192
    assert 0 < r and r + 40 < 8192
    # part 9's buckets: 512 digits x 1, the 40 keys in them
    part9 = p["sizes"].reshape(512, 32)[:, 9]
    assert int(part9.sum()) == 40 and int((part9 == 1).sum()) >= 30
    assert int((p["sizes"] == 0).sum()) == int((part9 == 0).sum())


@pytest.mark.parametrize("bits", [64, 32])
def test_case_e_plans_differ_on_one_scratch(bits):
    plans = [M.plan_of(*c) for c in M.cases_e(bits)]
    assert all(p["padded"] and not p["overflow"] for p in plans)
    assert plans[0]["b2"] in (1, 2) and plans[1]["b2"] == 3 and plans[2]["b2"] in (1, 2)
    assert plans[0]["nb"] != plans[1]["nb"] and plans[0]["cap"] != plans[1]["cap"]
    for c, p in zip(M.cases_e(bits), plans):
        assert_margin(c, p, b2_too=False)
    assert M.census(plans[2])["empty"] == 0 and M.census(plans[2])["one"] == []  # the plain uniform input
