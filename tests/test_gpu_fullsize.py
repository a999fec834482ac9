"""Full-size checks at the benchmark's scales (BASELINE.json configs[1] and
[2]: 2^30 int64/double reduce and scan, 2^30 uint64 sort), through
size-independent properties and closed forms, plus the range overload of
sort (container_algorithms/sort.hpp:102, sort_range_tests.hpp) and
is_sorted (is_sorted.hpp).

* double reduce/scan at 2^30: x_i = 0.5 * k_i with integers k_i in [0, 1023]
  -> every partial sum is a multiple of 0.5 below 2^53, so every summation
  order gives the same double: the GPU results equal 0.5 * the int64 results
  bit for bit (the reference's all-1.0 benchmark, inclusive_scan_tests.hpp:26-60,
  generalised);
* mixed-sign double scan: |gpu - exact prefix| <= (2 ntiles + 64) u sum_{j<=i}|x_j|
  (exact prefix in 80-bit long double on the host), a bound that stays
  meaningful under cancellation;
* sort of 2^30 uint64: a permutation of the input (XOR and wrapping sum of the
  keys unchanged) with no adjacent pair out of order (device-side is_sorted);
  and (r05) element for element against a closed form: keys whose top bits
  are a permutation of [0, n) (test_sort_2p30_element_exact)."""
import ctypes

import numpy as np
import pytest

import hpx_amd as hpx
from hpx_amd import _lib as L
from hpx_amd import execution as ex, functional as F
from hpx_amd import parallel as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pol(gpu_target):
    return ex.par.on(hpx.default_executor(gpu_target))


def window(v, lo, n, dt):
    out = np.empty(n, dt)
    L.call("hpxhip_memcpy_async", out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(v.data() + lo * out.itemsize),
           out.nbytes, L.D2H, v.target().stream)
    v.target().synchronize()
    return out


def test_double_reduce_scan_2p30_exact(pol, gpu_target):
    n = 1 << 30
    k = hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    P.generate(pol, k.begin(), k.end(), "range", 0x5EED, 0, 1023)
    x = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    L.call("hpxhip_transform", L.I64, L.F64, L.F64, L.U_SCALE, L.scalars_buf(L.F64, [0.5]), ctypes.c_void_p(k.data()),
           ctypes.c_void_p(x.data()), n, gpu_target.stream)
    ki = P.reduce(pol, k.begin(), k.end(), 0, F.plus)
    xs = P.reduce(pol, x.begin(), x.end(), 0.0, F.plus)
    assert xs == 0.5 * ki and ki > 0
    y = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    P.inclusive_scan(pol, x.begin(), x.end(), y.begin(), F.plus, 0.0)
    ky = hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    P.inclusive_scan(pol, k.begin(), k.end(), ky.begin(), F.plus, 0)
    for lo in (0, (1 << 20) - 3, n // 2 + 4097, n - 4096):
        np.testing.assert_array_equal(window(y, lo, 4096, np.float64), 0.5 * window(ky, lo, 4096, np.int64))
    assert window(y, n - 1, 1, np.float64)[0] == xs
    # exclusive: y_ex[i] = y_in[i] - x[i] exactly (all values are multiples of 0.5)
    P.exclusive_scan(pol, x.begin(), x.end(), y.begin(), 0.0)
    w = window(y, n - 4096, 4096, np.float64)
    kk = window(ky, n - 4096, 4096, np.int64) - window(k, n - 4096, 4096, np.int64)
    np.testing.assert_array_equal(w, 0.5 * kk)
    for v in (k, x, y, ky):
        v.free()


def test_int64_scan_2p30_properties(pol, gpu_target):
    n = 1 << 30
    x = hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    P.generate(pol, x.begin(), x.end(), "range", 7, -(1 << 40), 1 << 40)
    y = hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    P.inclusive_scan(pol, x.begin(), x.end(), y.begin(), F.plus, 11)
    r = P.reduce(pol, x.begin(), x.end(), 11, F.plus)
    assert window(y, n - 1, 1, np.int64)[0] == r
    # sampled windows against the host restatement of the generator + a scan
    for lo in (0, n // 3, n - 8192):
        xs = O.generate(np.int64, "range", 8192, 7, -(1 << 40), 1 << 40, offset=lo)
        base = 11 if lo == 0 else int(window(y, lo - 1, 1, np.int64)[0])
        np.testing.assert_array_equal(window(y, lo, 8192, np.int64), O.scan(xs, base, True))
    x.free()
    y.free()


def test_mixed_sign_double_scan_bound(pol, gpu_target):
    n = (1 << 24) + 3
    x = O.generate(np.float64, "unit", n, 0x5EED) - 0.5
    dx = hpx.vector.from_host(x, gpu_target)
    dy = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    P.inclusive_scan(pol, dx.begin(), dx.end(), dy.begin(), F.plus, 0.0)
    got = dy.to_host()
    exact = np.cumsum(x.astype(np.longdouble))
    u = 2.0 ** -53
    ntiles = n // 12288 + 2
    bound = (2 * ntiles + 64) * u * np.cumsum(np.abs(x))
    err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
    assert np.all(err <= bound), float(np.max(err / bound))
    # the bound is not vacuous: the prefixes cancel to a few units while sum|x| grows to n/4
    assert float(np.max(np.abs(got[-1000:]))) < 0.01 * float(np.sum(np.abs(x)))


@pytest.mark.parametrize("desc,kdt", [(False, np.uint64), (True, np.uint64), (False, np.uint32)])
def test_sort_2p30_permutation_and_order(pol, gpu_target, desc, kdt):
    # u64: the 18-bit hybrid (two 9-bit prefix passes, ~4096-key buckets in
    # 512 x 9 LDS segments); u32: the same hybrid on 32-bit keys (two LDS
    # passes finish each bucket)
    n = 1 << 30
    keys = hpx.vector(n, dtype=kdt, tgt=gpu_target)
    P.generate(pol, keys.begin(), keys.end(), "bits", 7)
    xor0 = P.reduce(pol, keys.begin(), keys.end(), 0, F.bit_xor)
    sum0 = P.reduce(pol, keys.begin(), keys.end(), 0, F.plus)
    comp = F.greater if desc else F.less
    assert not P.is_sorted(pol, keys.begin(), keys.end(), comp)
    P.sort(pol, keys.begin(), keys.end(), comp)
    assert P.is_sorted(pol, keys.begin(), keys.end(), comp)
    assert not P.is_sorted(pol, keys.begin(), keys.end(), F.less if desc else F.greater)
    assert P.reduce(pol, keys.begin(), keys.end(), 0, F.bit_xor) == xor0
    assert P.reduce(pol, keys.begin(), keys.end(), 0, F.plus) == sum0
    keys.free()


# ---------------------------------------------------- sort_range_tests.hpp
@pytest.mark.parametrize("dt", [np.int64, np.uint32, np.float64, np.int32])
def test_sort_range_overload(pol, gpu_target, dt):
    # test_sort1/2: HPX_SORT_TEST_SIZE (5,000,000) random values, default and
    # std::greater comparisons, sync and task policies; verify_ = sortedness
    n = 5000000
    rng = np.random.default_rng(int(np.dtype(dt).itemsize))
    if np.dtype(dt).kind == "f":
        h = rng.uniform(-1e300, 1e300, n).astype(dt)
    else:
        info = np.iinfo(dt)
        h = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v = hpx.vector.from_host(h, gpu_target)
    end = P.sort(pol, v)
    assert end == v.end()
    np.testing.assert_array_equal(v.to_host(), O.sort(h))
    assert P.is_sorted(pol, v.begin(), v.end())
    v2 = hpx.vector.from_host(h, gpu_target)
    tpol = ex.par(ex.task).on(hpx.default_executor(gpu_target))
    P.sort(tpol, v2, F.greater).get()
    np.testing.assert_array_equal(v2.to_host(), O.sort(h, True))
    assert P.is_sorted(tpol, v2.begin(), v2.end(), F.greater).get()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000, 4097])
def test_is_sorted_small(pol, gpu_target, n):
    for dt in (np.int32, np.int64, np.float32):
        h = np.sort(np.random.default_rng(n).integers(-100, 100, n).astype(dt))
        v = hpx.vector.from_host(h, gpu_target)
        assert P.is_sorted(pol, v.begin(), v.end())
        if n >= 2:
            h2 = h.copy()
            h2[0] = h2.max() + 1  # one pair out of order
            v2 = hpx.vector.from_host(h2, gpu_target)
            assert not P.is_sorted(pol, v2.begin(), v2.end())
            assert P.is_sorted(pol, v2.begin(), v2.end(), F.greater) == (n == 2)
        # unaligned start
        if n >= 3:
            assert P.is_sorted(pol, v.begin() + 1, v.end())


def _host_is_sorted(h, desc=False):
    """is_sorted.hpp:40-120: no i with pred(h[i+1], h[i]) (pred = less / greater)."""
    return not any((h[i] < h[i + 1]) if desc else (h[i + 1] < h[i]) for i in range(len(h) - 1))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_is_sorted_signed_zero_and_nan(pol, gpu_target, dt):
    """Values, not the sort's radix key order, decide: [0.0, -0.0] is sorted
    (they compare equal), and a NaN is never out of order."""
    nan = np.nan
    cases = [[0.0, -0.0], [-0.0, 0.0], [1.0, -0.0, 0.0, 2.0], [1.0, nan, 0.5], [nan, nan], [nan, -1.0, 3.0],
             [2.0, 1.0, nan], [-np.inf, -0.0, 0.0, np.inf], [3.0, 2.0, -0.0, 0.0, nan, -5.0]]
    for c in cases:
        for pad in (0, 1, 6):  # the pair inside a 16-B vector, across vectors, unaligned start
            h = np.array([-1e30] * pad + c, dt)
            v = hpx.vector.from_host(h, gpu_target)
            for desc, comp in ((False, F.less), (True, F.greater)):
                hh = h if not desc else np.array([1e30] * pad + c, dt)
                if desc:
                    v = hpx.vector.from_host(hh, gpu_target)
                exp = _host_is_sorted(hh, desc)
                assert P.is_sorted(pol, v.begin(), v.end(), comp) == exp, (c, pad, desc)
                if len(hh) > 2:
                    assert P.is_sorted(pol, v.begin() + 1, v.end(), comp) == _host_is_sorted(hh[1:], desc)


def test_sort_2p30_oversized_bucket(pol, gpu_target):
    # 2^30 keys: the hybrid sorts one bucket per workgroup straight from the
    # bucket bounds; 30000 extra keys in one prefix make that bucket too
    # large for the LDS segment -- the segment sort records it and the plan
    # finishes it on the device (sort.hip: the oversized-bucket finish, or
    # the whole-array LSD beyond its bucket limit).  Checked on the device:
    # ordered, and a permutation of the input (XOR and wrapping sum unchanged).
    n = 1 << 30
    keys = hpx.vector(n, dtype=np.uint64, tgt=gpu_target)
    P.generate(pol, keys.begin(), keys.end(), "bits", 9)
    rng = np.random.default_rng(5)
    crafted = (np.uint64(0x1ABCD) << np.uint64(47)) | rng.integers(0, 1 << 47, 30000, dtype=np.uint64)
    crafted[:100] = np.uint64(0x1ABCD) << np.uint64(47)  # duplicates inside the big bucket
    P.copy(pol, crafted, None, keys.begin() + 12345)
    xor0 = P.reduce(pol, keys.begin(), keys.end(), 0, F.bit_xor)
    sum0 = P.reduce(pol, keys.begin(), keys.end(), 0, F.plus)
    P.sort(pol, keys.begin(), keys.end())
    assert P.is_sorted(pol, keys.begin(), keys.end())
    assert P.reduce(pol, keys.begin(), keys.end(), 0, F.bit_xor) == xor0
    assert P.reduce(pol, keys.begin(), keys.end(), 0, F.plus) == sum0
    keys.free()


_PERM_A, _PERM_B = 0x2545F491, 0x1234567  # i -> (A i + B) mod n: a bijection of [0, n) (A odd)
_HASH_C = 0x9E3779B97F4A7C15 - (1 << 64)  # multiplicative hash (as int64)
_CHUNK = 1 << 26


def _perm_keys(lo, cnt, n, shift, dev):
    """Bit patterns (int64) of the keys of indices [lo, lo + cnt): the top
    bits hold a permutation of [0, n), the `shift` low bits a hash of the
    index.  Computed with torch on the test's GPU (test plumbing: numpy took
    ~3 s per 2^26 keys); int64 products wrap like uint64 ones."""
    import torch
    i = torch.arange(lo, lo + cnt, dtype=torch.int64, device=dev)
    p = (i * _PERM_A + _PERM_B) & (n - 1)
    h = ((i * _HASH_C) >> (64 - shift)) & ((1 << shift) - 1)
    return (p << shift) | h


def _perm_sorted(lo, cnt, n, shift, dev):
    """Ascending positions [lo, lo + cnt) of the sorted keys, in closed form:
    position j holds the key whose permuted top bits are j."""
    import torch
    j = torch.arange(lo, lo + cnt, dtype=torch.int64, device=dev)
    i = ((j - _PERM_B) * pow(_PERM_A, -1, n)) & (n - 1)
    h = ((i * _HASH_C) >> (64 - shift)) & ((1 << shift) - 1)
    return (j << shift) | h


@pytest.mark.parametrize("kdt,logn,desc", [(np.uint64, 30, False), (np.uint32, 30, False), (np.uint64, 28, True)])
def test_sort_2p30_element_exact(pol, gpu_target, kdt, logn, desc):
    """Element for element at the benchmark's size (weak item r04: the 2^30
    sort had been checked by checksums and sortedness only): the keys' top
    log2(n) bits are a permutation of [0, n) and the low bits a hash of the
    index, so the sorted array has a closed form (_perm_sorted).  Keys are
    made and checked in 2^26-key windows on the device with torch (D2D
    copies in and out of the library's vector); the sort is the library's."""
    import torch
    dev = torch.device("cuda", gpu_target.device)
    n = 1 << logn
    isz = np.dtype(kdt).itemsize
    shift = 8 * isz - logn
    tdt = torch.int64 if isz == 8 else torch.int32

    def narrow(x):  # int64 bit patterns -> the key width (exact: wrap 32-bit patterns to int32)
        return x if isz == 8 else (x - ((x >> 31) & 1) * (1 << 32)).to(torch.int32)

    keys = hpx.vector(n, dtype=kdt, tgt=gpu_target)
    torch.cuda.synchronize(dev)
    for lo in range(0, n, _CHUNK):
        h = narrow(_perm_keys(lo, _CHUNK, n, shift, dev))
        torch.cuda.synchronize(dev)
        L.call("hpxhip_memcpy_async", ctypes.c_void_p(keys.data() + lo * isz), ctypes.c_void_p(h.data_ptr()),
               h.numel() * isz, L.D2D, gpu_target.stream)
        gpu_target.synchronize()
    P.sort(pol, keys.begin(), keys.end(), F.greater if desc else F.less)
    got = torch.empty(_CHUNK, dtype=tdt, device=dev)
    for lo in range(0, n, _CHUNK):
        L.call("hpxhip_memcpy_async", ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(keys.data() + lo * isz),
               _CHUNK * isz, L.D2D, gpu_target.stream)
        gpu_target.synchronize()
        if desc:  # position lo + t holds ascending rank n - 1 - lo - t
            exp = narrow(_perm_sorted(n - lo - _CHUNK, _CHUNK, n, shift, dev)).flip(0)
        else:
            exp = narrow(_perm_sorted(lo, _CHUNK, n, shift, dev))
        bad = int((got != exp).sum())
        assert bad == 0, (lo, bad)
    keys.free()


@pytest.mark.parametrize("kdt", [np.uint64, np.uint32])
def test_sort_2p29_all_equal_buckets_padded(pol, gpu_target, kdt, monkeypatch):
    """Buckets of EQUAL keys in the padded second prefix pass: 2^29 keys
    taking 2^17 values v << (bits - 17) -- small ids in the high bits --,
    key i = ((A i + B) mod 2^17) << (bits - 17), so every value occurs 4096
    times and sorted position j holds (j >> 12) << (bits - 17).

    By the planner (sort.hip k_sort_plan; tests/sort_plan_model.py restates
    it, but would need the 2^29 keys on the host): live bytes P-1, P-2, P-3
    (bit bits-17 lies in byte P-3); top-9 digit = v >> 8, 2^20 keys each; the
    field is (v & 255) << 1, 256 bins of 2^21; b2 <= 7 groups four or more
    bins (est >= 8192: no fit), b2 = 8 gives est = 2^20 * 2^21 / 2^29 = 4096,
    4096 + 5 * 64 <= 4608; no joint cell over 4608 * 32; cap = (4096 + 448 + 1
    + 63) & ~63 = 4608; nb * cap = 2^17 * 4608 = 604 M <= pad_keys = 671 M:
    the padded pass, each bucket one value's 4096 keys.  s2 = bits - 17 and no
    bit under it varies, so top_single = 0: k_bucket_sort finds `top <= 0` in
    every bucket and, before the fix, returned without writing the bucket
    from its slot to the keys -- the output was the stale buffer (536866816
    of the 536870912 positions wrong, u64 and u32 alike).  2^29 is the
    smallest such n (at 2^28 byte P-3 is dead: the LSD)."""
    import torch
    monkeypatch.delenv("HPXHIP_SORT_HYBRID", raising=False)
    dev = torch.device("cuda", gpu_target.device)
    n = 1 << 29
    isz = np.dtype(kdt).itemsize
    shift = 8 * isz - 17
    tdt = torch.int64 if isz == 8 else torch.int32

    def narrow(x):  # int64 bit patterns -> the key width
        return x if isz == 8 else (x - ((x >> 31) & 1) * (1 << 32)).to(torch.int32)

    keys = hpx.vector(n, dtype=kdt, tgt=gpu_target)
    torch.cuda.synchronize(dev)
    for lo in range(0, n, _CHUNK):
        i = torch.arange(lo, lo + _CHUNK, dtype=torch.int64, device=dev)
        h = narrow(((i * _PERM_A + _PERM_B) & ((1 << 17) - 1)) << shift)
        torch.cuda.synchronize(dev)
        L.call("hpxhip_memcpy_async", ctypes.c_void_p(keys.data() + lo * isz), ctypes.c_void_p(h.data_ptr()),
               h.numel() * isz, L.D2D, gpu_target.stream)
        gpu_target.synchronize()
    P.sort(pol, keys.begin(), keys.end())
    got = torch.empty(_CHUNK, dtype=tdt, device=dev)
    wrong = 0
    for lo in range(0, n, _CHUNK):
        L.call("hpxhip_memcpy_async", ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(keys.data() + lo * isz),
               _CHUNK * isz, L.D2D, gpu_target.stream)
        gpu_target.synchronize()
        j = torch.arange(lo, lo + _CHUNK, dtype=torch.int64, device=dev)
        wrong += int((got != narrow((j >> 12) << shift)).sum())
    keys.free()
    assert wrong == 0, f"{wrong} of {n} positions hold another key than the sorted order's"


def test_fp_scan_reproducible_2p30(pol, gpu_target):
    """The fixed-association look-back at the benchmark's size (configs[1]
    names double): two inclusive scans of the same 2^30 mixed-sign doubles,
    with other scans launched between them, agree bit for bit (their int64
    views subtract to zero everywhere, checked on the device)."""
    n = 1 << 30
    x = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    P.generate(pol, x.begin(), x.end(), "unit", 0xF00D)
    P.transform(pol, x.begin(), x.end(), x.begin(), F.add_value(-0.5))
    y1 = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    y2 = hpx.vector(n, dtype=np.float64, tgt=gpu_target)
    P.inclusive_scan(pol, x.begin(), x.end(), y1.begin(), F.plus, 0.0)
    P.exclusive_scan(pol, x.begin(), x.end(), y2.begin(), 0.0)  # other work in between
    P.inclusive_scan(pol, x.begin() + 1, x.end(), y2.begin() + 1, F.plus, 0.0)
    P.inclusive_scan(pol, x.begin(), x.end(), y2.begin(), F.plus, 0.0)
    d = hpx.vector(n, dtype=np.int64, tgt=gpu_target)
    L.call("hpxhip_transform_binary", L.I64, L.I64, L.I64, L.B_SUB, L.scalars_buf(L.I64, []),
           ctypes.c_void_p(y1.data()), ctypes.c_void_p(y2.data()), ctypes.c_void_p(d.data()), n, gpu_target.stream)
    assert P.reduce(pol, d.begin(), d.end(), 0, F.bit_or) == 0
    assert np.isfinite(window(y1, n - 1, 1, np.float64)[0])
