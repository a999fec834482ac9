// set_kernel.hpp -- set_union, set_intersection, set_difference and
// set_symmetric_difference of two sorted ranges in one pass (includes is
// set_difference with the ranges swapped, counted only); see
// hpx_amd/csrc/set.hip for the entry point.  Header so that the library and
// the device-closure layer (hpx/parallel/detail/device_algorithms.hpp)
// instantiate the same kernels through the same launcher.
//
// Semantics: std::set_* on multisets (set_union.hpp:47 and its siblings call
// them).  For a value v with cntA / cntB equivalent elements in range 1 / 2,
// and an element's rank k inside its own range's run of v:
//   union                 range 1: always        range 2: k >= cntA
//   intersection          range 1: k < cntB      range 2: never
//   difference            range 1: k >= cntB     range 2: never
//   symmetric difference  range 1: k >= cntB     range 2: k >= cntA
// Kept elements leave in the order of the stable merge (range 1 first on
// ties).  The reference's parallel form (detail/set_operation.hpp:72-193)
// runs std::set_* per chunk into a len1 + len2 buffer and copies the pieces
// together; here each input is read once and only kept elements are written.
//
// Tiles are those of the merge (merge_kernel.hpp): kTile elements of the
// MERGED order each, cut by merge-path diagonals.  Inside a tile the runs of
// every value strictly between the tile's first merged value vF and its last
// vL lie wholly in the tile (tile elements bracket them in merged order), so
// their bounds come from the tile's LDS copy.  Only the runs of vF and vL can
// leave the tile, and of the bounds the keep rule needs, only three can lie
// outside: lower_bound_A(vF), lower_bound_B(vF) and upper_bound_B(vL) --
//   an A-element (value v, i-th of A) needs  lbA(v), ubB(v) and lbB(v);
//   a  B-element (value v, j-th of B) needs  lbA(v), ubA(v) and lbB(v);
//   lbB(v) of an A-element is the number of B-elements merged before it and
//   ubA(v) of a B-element the number of A-elements merged before it (A first
//   on ties): both fall out of the serial merge step.
// k_set_partition finds the three with the tile's split point, one thread per
// tile boundary (each is a single load when the run ends at the boundary).
//
//   k_set_partition  splits[t] (the merge's) and bounds[3 t ..]
//   k_set            one block per tile (tile id = blockIdx.x, as the scan:
//                    lookback.hpp's dispatch-order argument; ids from an
//                    atomic counter put a device-scope round trip in front
//                    of every tile's first load, 1.75 against 1.46 ms for the
//                    2^27 + 2^27 u64 union, profiles/set_ops_ubench*.log):
//                    stage both runs in LDS, per-thread diagonal search and
//                    an 8-step serial merge that also classifies each
//                    element: kept, dropped, or `slow` when equal elements of
//                    the other range exist -- those take galloping searches
//                    in LDS for the run bounds; the tile's kept count goes
//                    through a decoupled look-back (two_level_prefix), the
//                    kept elements are compacted in LDS in merged order and
//                    stored from the output's next 128-B line with 16-B
//                    stores.  out == nullptr: count only -- no offsets are
//                    needed, so the tiles add their counts to *count_dev
//                    (zeroed by the launcher) and skip the look-back.
// Unsorted input: the split points are clamped as in k_merge (device error
// word HPXHIP_DEVERR_RANGE); every other quantity only feeds keep flags, and
// the output offset is clamped to the tile's merged offset, so nothing is
// read or written outside the ranges and out[0, n1 + n2).
#pragma once

#include <hpxhip/kernels/common.hpp>
#include <hpxhip/kernels/lookback.hpp>
#include <hpxhip/kernels/merge_kernel.hpp>

namespace hpxhip {
namespace set_detail {

using merge_detail::kItems;
using merge_detail::kThreads;
using merge_detail::kTile;  // merged elements per tile
using merge_detail::not_after;
using merge_detail::path_split;
using merge_detail::stage;
using merge_detail::vec_elems;

enum : int { kUnion = 0, kIntersection = 1, kDifference = 2, kSymmetricDifference = 3 };

// first index in [lo, hi) of sorted a[] whose element is not before v
template <typename T, typename I, typename Less>
__device__ __forceinline__ I lower_bound_in(const T* a, I lo, I hi, const T& v, const Less& less) {
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (less(a[mid], v)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// ... whose element is after v
template <typename T, typename I, typename Less>
__device__ __forceinline__ I upper_bound_in(const T* a, I lo, I hi, const T& v, const Less& less) {
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (!less(v, a[mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// The same, galloping from the end the answer is near: lower bound of v in
// a[lo, hi) when a[hi - 1], a[hi - 2], ... are probed first (every element of
// a[lo, hi) is <= v's successors: the caller knows a[hi] is not before v).
template <typename T, typename Less>
__device__ __forceinline__ int gallop_lower(const T* a, int lo, int hi, const T& v, const Less& less) {
    int h = hi, step = 1;
    while (h - step >= lo && !less(a[h - step], v)) {
        h -= step;
        step <<= 1;
    }
    // a[h] is not before v (or h == hi); a[h - step] is, or lies below lo
    return lower_bound_in(a, h - step >= lo ? h - step + 1 : lo, h, v, less);
}
// upper bound of v in a[lo, hi), probing a[lo], a[lo + 1], a[lo + 3], ...
template <typename T, typename Less>
__device__ __forceinline__ int gallop_upper(const T* a, int lo, int hi, const T& v, const Less& less) {
    int l = lo, step = 1;
    while (l + step <= hi && !less(v, a[l + step - 1])) {
        l += step;
        step <<= 1;
    }
    // every element below l is not after v; a[l + step - 1] is, or lies past hi
    return upper_bound_in(a, l, l + step <= hi ? l + step - 1 : hi, v, less);
}

constexpr int kBoundsPerTile = 3;  // lbA(vF), lbB(vF) of tile t; ubB(vL) of tile t - 1

// One thread per tile boundary t (merged offset d = t * kTile): the merge's
// split point and, for the runs that cross the boundary, the bounds the two
// neighbouring tiles cannot see.
template <typename T, typename Less>
__global__ __launch_bounds__(256) void k_set_partition(const T* __restrict__ a, uint64_t na, const T* __restrict__ b,
                                                        uint64_t nb, uint64_t ntiles, Less less,
                                                        uint64_t* __restrict__ splits, uint64_t* __restrict__ bounds) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t > ntiles) return;
    const uint64_t total = na + nb;
    const uint64_t d = t * kTile < total ? t * kTile : total;
    const uint64_t sa = path_split(a, na, b, nb, d, less);
    const uint64_t sb = d - sa;
    splits[t] = sa;
    uint64_t lba = sa, lbb = sb, ubb = sb;
    if (t < ntiles) {  // d < total: tile t has a first element
        const bool from_a = sa < na && (sb >= nb || !less(b[sb], a[sa]));
        const T vf = from_a ? a[sa] : b[sb];
        // every element before the boundary is not after vf
        if (sa > 0 && !less(a[sa - 1], vf)) lba = lower_bound_in(a, uint64_t{0}, sa - 1, vf, less);
        if (sb > 0 && !less(b[sb - 1], vf)) lbb = lower_bound_in(b, uint64_t{0}, sb - 1, vf, less);
    }
    if (t > 0) {  // d > 0: tile t - 1 has a last element
        const bool from_b = sb > 0 && (sa == 0 || !less(b[sb - 1], a[sa - 1]));
        const T vl = from_b ? b[sb - 1] : a[sa - 1];
        // every element behind the boundary is not before vl
        if (sb < nb && !less(vl, b[sb])) ubb = upper_bound_in(b, sb + 1, nb, vl, less);
    }
    bounds[t * kBoundsPerTile + 0] = lba;
    bounds[t * kBoundsPerTile + 1] = lbb;
    bounds[t * kBoundsPerTile + 2] = ubb;
}

// stage[0, cnt) -> o[0, cnt) by the block: single elements up to o's next
// 128-B line, whole 16-B nontemporal vectors, a tail (compaction_kernel.hpp
// store_run, for this block size); VEC: o is element-aligned in a 16-B
// aligned buffer, else element stores.
template <typename T, bool VEC>
__device__ __forceinline__ void store_kept(T* o, const T* stg, uint32_t cnt) {
    constexpr int V = vec_elems<T>();
    if constexpr (VEC && V > 1) {
        using VT = vec<T, V>;
        const uint32_t head =
            min(cnt, static_cast<uint32_t>(((128u - (reinterpret_cast<uintptr_t>(o) & 127u)) & 127u) / sizeof(T)));
        const uint32_t nvec = (cnt - head) / V;
        for (uint32_t e = threadIdx.x; e < head; e += kThreads) o[e] = stg[e];
        for (uint32_t q = threadIdx.x; q < nvec; q += kThreads) {
            VT w;
#pragma unroll
            for (int e = 0; e < V; ++e) w.v[e] = stg[head + q * V + e];
            st_stream(reinterpret_cast<VT*>(o + head) + q, w);
        }
        for (uint32_t e = head + nvec * V + threadIdx.x; e < cnt; e += kThreads) o[e] = stg[e];
    } else {
        for (uint32_t e = threadIdx.x; e < cnt; e += kThreads) o[e] = stg[e];
    }
}

// The tile's output offset: the kept counts of every earlier tile, through a
// two-level look-back without a serial chain of hand-offs.  A merge tile is
// 2048 elements, so 2^28 keys are 131072 tiles: the fixed-association
// look-back's E(g) chain (lookback.hpp: one hand-off per 64 tiles, each
// waiting for the one before) is then 2048 links of ~1.3 us and bounds the
// kernel at ~2.7 ms whatever the operation writes (measured).
// Here tiles form groups of 64 and groups supergroups of 64 (4096 tiles):
//   tiles.aggregate(t)      the tile's kept count, published by the tile
//   groups.aggregate(g)     the sum over group g's tiles, published by the
//                           first tile of group g + 1 from those 64 counts --
//                           it depends on no prefix
//   groups.inclusive(64 G)  E2(G), the sum over every tile before supergroup
//                           G: E2(G - 1) plus the 64 group sums of supergroup
//                           G - 1, published by supergroup G's first tile:
//                           the only chain, one link per 4096 tiles
// and tile t of group g (supergroup G) takes E2(G) + the group sums of G's
// groups before g + the counts of g's tiles before t: three sets of slots,
// polled together.  Every wait is on a slot that a tile with a lower id
// publishes (workgroups are dispatched in id order, lookback.hpp), is bounded
// (kSpinLimit) and raises the device error word.  Integer sums: the
// order of the folds does not matter.
struct two_level_prefix {
    using state = tile_state<uint64_t>;
    static constexpr uint64_t kGroup = 64;
    state tiles, groups;

    // slot `which` (0 aggregate, 1 inclusive) of entry j
    __device__ __forceinline__ static bool try_slot(const state& st, uint64_t j, int which, uint64_t* v) {
        const uint64_t* p = st.slots + (j * 2 + which) * state::G;
        const uint32_t status = which ? TILE_INCLUSIVE : TILE_AGGREGATE;
        const uint64_t g0 = __hip_atomic_load(&p[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t g1 = __hip_atomic_load(&p[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (static_cast<uint32_t>(g0 >> 32) != status || static_cast<uint32_t>(g1 >> 32) != status) return false;
        const uint32_t w[2] = {static_cast<uint32_t>(g0), static_cast<uint32_t>(g1)};
        *v = from_words<uint64_t>(w);
        return true;
    }

    // Per lane: the sum of up to three slots (wanted: want[i]), all polled
    // together until published.  False on timeout.
    __device__ __forceinline__ bool wait_sum(const bool (&want)[3], const uint64_t (&j)[3], uint64_t* sum) const {
        bool pending[3] = {want[0], want[1], want[2]};
        uint64_t acc = 0;
        uint32_t spins = 0;
        while (true) {
            uint64_t v[3] = {0, 0, 0};
            bool got[3] = {false, false, false};
            if (pending[0]) got[0] = try_slot(groups, j[0], 0, &v[0]);
            if (pending[1]) got[1] = try_slot(tiles, j[1], 0, &v[1]);
            if (pending[2]) got[2] = try_slot(groups, j[2], 1, &v[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (got[i]) {
                    acc += v[i];
                    pending[i] = false;
                }
            if (!(pending[0] || pending[1] || pending[2])) break;
            __builtin_amdgcn_s_sleep(HPXHIP_LB_SLEEP);
            if (++spins > kSpinLimit) return false;
        }
        *sum = acc;
        return true;
    }

    // Called by ALL 64 lanes of one wave after the tile's count was
    // published (tile 0: also groups.inclusive(0) = 0); t > 0.  Returns the
    // kept count of every earlier tile on every lane (0 after a timeout).
    __device__ __forceinline__ uint64_t exclusive(uint64_t t) const {
        const uint64_t lane = static_cast<uint64_t>(lane_id());
        const uint64_t g = t / kGroup, pos = t % kGroup;
        const uint64_t sg0 = g / kGroup * kGroup, gpos = g % kGroup;  // the supergroup's first group
        bool ok = true;
        if (pos == 0) {  // a group's first tile: the sum of the group before
            uint64_t a = 0;
            ok = wait_sum({false, true, false}, {0, t - kGroup + lane, 0}, &a);
            const uint64_t ga = wave_reduce(a, op_plus{});
            if (lane == 0) groups.publish(g - 1, ga, TILE_AGGREGATE);
            if (gpos == 0 && __all(ok)) {  // a supergroup's first tile: E2
                uint64_t b = 0;
                ok = wait_sum({lane + 1 < kGroup, false, lane == 0}, {g - kGroup + lane, 0, g - kGroup}, &b);
                const uint64_t e2 = wave_reduce(b, op_plus{}) + ga;  // (lane 63's group sum is ga itself)
                if (__all(ok) && lane == 0) groups.publish(g, e2, TILE_INCLUSIVE);
            }
        }
        uint64_t c = 0;
        if (__all(ok)) ok = wait_sum({lane < gpos, lane < pos, lane == 0}, {sg0 + lane, g * kGroup + lane, sg0}, &c);
        if (!__all(ok)) {
            if (lane == 0) raise_device_error(tiles.err, HPXHIP_DEVERR_LOOKBACK_TIMEOUT);
            return 0;
        }
        return wave_reduce(c, op_plus{});
    }
};

// One block per kTile elements of the merged order of a[0, na), b[0, nb).
// VEC: a, b and out 16-B aligned.  st (zeroed) is the look-back state;
// *count_dev <- the kept elements.
template <typename T, typename Less, bool VEC>
__global__ __launch_bounds__(kThreads) void k_set(const T* __restrict__ a, uint64_t na, const T* __restrict__ b,
                                                   uint64_t nb, const uint64_t* __restrict__ splits,
                                                   const uint64_t* __restrict__ bounds, int op, Less less,
                                                   T* __restrict__ out, uint64_t* __restrict__ count_dev,
                                                   two_level_prefix st, uint64_t ntiles,
                                                   uint32_t* __restrict__ err) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ T s[kTile];
    __shared__ uint32_t s_wave_total[kWaves];
    __shared__ uint64_t s_prefix;
    const uint64_t t = blockIdx.x;
    const uint64_t total = na + nb;
    const uint64_t d0 = t * kTile;
    const uint64_t d1 = d0 + kTile < total ? d0 + kTile : total;
    // clamped as in k_merge: consistent splits pass unchanged
    const uint64_t s0 = splits[t], s1 = splits[t + 1];
    const uint64_t a1 = min(s1, min(na, d1));
    const uint64_t a0 = min(s0, min(a1, d0));
    const uint64_t b0 = min(d0 - a0, nb), b1 = max(b0, min(d1 - a1, nb));
    if (threadIdx.x == 0 && (a0 != s0 || a1 != s1 || b0 != d0 - a0 || b1 != d1 - a1))
        raise_device_error(err, HPXHIP_DEVERR_RANGE);
    const int la = static_cast<int>(a1 - a0), lb = static_cast<int>(b1 - b0);
    const int len = la + lb;
    const uint64_t f_lba = bounds[t * kBoundsPerTile + 0];
    const uint64_t f_lbb = bounds[t * kBoundsPerTile + 1];
    const uint64_t l_ubb = bounds[(t + 1) * kBoundsPerTile + 2];
    stage<T, VEC>(a, a0, a1, s);
    stage<T, VEC>(b, b0, b1, s + la);
    __syncthreads();
    const T* sa = s;
    const T* sb = s + la;

    uint32_t keep = 0;   // bit k: this thread's k-th merged element is kept
    uint32_t bmask = 0;  // bit k: it comes from b
    T r[kItems];
    const int dk = min(static_cast<int>(threadIdx.x) * kItems, len);
    if (len > 0) {  // (always: a tile is not empty; guards the reads of vF / vL)
        // the tile's first and last merged value
        const T vf = (la > 0 && (lb == 0 || !less(sb[0], sa[0]))) ? sa[0] : sb[0];
        const T vl = (lb > 0 && (la == 0 || !less(sb[lb - 1], sa[la - 1]))) ? sb[lb - 1] : sa[la - 1];
        int lo = dk > lb ? dk - lb : 0, hi = dk < la ? dk : la;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (not_after(sa[mid], sb[dk - mid - 1], less)) lo = mid + 1;
            else hi = mid;
        }
        const int ia0 = lo, ib0 = dk - lo;
        int ia = ia0, ib = ib0;
        const bool keep_a = op == kUnion, drop_b = op == kIntersection || op == kDifference;
        const bool inter = op == kIntersection;
        // the merge step of merge_in_lds; pa: the a-element before a's head
        T va = s[ia < la ? ia : 0];
        T vb = s[la + ib < len ? la + ib : 0];
        T pa = s[ia > 0 ? ia - 1 : 0];
        uint32_t slow = 0;  // bit k: equal elements of the other range exist, ranks decide
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const bool valid = dk + k < len;
            const bool takeb = ib < lb && (ia >= la || less(vb, va));
            // an a-element: equal b-elements follow it -- b's head, or (b's
            // part of the tile used up) behind the tile, the run of vL only
            const bool has_b = ib < lb ? !less(va, vb) : !less(va, vl);
            // a b-element: equal a-elements precede it -- the a-element just
            // before a's head, or (none in the tile yet) before the tile, the
            // run of vF only
            const bool has_a = ia > 0 ? !less(pa, vb) : !less(vf, vb);
            const bool other = takeb ? has_a : has_b;
            const bool fixed = takeb ? drop_b : keep_a;  // the op decides without ranks
            const bool kp = takeb ? (!drop_b && !has_a) : (keep_a || (!has_b && !inter));
            r[k] = takeb ? vb : va;
            keep |= static_cast<uint32_t>(valid && kp) << k;
            slow |= static_cast<uint32_t>(valid && !fixed && other) << k;
            bmask |= static_cast<uint32_t>(valid && takeb) << k;
            pa = takeb ? pa : va;
            ia += takeb ? 0 : 1;
            ib += takeb ? 1 : 0;
            const int ni = takeb ? la + ib : ia;
            const T nv = s[ni < len ? ni : 0];
            va = takeb ? va : nv;
            vb = takeb ? nv : vb;
        }
        // rank against the other range's count, bounds from LDS; a run that
        // reaches the tile's edge is vF's or vL's and takes the global bound
        while (slow) {
            const int k = __builtin_ctz(slow);
            slow &= slow - 1;
            const bool isb = (bmask >> k) & 1u;
            const int nbk = __builtin_popcount(bmask & ((1u << k) - 1u));
            const int ja = ia0 + (k - nbk), jb = ib0 + nbk;  // a- and b-elements merged before it
            const T v = isb ? sb[jb] : sa[ja];
            const bool eqf = !less(vf, v), eql = !less(v, vl);
            const int l = gallop_lower(sa, 0, ja, v, less);
            const uint64_t lba = (l == 0 && eqf) ? f_lba : a0 + static_cast<uint64_t>(l);
            bool kp;
            if (!isb) {
                const int u = gallop_upper(sb, jb, lb, v, less);
                const uint64_t ubb = (u == lb && eql) ? l_ubb : b0 + static_cast<uint64_t>(u);
                const uint64_t cntb = ubb - (b0 + static_cast<uint64_t>(jb));
                const uint64_t ka = a0 + static_cast<uint64_t>(ja) - lba;
                kp = inter ? ka < cntb : ka >= cntb;
            } else {
                const int l2 = gallop_lower(sb, 0, jb, v, less);
                const uint64_t lbb = (l2 == 0 && eqf) ? f_lbb : b0 + static_cast<uint64_t>(l2);
                const uint64_t cnta = a0 + static_cast<uint64_t>(ja) - lba;
                const uint64_t kb = b0 + static_cast<uint64_t>(jb) - lbb;
                kp = kb >= cnta;
            }
            keep |= static_cast<uint32_t>(kp) << k;
        }
    }

    // the tile's kept count and this thread's place in it
    const int wave = threadIdx.x / kWave, lane = lane_id();
    const uint32_t mine = static_cast<uint32_t>(__builtin_popcount(keep));
    const uint32_t incl = wave_inclusive_scan(mine, op_plus{});
    if (lane == kWave - 1) s_wave_total[wave] = incl;
    __syncthreads();  // wave totals; every thread is done with the staged runs
    uint32_t pos = incl - mine, agg = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) pos += s_wave_total[w];
        agg += s_wave_total[w];
    }
    if (!out) {  // count only (uniform): integer sums, any order
        if (threadIdx.x == 0 && agg)
            __hip_atomic_fetch_add(count_dev, static_cast<uint64_t>(agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (t > 0 && threadIdx.x == 0) st.tiles.publish(t, static_cast<uint64_t>(agg), TILE_AGGREGATE);
#pragma unroll
    for (int k = 0; k < kItems; ++k)
        if ((keep >> k) & 1u) s[pos++] = r[k];
    if (wave == 0) {
        uint64_t p = 0;
        if (t == 0) {
            if (lane == 0) {
                st.tiles.publish(0, static_cast<uint64_t>(agg), TILE_AGGREGATE);
                st.groups.publish(0, uint64_t{0}, TILE_INCLUSIVE);  // E2(0): nothing before the input
            }
        } else {
            p = st.exclusive(t);
        }
        if (lane == 0) {
            s_prefix = p;
            if (t == ntiles - 1) *count_dev = p + agg;
        }
    }
    __syncthreads();  // the kept elements are in LDS, the tile's output offset is known
    // at most d0 elements are kept before the tile, also after a look-back
    // timeout (0): the run stays inside out[0, na + nb)
    const uint64_t P = s_prefix < d0 ? s_prefix : d0;
    store_kept<T, VEC>(out + P, s, agg);
}

// ---------------------------------------------------------------- host side
// Scratch of one call: [tile slots | group slots | splits | bounds];
// launch() zeroes the slots.
constexpr size_t kSlotsOff = 0;
inline uint64_t ntiles_for(uint64_t total) { return (total + kTile - 1) / kTile; }
inline uint64_t ngroups_for(uint64_t total) { return ntiles_for(total) / two_level_prefix::kGroup + 1; }
inline size_t group_slots_off(uint64_t total) {
    return kSlotsOff + ntiles_for(total) * tile_state<uint64_t>::bytes_per_tile();
}
inline size_t splits_off(uint64_t total) {
    return (group_slots_off(total) + ngroups_for(total) * tile_state<uint64_t>::bytes_per_tile() + 255) / 256 * 256;
}
inline size_t bounds_off(uint64_t total) {
    return (splits_off(total) + (ntiles_for(total) + 1) * sizeof(uint64_t) + 255) / 256 * 256;
}
inline size_t scratch_bytes(uint64_t total) {
    return (bounds_off(total) + (ntiles_for(total) + 1) * kBoundsPerTile * sizeof(uint64_t) + 255) / 256 * 256;
}

// Queue op on (a[0, na), b[0, nb)) -> out (null: count only) on s;
// *count_dev <- the kept elements.  ws: scratch_bytes(na + nb) of scratch,
// err_word: the device error word.
template <typename T, typename Less>
hipError_t launch(const T* a, uint64_t na, const T* b, uint64_t nb, T* out, int op, Less less, uint64_t* count_dev,
                  void* ws, uint32_t* err_word, hipStream_t s) {
    const uint64_t total = na + nb;
    if (total == 0) return hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s);
    const uint64_t ntiles = ntiles_for(total);
    char* base = static_cast<char*>(ws);
    hipError_t e = out ? hipMemsetAsync(base, 0, splits_off(total), s) : hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    auto* splits = reinterpret_cast<uint64_t*>(base + splits_off(total));
    auto* bounds = reinterpret_cast<uint64_t*>(base + bounds_off(total));
    hipLaunchKernelGGL((k_set_partition<T, Less>), dim3(static_cast<unsigned>((ntiles + 1 + 255) / 256)), dim3(256), 0,
                       s, a, na, b, nb, ntiles, less, splits, bounds);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    two_level_prefix st{{reinterpret_cast<uint64_t*>(base + kSlotsOff), err_word},
                        {reinterpret_cast<uint64_t*>(base + group_slots_off(total)), err_word}};
    const bool aligned =
        (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    if (aligned)
        hipLaunchKernelGGL((k_set<T, Less, true>), dim3(static_cast<unsigned>(ntiles)), dim3(kThreads), 0, s, a, na, b,
                           nb, splits, bounds, op, less, out, count_dev, st, ntiles, err_word);
    else
        hipLaunchKernelGGL((k_set<T, Less, false>), dim3(static_cast<unsigned>(ntiles)), dim3(kThreads), 0, s, a, na,
                           b, nb, splits, bounds, op, less, out, count_dev, st, ntiles, err_word);
    return hipGetLastError();
}

}  // namespace set_detail
}  // namespace hpxhip
