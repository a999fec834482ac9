// reduce_by_key_kernel.hpp -- single-pass segmented reduction
// (hpx::parallel::reduce_by_key, reduce_by_key.hpp:586).  Header so that the
// C++ layer instantiates exactly this kernel with user callables
// (hpx/parallel/detail/device_algorithms.hpp).
//
// A run is a maximal range of consecutive equal keys; run j gives
// keys_out[j] = its first key and values_out[j] = its values folded left to
// right with an operator that is only assumed associative.  The reference
// makes three passes: key states (reduce_by_key.hpp:294-334), an inclusive
// scan over (value, state) tuples into an n-element output (:360-390) and a
// zipped copy_if (:399-411).  Here: one pass, each key and value read once,
// one pair written per run.
//
//   heads    Position i in [1, n] is a CLOSING HEAD when i == n or
//            keys[i] != keys[i-1]: the run that ends at i-1 closes there.
//            The n-th position is virtual (no key, no value); with it every
//            run is closed by exactly one head, count = heads, and the run
//            still open at the end of the input needs no case of its own.
//            The grid has n / TILE + 1 tiles so that position n always lies
//            in a tile.  The neighbour key comes from the adjacent lane
//            (DPP), the previous round (readlane), the adjacent wave (LDS),
//            or one global load of keys[tile_start - 1] issued with the
//            tile's own loads.
//   fold     Every range of elements is summarised by seg<V> = (flags,
//            partial): "a head was seen" and the fold of the values after
//            the last head (of all values if none).  seg_op,
//            (f1,v1) o (f2,v2) = (f1|f2, f2 ? v2 : op(v1,v2)), is
//            associative, so lanes, waves and tiles fold it like any scan
//            operator; an EMPTY flag is its identity, so the user operator
//            never needs one (it sees a padded value only past the end of
//            the input, where nothing is stored).  The fold is lane-serial
//            over a lane's E elements, a DPP wave scan over the lanes
//            (seg_wave_scan: the flags travel as one ballot), a carry over
//            the wave's rounds, LDS over the waves.
//   lookback The tile publishes {heads in the tile, seg} through
//            tile_state (lookback.hpp), in the fixed-association form: the
//            result is a function of the input alone, bitwise reproducible.
//            Tile ids are blockIdx.x (forward progress: lookback.hpp); every
//            wait is bounded and raises the device error word.
//   write    With C = heads before i (exclusive, over all tiles), head i
//            stores values_out[C] = fold of the run it closes and, for
//            i < n, keys_out[C + 1] = keys[i]; keys_out[0] = keys[0]; head n
//            stores *count = C + 1.
//
// In place (keys_out == keys and/or values_out == values, exactly aliased;
// the reference's own test runs so, tests/unit/parallel/algorithms/
// reduce_by_key.cpp:162-168):
//   - C counts heads in [1, i), so C <= i - 1: an output position p is only
//     written from elements at index >= p (keys) or > p (values);
//   - a tile writes only after its look-back, and the look-back completes
//     only after every earlier tile has published;
//   - a tile publishes only after ALL of its loads are in registers, the
//     look-behind key included (the vmcnt(0) wait before the first barrier);
//   so no store can reach a position whose tile has not read it yet.  The
//   one position another tile may still read late is keys[tile_start - 1],
//   read by the tile AFTER the one that owns it: the only writer that can
//   run before that read is the owning tile, and it stores there only when
//   C + 1 == i, i.e. it stores keys[i] over itself.
// A pipelined or persistent form must keep these orderings.  Partial overlap
// is the caller's error.
#pragma once

#include <hpxhip/kernels/common.hpp>
#include <hpxhip/kernels/lookback.hpp>

namespace hpxhip {
namespace reduce_by_key_detail {

// Tile shape: 512 threads x 16 elements per lane = 8192 elements for every
// key / value width, two workgroups per CU (128 VGPRs), so one workgroup's
// look-back and write-out overlap the other's loads.  Measured at 2^28
// int64 / int64 pairs, runs of 128 (profiles/reduce_by_key_ubench.log,
// section 3): 1024 threads x 8 elements (one workgroup per CU) 1.52-1.63 ms,
// 1024 x 16 1.60, 512 x 8 1.72, 512 x 16 1.29-1.34, 256 x 16 1.95; 256 x 8
// (2048-element tiles, a look-back chain of 2048 group links) 3.23.
constexpr int kThreads = 512;
constexpr int kLaneElems = 16;  // per lane and tile: two bits each in a 32-bit word

// Elements per lane per round: the wider of key and value fills 16 bytes
// (the narrower of a mixed-width pair is loaded as 8-B vectors).
template <typename K, typename V>
constexpr int lane_elems() {
    return 16 / static_cast<int>(sizeof(K) > sizeof(V) ? sizeof(K) : sizeof(V));
}
// Rounds (vectors per lane) of the shipped shape.
template <typename K, typename V>
constexpr int rounds_for() {
    return kLaneElems / lane_elems<K, V>();
}
// Elements per tile (8192 for the shipped shape).
template <typename K, typename V, int ROUNDS = rounds_for<K, V>(), int THREADS = kThreads>
constexpr uint64_t tile_elems() {
    return static_cast<uint64_t>(THREADS) * ROUNDS * lane_elems<K, V>();
}
// Position n is a (virtual) head of its own: always one tile past n / TILE.
template <typename K, typename V, int ROUNDS = rounds_for<K, V>(), int THREADS = kThreads>
constexpr uint64_t ntiles_for(uint64_t n) {
    return n / tile_elems<K, V, ROUNDS, THREADS>() + 1;
}

enum : uint32_t { SEG_HEAD = 1, SEG_EMPTY = 2 };

template <typename V>
struct seg {
    V p;
    uint32_t f;
};

template <typename F>
struct seg_op {
    F f;
    template <typename V>
    __device__ __forceinline__ seg<V> operator()(seg<V> a, seg<V> b) const {
        if (b.f & SEG_EMPTY) return a;
        if ((b.f & SEG_HEAD) || (a.f & SEG_EMPTY)) return b;
        return seg<V>{static_cast<V>(f(a.p, b.p)), a.f};
    }
    template <typename X>
    __host__ __device__ static constexpr X identity() {
        return X{{}, SEG_EMPTY};
    }
};

// What a tile hands on: the heads it holds and the seg of its elements.
// CT: uint32_t while n < 2^32 (one granule less per slot), else uint64_t.
template <typename CT, typename V>
struct tile_value {
    CT count;
    uint32_t f;
    V p;
};

template <typename F>
struct tile_op {
    seg_op<F> s;
    template <typename CT, typename V>
    __device__ __forceinline__ tile_value<CT, V> operator()(tile_value<CT, V> a, tile_value<CT, V> b) const {
        const seg<V> r = s(seg<V>{a.p, a.f}, seg<V>{b.p, b.f});
        return tile_value<CT, V>{static_cast<CT>(a.count + b.count), r.f, r.p};
    }
    template <typename X>
    __host__ __device__ static constexpr X identity() {
        return X{0, SEG_EMPTY, {}};
    }
};

template <typename CT, typename V>
using state_t = tile_state<tile_value<CT, V>>;

// Inclusive segmented wave scan of the lanes' partials: lane l receives the
// fold of x over the lanes [s(l), l], s(l) = the last lane <= l whose bit is
// set in head_mask (lane 0 if none).  The flags travel as that one ballot, so
// the DPP steps move the partials alone.  The steps are those of
// wave_inclusive_scan_noid (common.hpp); a step's source lane src holds the
// fold over [max(s(src), lo), src], and lane l takes it when s(l) <= src --
// then no head lies in (src, l], so s(src) == s(l) and the two ranges join.
// Identity-free: a lane whose source lies outside its row / the wave keeps
// its value.  *seen: a head at a lane <= l.
template <typename V, typename F>
__device__ __forceinline__ V seg_wave_scan(V x, uint64_t head_mask, F f, bool* seen) {
    const int l = lane_id();
    const int r = l & 15;
    const uint64_t m = head_mask & ((uint64_t{2} << l) - 1);  // heads at lanes <= l
    const int s = m ? 63 - __builtin_clzll(m) : 0;
    *seen = m != 0;
    V acc = x;
    V t = static_cast<V>(f(dpp<DPP_ROW_SHR1>(x, x), x));
    acc = (r >= 1 && s <= l - 1) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_SHR2>(x, x), acc));
    acc = (r >= 2 && s <= l - 2) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_SHR3>(x, x), acc));
    acc = (r >= 3 && s <= l - 3) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_SHR4>(acc, acc), acc));
    acc = (r >= 4 && s <= l - 4) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_SHR8>(acc, acc), acc));
    acc = (r >= 8 && s <= l - 8) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_BCAST15>(acc, acc), acc));
    acc = ((l & 16) && s <= (l & ~15) - 1) ? t : acc;
    t = static_cast<V>(f(dpp<DPP_ROW_BCAST31>(acc, acc), acc));
    acc = (l >= 32 && s <= 31) ? t : acc;
    return acc;
}

__device__ __forceinline__ uint32_t rank_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// vec_ok: keys and values are aligned for E-element vector loads (a tile
// past the end of the input, or an unaligned range, loads element-wise).
template <typename K, typename V, typename Eq, typename F, typename CT, int ROUNDS = rounds_for<K, V>(),
          int THREADS = kThreads, int MINW = 4>
__global__ __launch_bounds__(THREADS, MINW) void k_reduce_by_key(const K* keys, const V* vals, K* keys_out,
                                                                 V* vals_out, uint64_t n, Eq eq, F f,
                                                                 uint64_t* count_dev, state_t<CT, V> st, int vec_ok) {
    constexpr int E = lane_elems<K, V>();
    constexpr int WAVES = THREADS / kWave;
    constexpr uint64_t TILE = tile_elems<K, V, ROUNDS, THREADS>();
    constexpr uint64_t WAVE_ELEMS = TILE / WAVES;
    using KV = vec<K, E>;
    using VV = vec<V, E>;
    using X = seg<V>;
    using TV = tile_value<CT, V>;
    static_assert(ROUNDS * E <= kLaneElems, "head and flag bits per lane");
    static_assert(sizeof(TV) % 4 == 0 && sizeof(TV) <= 32, "tile_state value");

    __shared__ K s_last_key[WAVES];
    __shared__ X s_wave_seg[WAVES];
    __shared__ uint32_t s_wave_heads[WAVES];
    __shared__ TV s_prefix;

    const seg_op<F> sop{f};
    const X sid = seg_op<F>::template identity<X>();
    const uint64_t tile = blockIdx.x;  // tile order = dispatch order (lookback.hpp)
    const int wave = threadIdx.x / kWave;
    const int lane = lane_id();
    const uint64_t tile_base = tile * TILE;
    const uint64_t wbase = tile_base + wave * WAVE_ELEMS;
    const bool full = vec_ok && tile_base + TILE <= n;

    // ---- loads: the tile's keys and values, and the key before the tile
    KV k[ROUNDS];
    VV v[ROUNDS];
    K behind{};
    if (threadIdx.x == 0 && tile_base > 0) behind = keys[tile_base - 1];
    if (full) {
        const KV* ks = reinterpret_cast<const KV*>(keys + wbase);
        const VV* vs = reinterpret_cast<const VV*>(vals + wbase);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) k[r] = ld_stream(&ks[r * kWave + lane]);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) v[r] = ld_stream(&vs[r * kWave + lane]);
    } else {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint64_t i = wbase + (static_cast<uint64_t>(r) * kWave + lane) * E + e;
                k[r].v[e] = i < n ? keys[i] : K{};
                v[r].v[e] = i < n ? vals[i] : V{};
            }
    }
    if (lane == kWave - 1) s_last_key[wave] = k[ROUNDS - 1].v[E - 1];
    // Every load of the tile is in registers before anything is published
    // (the in-place argument above).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (lane == 0 && wave > 0) behind = s_last_key[wave - 1];

    // ---- heads and the segmented fold of the wave's elements, in segment
    // order (round, lane, element).  v[r][e] becomes the seg of the wave's
    // elements BEFORE (r, lane, e): its partial in place, its flags in xf.
    uint32_t heads = 0;  // bit r*E+e
    uint32_t xf = 0;     // two bits per element
    X carry = sid;       // the wave's rounds so far
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        // key before the lane's first element: previous lane, previous round
        // (lane 0), previous wave or tile (lane 0 of round 0)
        K before = dpp<DPP_WAVE_SHR1>(behind, k[r].v[E - 1]);
        if (r > 0) {
            const K prev_round = readlane(k[r - 1].v[E - 1], kWave - 1);
            if (lane == 0) before = prev_round;
        }
        X run = sid;
        X ex[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint64_t i = wbase + (static_cast<uint64_t>(r) * kWave + lane) * E + e;
            const K prev = e == 0 ? before : k[r].v[e - 1];
            bool h;
            if (full) h = i > 0 && !eq(prev, k[r].v[e]);
            else h = i > 0 && (i == n || (i < n && !eq(prev, k[r].v[e])));
            heads |= static_cast<uint32_t>(h) << (r * E + e);
            ex[e] = run;
            // past the virtual head n there is nothing
            const uint32_t ef = (!full && i > n) ? uint32_t(SEG_EMPTY) : (h ? uint32_t(SEG_HEAD) : 0u);
            run = sop(run, X{v[r].v[e], ef});
        }
        // the lanes' (flags, partial) in lane order (a lane past the end of
        // the input holds no head and any partial: nothing after n is read)
        bool seen;
        const V incl_p = seg_wave_scan(run.p, __ballot((run.f & SEG_HEAD) != 0), f, &seen);
        const X incl{incl_p, seen ? uint32_t(SEG_HEAD) : 0u};
        const X lane_ex = sop(carry, wave_shift_right<X, seg_op<F>>(incl));
        carry = sop(carry, readlane(incl, kWave - 1));
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const X s = sop(lane_ex, ex[e]);
            v[r].v[e] = s.p;
            xf |= s.f << (2 * (r * E + e));
        }
    }
    const uint32_t wave_heads = wave_reduce(static_cast<uint32_t>(__builtin_popcount(heads)), op_plus{});
    if (lane == 0) {
        s_wave_seg[wave] = carry;
        s_wave_heads[wave] = wave_heads;
    }
    __syncthreads();
    X wave_ex = sid, tile_seg = sid;  // the tile's waves before this one; all of them
    uint32_t heads_before = 0, tile_heads = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const X ws = s_wave_seg[w];
        const uint32_t wh = s_wave_heads[w];
        if (w < wave) {
            wave_ex = sop(wave_ex, ws);
            heads_before += wh;
        }
        tile_seg = sop(tile_seg, ws);
        tile_heads += wh;
    }

    // ---- look-back (wave 0): the heads and the seg of every earlier tile
    if (wave == 0) {
        const tile_op<F> top{sop};
        const TV agg{static_cast<CT>(tile_heads), tile_seg.f, tile_seg.p};
        TV p = tile_op<F>::template identity<TV>();
        if (tile == 0) {
            if (lane == 0) {
                st.publish(0, agg, TILE_AGGREGATE);
                st.publish(0, p, TILE_INCLUSIVE);  // E(0): nothing before the input
            }
        } else {
            if (lane == 0) st.publish(tile, agg, TILE_AGGREGATE);
            p = st.template exclusive_prefix_fixed<false>(tile, top);
        }
        if (lane == 0) s_prefix = p;
    }
    __syncthreads();
    const TV prefix = s_prefix;
    const X before_wave = sop(X{prefix.p, prefix.f}, wave_ex);
    uint64_t c = static_cast<uint64_t>(prefix.count) + heads_before;  // heads before the wave

    // ---- write-out: head i closes the run that ends at i - 1
    if (tile == 0 && threadIdx.x == 0) keys_out[0] = k[0].v[0];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        uint32_t cnt = 0, below = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint64_t m = __ballot((heads >> (r * E + e)) & 1u);
            below += rank_below(m);
            cnt += static_cast<uint32_t>(__builtin_popcountll(m));
        }
        uint64_t rank = c + below;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if ((heads >> (r * E + e)) & 1u) {
                const uint64_t i = wbase + (static_cast<uint64_t>(r) * kWave + lane) * E + e;
                const X closed = sop(before_wave, X{v[r].v[e], (xf >> (2 * (r * E + e))) & 3u});
                vals_out[rank] = closed.p;
                if (i < n) keys_out[rank + 1] = k[r].v[e];
                else *count_dev = rank + 1;
                ++rank;
            }
        }
        c += cnt;
    }
}

}  // namespace reduce_by_key_detail
}  // namespace hpxhip
