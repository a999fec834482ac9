// compaction_kernel.hpp -- single-pass, stable stream compaction: the kernel
// and its host launcher for copy_if (one-sided), for partition_copy,
// stable_partition, remove_copy_if and remove_if (two-sided) and for
// unique_copy and unique (one-sided, adjacent mode); see
// hpx_amd/csrc/compaction.hip for the entry points.  Header so that the
// library and the device-closure layer (hpx/parallel/detail/
// device_algorithms.hpp) instantiate the same kernel through the same
// launcher, and scripts/ubench the same kernel at other shapes.
//
// Persistent and pipelined: one 1024-thread workgroup per CU walks tiles
// claimed in order from an atomic counter.  A tile is 1024 threads x 8 rounds
// x 16 B = 128 KiB, which is also the workgroup's LDS stage.  Per tile:
//   1. 16-B nontemporal loads (issued one tile ahead, below), the predicate's
//      hit bits in a register word;
//   2. wave totals -> the tile's count of accepted elements, published as the
//      tile's aggregate (lookback.hpp, fixed association);
//   3. `ballot` + `mbcnt` ranks into LDS: element j of the tile (index order)
//      with a accepted elements before it lands at stage[a] if accepted, so
//      the accepted ones fill [0, agg) in index order.  TWO_SIDED: a rejected
//      one lands at stage[agg + (j - a)], so the rejected ones fill
//      [agg, valid), in index order too;
//   4. the registers are free now: the NEXT tile's loads are issued;
//   5. the look-back gives P, the accepted count of every earlier tile (and
//      of a split-off head);
//   6. stage[0, agg) -> out_true[P ..); TWO_SIDED: stage[agg, valid) ->
//      out_false[head + tile_base - P ..): a tile has a known number of
//      elements, so the one look-back value places both sides.  Each side is
//      one contiguous run, stored as whole 16-B vectors from a 128-B boundary.
// So a CU's look-back and write-out run under its next tile's reads instead
// of between them: against one tile per workgroup, held in registers until
// its write-out (two such workgroups per CU fall into step), copy_if at 50 %
// hits went 2.13-2.14 -> 1.96-1.97 ms at 2^30 int64 and 2.26-2.28 -> 2.15 ms
// at 2^31 int32 (profiles/r05_ubench_copyif9.log).  Tiles are claimed in
// order, so every look-back waits only on tiles already claimed by running
// workgroups (forward progress without co-residency).
// One-sided (TWO_SIDED = false, compile-time: the two-sided kernel with one
// output absent costs 0.538 against 0.507 ms at 2^28 int64,
// profiles/partition_ubench.log): rejected elements are neither staged nor
// stored and out_false is ignored.  TWO_SIDED: either output may be null (a
// uniform run-time branch): that side is ranked and staged but not stored.
//
// Adjacent mode (ADJ = true, compile-time, one-sided; unique_copy, and unique
// with out == in): the predicate is a binary relation rel and the hit bit of
// element i is !rel(in[i - 1], in[i]); the range's first element has no
// element before it and is a hit.  Every element is compared with its
// immediate predecessor (std::unique_copy for equivalence relations; the
// reference compares with the last kept element).  The tile's index order is
// (wave, round, lane, element), wbase + (r * 64 + lane) * V + e, so the
// element before comes from
//   x[r].v[e - 1]                       for e > 0,
//   the previous lane's v[V - 1]        for e == 0 (DPP wave_shr:1),
//   lane 63 of round r - 1              for lane 0 (readlane),
//   in[wbase - 1]                       for lane 0 of round 0: one extra
//     element load per wave (lane 0), issued in load(t) in front of the wave's
//     vector loads -- the early next-tile load included -- and held in a
//     register until the hit bits are formed.  For wave 0 that is the last
//     element of the previous tile, for tile 0 behind a split-off head
//     in[-1], the head's last element.
// The other source of the previous wave's last element, a hand-over through
// LDS (lane 63 writes, a barrier, lane 0 of the next wave reads; only thread 0
// loads in[tile_base - 1]), puts a workgroup barrier in front of the hit bits.
// Both were measured (profiles/unique_ubench.log against
// unique_ubench_lds_handover.log); the load per wave is shipped.  Everything else -- tile claim, ranks, stage, pipelined
// load, look-back, store_run, the launcher -- is the code copy_if runs; the
// other instantiations compile to the same registers, spills and LDS as
// before (profiles/unique_resource_usage.txt).  A separate kernel was not
// needed.  Element-wise loads and partial tiles: a padded position is never a
// hit and never the element before a valid one (it lies behind all of them).
//
// Aliasing.  Each output may be exactly the input (not both; the outputs must
// not overlap each other).  This covers the one-sided form: copy_if with
// out == in is the out_true == in case.  Why no tile overwrites input that is
// still to be read:
//   (a) a tile learns P only after every earlier tile has published its
//       aggregate (the look-back folds them all);
//   (b) a tile publishes its aggregate only after its own loads have been
//       consumed: the aggregate is computed from the hit bits, which are
//       computed from the loaded values;
//   (c) an element's destination index never exceeds its source index, on
//       either side: the accepted element i goes to (accepted before i) <= i,
//       the rejected one to i - (accepted before i) <= i.
//   So tile t stores only below (t + 1) * TILE -- into its own range, which
//   it has wholly in LDS by then (the barrier before the write-out), and into
//   ranges of earlier tiles, which by (a) and (b) have consumed their loads.
//   Later tiles' input is never stored to by tile t.
//   The early load of step 4 reads the range of a tile u claimed after t.
//   Tiles before u never store at or above u * TILE (above); tiles after u
//   store only after their look-back, i.e. by (a) and (b) after u's loads
//   were consumed; u itself stores after its own barrier.  So the early load
//   sees the caller's values wherever it falls in time.
//   In place only [0, count) of the aliased output is stored; the elements
//   from the new end onward are not touched.
//   Adjacent mode, out_true == in (unique).  (a)-(c) hold unchanged: the
//   destination index is at most the source index.  New are the reads of
//   in[wbase - 1]:
//   - wave > 0: the element lies in the tile's own range, and the argument
//     for the tile's own loads covers it (early load included).
//   - wave 0 of tile u > 0 reads in[u * TILE - 1], which tile u - 1 owns.
//     A tile t < u - 1 stores only below (t + 1) * TILE <= (u - 1) * TILE.
//     Tile u - 1 stores below u * TILE, and by (c) the only element it can
//     store AT u * TILE - 1 is the one whose source is that index, when
//     nothing before it was dropped: the same bytes.  Tiles from u on store
//     only after their look-back, i.e. after u has published its aggregate,
//     and that aggregate depends on this load: it is the operand of element
//     0's hit bit, which enters the wave count, the tile count and so the
//     value given to st.publish.  The dependence is a data dependence in the
//     code below (bnd -> hit -> wave_count -> agg), not a convention.
//   - tile 0 behind a split-off head reads in[-1], the head's last element.
//     k_compact_head runs before this kernel on the same stream; in place it
//     stores out_true[c] with c <= i, so position h - 1 can only receive the
//     element h - 1 itself.  Within this kernel in[-1] lies below every
//     tile's range: tile 0 stores after its own barrier (B), later tiles
//     after tile 0 has published, both after the load was consumed.
//   The head kernel keeps the element before in a register, so its own
//   in-place stores (destination <= source) never feed a comparison.
#pragma once

#include <hpxhip/kernels/common.hpp>
#include <hpxhip/kernels/lookback.hpp>

namespace hpxhip {
namespace compaction_detail {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kRounds = 8;  // 16-B vectors per lane: the tile is 128 KiB

template <typename T, int ROUNDS = kRounds>
constexpr uint64_t tile_elems() {
    return static_cast<uint64_t>(kThreads) * ROUNDS * (16 / sizeof(T));
}
template <typename T, int ROUNDS = kRounds>
constexpr uint64_t ntiles_for(uint64_t n) {
    return (n + tile_elems<T, ROUNDS>() - 1) / tile_elems<T, ROUNDS>();
}

__device__ __forceinline__ uint32_t rank_below(uint64_t mask) {
    // number of set bits of `mask` in lanes below this lane
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// Hit bits of one lane: bit (r*V + e) for element e of round r.
template <int BITS>
using hit_word = std::conditional_t<(BITS <= 32), uint32_t, uint64_t>;

// stage[0, cnt) -> o[0, cnt) by the whole workgroup: single elements up to
// o's next ALIGN boundary, whole 16-B vectors, a tail.  16-B nontemporal
// stores: for 8-byte elements, against plain element stores, nontemporal ones
// took copy_if at 2^30 int64 2.182-2.199 -> 2.175-2.176 ms and 16-B ones
// 2.191-2.196 -> 2.183-2.185 (profiles/r04_ubench_copyif8.log,
// r04_ubench_copyif8_wide.log).  ALIGN = 128 (a cache
// line): each wave's 1-KiB store run covers whole lines, so two waves never
// write halves of one line -- against ALIGN = 16, copy_if at 2^30 int64
// WRITE_SIZE 1.02 -> 1.0015x the hits, 1.985 -> 1.96-1.97 ms
// (profiles/r05_ubench_copyif9_align128.log, r05_pmc_copy_if.txt).
template <typename T, int ROUNDS, int ALIGN>
__device__ __forceinline__ void store_run(T* o, const T* stage, uint32_t cnt) {
    constexpr int V = 16 / sizeof(T);
    using VT = vec<T, V>;
    constexpr uintptr_t AM = ALIGN - 1;
    const uint32_t head =
        cnt ? min(cnt, static_cast<uint32_t>(((ALIGN - (reinterpret_cast<uintptr_t>(o) & AM)) & AM) / sizeof(T))) : 0u;
    const uint32_t nvec = (cnt - head) / V;
    const uint32_t tail = cnt - head - nvec * V;
    if (threadIdx.x < head) o[threadIdx.x] = stage[threadIdx.x];
    else if (threadIdx.x >= 64 && threadIdx.x - 64 < tail) {
        const uint32_t j = head + nvec * V + (threadIdx.x - 64);
        o[j] = stage[j];
    }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const uint32_t q = k * kThreads + threadIdx.x;
        if (q < nvec) {
            VT w;
#pragma unroll
            for (int e = 0; e < V; ++e) w.v[e] = stage[head + q * V + e];
            st_stream(reinterpret_cast<VT*>(o + head) + q, w);
        }
    }
}

// in: n elements (ALIGNED: 16-B aligned; else every load is element-wise).
// head: elements of the caller's range in front of `in` that k_compact_head
// placed already, *prefix0 of them accepted (0 / null without a head).
// counter (zeroed) hands out the tile ids, st (zeroed) is the tile state.
// SV, the look-back value type: counts are at most n + head, so below 2^32
// elements they travel as 32-bit values, one granule per slot instead of two
// (copy_if at 2^30 int64 2.55 -> 2.32 ms, profiles/r01_ubench_copyif_state.log).
// The look-back is the fixed-association one (copy_if 2.34 -> 2.20-2.21 ms,
// profiles/r03_ubench_copyif7.log) in its one-hop form (2.176-2.184 ->
// 2.138-2.146 ms, profiles/r04_ubench_lookback_onehop.log).
// *count_dev <- accepted elements, the head's included.
// Grid: at most one workgroup per CU, at most ntiles.
// ADJ (one-sided only): pred is a binary relation and element i is accepted
// iff it has no element before it or !pred(in[i - 1], in[i]) (the head note
// above); in[-1] is read when head > 0.
template <typename T, typename Pred, bool ALIGNED, typename SV, bool TWO_SIDED, int MINW = 4, int ROUNDS = kRounds,
          int OUT_ALIGN = 128, bool ADJ = false>
__global__ __launch_bounds__(kThreads, MINW) void k_compact(const T* in, T* out_true, T* out_false, uint64_t n,
                                                            uint64_t head, Pred pred, uint64_t* count_dev,
                                                            uint32_t* counter, tile_state<SV> st, uint64_t ntiles,
                                                            const uint64_t* prefix0) {
    constexpr int V = 16 / sizeof(T);
    constexpr uint32_t TILE = static_cast<uint32_t>(tile_elems<T, ROUNDS>());
    constexpr uint32_t WAVE_ELEMS = TILE / kWaves;
    using VT = vec<T, V>;
    using H = hit_word<ROUNDS * V>;
    static_assert(ROUNDS * V <= 64, "hit bits per lane");
    static_assert(!(ADJ && TWO_SIDED), "the adjacent mode is one-sided");

    __shared__ T s_stage[TILE];
    __shared__ uint32_t s_wave_total[kWaves];
    __shared__ uint32_t s_next;
    __shared__ uint64_t s_prefix;

    const int wave = threadIdx.x / kWave;
    const int lane = lane_id();
    const uint32_t wlocal = wave * WAVE_ELEMS;  // the wave's first element in the tile
    auto claim = [&] {
        if (threadIdx.x == 0)
            s_next = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    VT x[ROUNDS];
    [[maybe_unused]] T bnd{};  // ADJ, lane 0: the element before the wave's first
    auto load = [&](uint64_t t) {
        const uint64_t wbase = t * TILE + wlocal;
        if constexpr (ADJ) {
            // the previous wave's, the previous tile's or the head's last
            // element; issued with the wave's own loads, held until the hit bits
            if (lane == 0 && wbase < n && (wbase > 0 || head > 0)) bnd = (in + wbase)[-1];
        }
        if (ALIGNED && wbase + WAVE_ELEMS <= n) {
            const VT* src = reinterpret_cast<const VT*>(in + wbase);
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) x[r] = ld_stream(&src[r * kWave + lane]);
        } else {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const uint64_t i = wbase + (static_cast<uint64_t>(r) * kWave + lane) * V + e;
                    x[r].v[e] = i < n ? in[i] : T(0);
                }
        }
    };

    claim();
    __syncthreads();
    uint64_t tile = s_next;
    if (tile >= ntiles) return;
    load(tile);
    while (true) {
        const uint64_t tile_base = tile * TILE;
        const uint64_t wbase = tile_base + wlocal;
        // Elements of the tile inside the input.  The two-sided form needs the
        // count for its rejected side and bounds the hit bits with it, per
        // tile; the one-sided form needs no count and tests per wave against
        // n.  (The per-wave test in the two-sided form moves its VGPR spills
        // from the 4-byte kernels onto the 8-byte any_bits ones, 0 -> 4.)
        [[maybe_unused]] uint32_t valid = TILE;
        if constexpr (TWO_SIDED) valid = n - tile_base < TILE ? static_cast<uint32_t>(n - tile_base) : TILE;
        auto inside = [&](int r, int e) {
            if constexpr (TWO_SIDED) return wlocal + (r * kWave + lane) * V + e < valid;
            else return wbase + (static_cast<uint64_t>(r) * kWave + lane) * V + e < n;
        };
        H hit = 0;
        if constexpr (ADJ) {
            // The element before (r, lane, e) in index order: x[r].v[e - 1];
            // e == 0: the previous lane's last (DPP wave_shr:1); lane 0: lane
            // 63 of the previous round; lane 0 of round 0: bnd.  The range's
            // first element has none and is kept.  A padded position is never
            // a hit, and none precedes a valid element (index order).
            const bool first = head == 0 && wbase == 0 && lane == 0;
            auto adjacent_hits = [&](auto bounded) {
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r) {
                    T old = bnd;
                    if (r > 0) old = readlane(x[r - 1].v[V - 1], kWave - 1);
                    const T before = dpp<DPP_WAVE_SHR1>(old, x[r].v[V - 1]);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        bool h = !pred(e == 0 ? before : x[r].v[e > 0 ? e - 1 : 0], x[r].v[e]);
                        if (r == 0 && e == 0) h = h || first;
                        if constexpr (decltype(bounded)::value) h = h && inside(r, e);
                        hit |= static_cast<H>(h) << (r * V + e);
                    }
                }
            };
            if (wbase + WAVE_ELEMS <= n) adjacent_hits(std::false_type{});
            else adjacent_hits(std::true_type{});
        } else if (TWO_SIDED ? valid == TILE : wbase + WAVE_ELEMS <= n) {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
                for (int e = 0; e < V; ++e) hit |= static_cast<H>(pred(x[r].v[e])) << (r * V + e);
        } else {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
#pragma unroll
                for (int e = 0; e < V; ++e) hit |= static_cast<H>(inside(r, e) && pred(x[r].v[e])) << (r * V + e);
        }
        const uint32_t wave_count = wave_reduce(static_cast<uint32_t>(__builtin_popcountll(hit)), op_plus{});
        if (lane == 0) s_wave_total[wave] = wave_count;
        claim();
        __syncthreads();  // (A) wave totals, the next tile id; the last tile's write-out has left the stage
        uint32_t wave_prefix = 0, agg = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) wave_prefix += s_wave_total[w];
            agg += s_wave_total[w];
        }
        // (b) of the aliasing argument: agg depends on every load of the tile
        if (tile > 0 && threadIdx.x == 0) st.publish(tile, static_cast<SV>(agg), TILE_AGGREGATE);

        // Into LDS in index order (round, lane, element): the accepted
        // elements, and behind them the rejected ones if they are wanted.
        uint32_t acc = wave_prefix;  // accepted elements of the tile before this wave round
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            uint32_t cnt = 0, below = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint64_t m = __ballot((hit >> (r * V + e)) & 1u);
                below += rank_below(m);
                cnt += static_cast<uint32_t>(__builtin_popcountll(m));
            }
            uint32_t a = acc + below;  // accepted before this lane's element e
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool h = (hit >> (r * V + e)) & 1u;
                if (h) s_stage[a] = x[r].v[e];
                else if constexpr (TWO_SIDED) {
                    const uint32_t j = wlocal + (r * kWave + lane) * V + e;
                    if (j < valid) s_stage[agg + (j - a)] = x[r].v[e];
                }
                a += h;
            }
            acc += cnt;
        }
        const uint64_t next = s_next;
        __syncthreads();  // (B) the whole tile is in LDS; x is free
        if (next < ntiles) load(next);
        if (wave == 0) {
            SV p = 0;
            if (tile == 0) {
                if (prefix0) p = static_cast<SV>(*prefix0);
                if (lane == 0) {
                    st.publish(0, static_cast<SV>(agg), TILE_AGGREGATE);
                    st.publish(0, p, TILE_INCLUSIVE);
                }
            } else {
                p = st.template exclusive_prefix_fixed<true>(tile, op_plus{});
            }
            if (lane == 0) {
                s_prefix = p;
                if (tile == ntiles - 1) *count_dev = static_cast<uint64_t>(p) + agg;
            }
        }
        __syncthreads();  // (C) the tile's output offsets
        if constexpr (TWO_SIDED) {
            // P <= head + tile_base (it counts elements before the tile), also
            // after a look-back timeout (P = 0): both runs stay inside the outputs.
            const uint64_t P = s_prefix < head + tile_base ? s_prefix : head + tile_base;
            if (out_true) store_run<T, ROUNDS, OUT_ALIGN>(out_true + P, s_stage, agg);
            if (out_false)
                store_run<T, ROUNDS, OUT_ALIGN>(out_false + (head + tile_base - P), s_stage + agg, valid - agg);
        } else {
            store_run<T, ROUNDS, OUT_ALIGN>(out_true + s_prefix, s_stage, agg);
        }
        if (next >= ntiles) break;
        tile = next;
    }
}

// Head of a misaligned input (fewer than 16 B of elements), placed by one
// thread: accepted -> out_true[0..c), rejected -> out_false[0..h - c),
// c -> *count; a null output is skipped.  In place: both destinations trail
// the source index.  ADJ: accepted iff i == 0 or !pred(in[i - 1], in[i]); the
// element before is kept in a register, so in place it is the caller's value.
template <typename T, typename Pred, bool ADJ = false>
__global__ void k_compact_head(const T* in, T* out_true, T* out_false, uint64_t h, Pred pred, uint64_t* count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t c = 0, f = 0;
    [[maybe_unused]] T before{};
    for (uint64_t i = 0; i < h; ++i) {
        const T v = in[i];
        bool accept;
        if constexpr (ADJ) {
            accept = i == 0 || !pred(before, v);
            before = v;
        } else {
            accept = pred(v);
        }
        if (accept) {
            if (out_true) out_true[c] = v;
            ++c;
        } else {
            if (out_false) out_false[f] = v;
            ++f;
        }
    }
    *count = c;
}

// stable_partition's second step: rejected[0, n - c) -> data[c, n), c read
// from device memory.  16-B stores from data + c's next 16-B boundary.
constexpr int kTailThreads = 256;
template <typename T>
__global__ __launch_bounds__(kTailThreads) void k_partition_tail(const T* rejected, T* data, uint64_t n,
                                                                 const uint64_t* count_dev) {
    constexpr int V = 16 / sizeof(T);
    using VT = vec<T, V>;
    const uint64_t c = *count_dev < n ? *count_dev : n;
    const uint64_t m = n - c;
    T* o = data + c;
    const uint64_t to16 = ((16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15) / sizeof(T);
    const uint64_t head = m < to16 ? m : to16;
    const uint64_t nvec = (m - head) / V;
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) o[threadIdx.x] = rejected[threadIdx.x];
        const uint64_t t0 = head + nvec * V;  // fewer than V elements past the vectors
        if (threadIdx.x >= 64 && t0 + (threadIdx.x - 64) < m) o[t0 + (threadIdx.x - 64)] = rejected[t0 + (threadIdx.x - 64)];
    }
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kTailThreads;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * kTailThreads + threadIdx.x; q < nvec; q += stride) {
        VT w;
        if (head == 0 && (reinterpret_cast<uintptr_t>(rejected) & 15) == 0) {
            w = ld_stream(reinterpret_cast<const VT*>(rejected) + q);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) w.v[e] = rejected[head + q * V + e];
        }
        st_stream(reinterpret_cast<VT*>(o + head) + q, w);
    }
}

// ---------------------------------------------------------------- host side
// Scratch of one call: [counter | tile slots | head count | stable_partition:
// n rejected elements].  launch() zeroes the counter and the slots it uses;
// the head count (misaligned inputs) sits past them.  The slots are sized
// for the 64-bit look-back value, so one size serves both.
constexpr size_t kSlotsOff = 256;
template <typename T>
size_t head_count_off(uint64_t n) {
    return (kSlotsOff + ntiles_for<T>(n) * tile_state<uint64_t>::bytes_per_tile() + 255) / 256 * 256;
}
// Bytes of state in front of stable_partition's rejected elements; all the
// scratch the other calls need.
template <typename T>
size_t state_bytes(uint64_t n) {
    return head_count_off<T>(n) + 256;
}

template <bool TWO_SIDED, bool ALIGNED, typename SV, bool ADJ = false, typename T, typename Pred>
hipError_t launch_sv(const T* in, T* out_true, T* out_false, uint64_t n, uint64_t head, Pred pred, uint64_t* count_dev,
                     char* ws, uint32_t* err_word, int cus, const uint64_t* prefix0, hipStream_t s) {
    const uint64_t ntiles = ntiles_for<T>(n);
    hipError_t e = hipMemsetAsync(ws, 0, kSlotsOff + ntiles * tile_state<SV>::bytes_per_tile(), s);
    if (e != hipSuccess) return e;
    tile_state<SV> st{reinterpret_cast<uint64_t*>(ws + kSlotsOff), err_word};
    // one persistent workgroup per CU (its stage is 128 of the CU's 160 KiB of LDS)
    const uint64_t grid = ntiles < static_cast<uint64_t>(cus) ? ntiles : static_cast<uint64_t>(cus);
    hipLaunchKernelGGL((k_compact<T, Pred, ALIGNED, SV, TWO_SIDED, 4, kRounds, 128, ADJ>),
                       dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, in, out_true, out_false, n, head, pred, count_dev, reinterpret_cast<uint32_t*>(ws), st,
                       ntiles, prefix0);
    return hipGetLastError();
}

// Queue the compaction of [in, in + n) on s: accepted elements to out_true,
// *count_dev <- their number; TWO_SIDED: rejected ones to out_false, and
// either output may be null.  ws: state_bytes<T>(n) of scratch, err_word: the
// device error word the look-back raises, cus: the device's compute units.
// force64: the 64-bit look-back value at any n (tests).
// ADJ (one-sided): pred is a binary relation rel, and element i is accepted
// iff i == 0 or !rel(in[i - 1], in[i]) -- unique_copy, unique with
// out_true == in.
// A misaligned input whose elements are naturally aligned: the head (< 16 B)
// is placed first, the rest takes the vector kernel seeded with the head's
// count (copy_if, int64 offset by one element: 3.83 -> ~2.4 ms at 2^30,
// profiles/r02_unaligned_ranges.log).  An input that is not element-aligned,
// or one no longer than four such heads, is loaded element by element.
template <bool TWO_SIDED, bool ADJ = false, typename T, typename Pred>
hipError_t launch(const T* in, T* out_true, T* out_false, uint64_t n, Pred pred, uint64_t* count_dev, void* ws,
                  uint32_t* err_word, int cus, bool force64, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s);
    char* base = static_cast<char*>(ws);
    const bool sv32 = n < (uint64_t{1} << 32) && !force64;
    auto run = [&](auto aligned, const T* ip, uint64_t m, uint64_t head, const uint64_t* prefix0) {
        constexpr bool A = decltype(aligned)::value;
        return sv32 ? launch_sv<TWO_SIDED, A, uint32_t, ADJ>(ip, out_true, out_false, m, head, pred, count_dev, base,
                                                             err_word, cus, prefix0, s)
                    : launch_sv<TWO_SIDED, A, uint64_t, ADJ>(ip, out_true, out_false, m, head, pred, count_dev, base,
                                                             err_word, cus, prefix0, s);
    };
    const uint64_t h = head_to_align16(in, sizeof(T));
    if (h == 0) return run(std::true_type{}, in, n, 0, nullptr);
    if (h != UINT64_MAX && n > 4 * h) {
        auto* hc = reinterpret_cast<uint64_t*>(base + head_count_off<T>(n));
        hipLaunchKernelGGL((k_compact_head<T, Pred, ADJ>), dim3(1), dim3(64), 0, s, in, out_true,
                           TWO_SIDED ? out_false : static_cast<T*>(nullptr), h, pred, hc);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        return run(std::true_type{}, in + h, n - h, h, hc);
    }
    return run(std::false_type{}, in, n, 0, nullptr);
}

// stable_partition's second step after launch<true>(data, data, rejected, ...).
template <typename T>
hipError_t launch_tail(const T* rejected, T* data, uint64_t n, const uint64_t* count_dev, int cus, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t nvec = n / (16 / sizeof(T)) + 1;
    const uint64_t want = (nvec + kTailThreads - 1) / kTailThreads, most = static_cast<uint64_t>(cus) * 8;
    hipLaunchKernelGGL((k_partition_tail<T>), dim3(static_cast<unsigned>(want < most ? want : most)),
                       dim3(kTailThreads), 0, s, rejected, data, n, count_dev);
    return hipGetLastError();
}

}  // namespace compaction_detail
}  // namespace hpxhip
