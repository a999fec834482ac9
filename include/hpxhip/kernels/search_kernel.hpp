// search_kernel.hpp -- the kernels of the search family: find / find_if /
// find_if_not / all_of / any_of / none_of / equal / mismatch (k_find_first)
// and min_element / max_element / minmax_element (k_arg_extreme).  count_if
// needs none: it is reduce_kernel.hpp's k_reduce over a source whose elem(x)
// is `pred(x) ? 1 : 0`.  Header so that the library's precompiled kinds
// (hpx_amd/csrc/search.hip) and the C++ layer's device closures
// (hpx/parallel/detail/device_algorithms.hpp) instantiate the same bodies.
//
// Geometry: reduce_kernel.hpp's.  1024 threads per block, 8 16-B vectors per
// thread (128 KiB per block and input), every load of a chunk in flight
// before the first compare, nontemporal; geom{head, nvec, tail} keeps the
// 16-B loads for sub-ranges; two inputs that cannot be aligned together take
// element loads (V = 1).
//
// k_find_first: the smallest i in [0, n) with hit(i), else n.
//   Src provides  const TI* a, *b;
//                 __device__ bool hit(TI x) const;         (unary)
//                 __device__ bool hit(TI x, TI y) const;   (binary)
//   The result word is the caller's uint64 itself.  A one-thread launch stores
//   n there; each block reduces its hits to one minimum index and, if it has
//   one, issues ONE agent-scope atomic min on the word.
//   Early exit: before it issues its loads, each wave reads the word (relaxed,
//   agent scope: served by L2, the XCD L2s are not coherent with each other
//   and a plain load could be served by a stale L1 line for ever) and skips
//   its loads if the value is below the block's first index: no element of
//   the block can then lower the result.  The read is only a hint.  Whatever
//   order blocks run in and whatever a wave sees -- n, a stale value, another
//   block's hit -- every value the word ever holds is n or the index of a
//   real hit, a wave skips only indices above such a hit, and every block
//   that did not skip folds its own minimum in with an atomic min.  So the
//   final value is the exact minimum over all hits.  Nothing waits on another
//   block: no look-back, no spin, no flag; a wave that skips still meets its
//   block's barrier (no wave leaves early).
//
// k_arg_extreme: the index of the extreme element(s) under a strict weak
//   order comp.  Per thread the best value(s) and where they were seen (the
//   index comes from the position, never from memory); per block a reduction
//   of (value, index) pairs; one pair per block and requested extreme to
//   scratch; k_arg_partials (one block) folds the partials in a fixed order.
//   Tie rules (the reference's sequential loops, minmax.hpp:46-66, 277,
//   513-541): min_element the FIRST smallest, max_element the FIRST largest,
//   minmax_element the FIRST smallest and the LAST largest.  The pair
//   operator orders by value under comp and, among equivalent values
//   (!comp(a,b) && !comp(b,a)), by index -- min or max as the rule needs;
//   for a strict weak order that is reducing the value first and the index
//   among the equivalent ones second, in one tree.  Floats compare by value:
//   -0.0 and +0.0 tie.
//   NaN: under std::less a NaN is "equivalent" to every value, which is no
//   strict weak order, and the standard leaves the result unspecified.  Here
//   the result is then the index the fixed tree arrives at: always the index
//   of an element of the range, and the same for the same input, n and
//   alignment run to run (nothing depends on the order blocks run in).  It
//   need not be what a sequential loop returns.
#pragma once

#include <hpxhip/kernels/reduce_kernel.hpp>

namespace hpxhip {
namespace search_detail {

using reduce_detail::geom;
using reduce_detail::kSteps;
using reduce_detail::kThreads;
using reduce_detail::kWaves;

constexpr uint64_t kNone = UINT64_MAX;   // "no index"
constexpr uint32_t kNoCode = UINT32_MAX;  // "no position in this thread's chunk"

// Index of position `code` (= k * V + e: vector k of the thread, element e)
// of the thread whose first vector is `base`.
template <int V>
__device__ __forceinline__ uint64_t code_index(const geom& g, uint64_t base, uint32_t code) {
    return g.head + (base + static_cast<uint64_t>(code / V) * kThreads) * V + code % V;
}

__device__ __forceinline__ uint64_t wave_uniform(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// ---------------------------------------------------------------- find first
// The calling thread's smallest hit in chunk c of nchunks (kNone: none).
// Chunk 0 also owns the scalar head, the last chunk the scalar tail.
template <typename TI, typename Src, bool BINARY, int V>
__device__ __forceinline__ uint64_t find_in_chunk(const Src& src, const geom& g, uint64_t c, uint64_t nchunks) {
    using VI = vec<TI, V>;
    const uint64_t tid = threadIdx.x;
    const uint64_t base = c * kThreads * kSteps + tid;
    auto hit_at = [&](uint64_t i) -> bool {
        if constexpr (BINARY) return src.hit(src.a[i], src.b[i]);
        else return src.hit(src.a[i]);
    };
    auto hit = [&](TI x, TI y) -> bool {
        if constexpr (BINARY) return src.hit(x, y);
        else return src.hit(x);
    };
    uint64_t best = kNone;
    if (c == 0 && tid < g.head && hit_at(tid)) best = tid;
    const VI* va = reinterpret_cast<const VI*>(src.a + g.head);
    const VI* vb = reinterpret_cast<const VI*>((BINARY ? src.b : src.a) + g.head);
    uint32_t code = kNoCode;
    if (base + static_cast<uint64_t>(kSteps - 1) * kThreads < g.nvec) {
        // full chunk: every load in flight before the first compare
        VI x[kSteps], y[kSteps];
#pragma unroll
        for (int k = 0; k < kSteps; ++k) {
            x[k] = ld_stream(&va[base + static_cast<uint64_t>(k) * kThreads]);
            if constexpr (BINARY) y[k] = ld_stream(&vb[base + static_cast<uint64_t>(k) * kThreads]);
            else y[k] = x[k];
        }
        // descending, so that the last assignment is the smallest position
#pragma unroll
        for (int k = kSteps - 1; k >= 0; --k)
#pragma unroll
            for (int e = V - 1; e >= 0; --e)
                if (hit(x[k].v[e], y[k].v[e])) code = k * V + e;
    } else {
#pragma unroll 2
        for (int k = 0; k < kSteps; ++k) {
            const uint64_t i = base + static_cast<uint64_t>(k) * kThreads;
            if (i < g.nvec) {
                const VI x = ld_stream(&va[i]);
                VI y = x;
                if constexpr (BINARY) y = ld_stream(&vb[i]);
#pragma unroll
                for (int e = V - 1; e >= 0; --e)
                    if (code > static_cast<uint32_t>(k * V + e) && hit(x.v[e], y.v[e])) code = k * V + e;
            }
        }
    }
    // head < every vector element < tail
    if (best == kNone && code != kNoCode) best = code_index<V>(g, base, code);
    if (c == nchunks - 1 && tid < g.tail) {
        const uint64_t i = g.head + g.nvec * V + tid;
        if (best == kNone && hit_at(i)) best = i;
    }
    return best;
}

// The smallest index chunk c looks at (chunk 0 also owns the head).
template <int V>
__device__ __forceinline__ uint64_t chunk_first(const geom& g, uint64_t c) {
    return c ? g.head + c * kThreads * kSteps * V : 0;
}

// One block per chunk, in ascending order as the reduce kernel runs them.
template <typename TI, typename Src, bool BINARY, int V>
__global__ __launch_bounds__(kThreads) void k_find_first(Src src, geom g, uint64_t* __restrict__ word) {
    __shared__ uint64_t lds[kWaves];
    uint64_t best = kNone;
    // the hint: a hit below this block is already known (per wave; see above)
    if (!(wave_uniform(ld_agent(word)) < chunk_first<V>(g, blockIdx.x)))
        best = find_in_chunk<TI, Src, BINARY, V>(src, g, blockIdx.x, gridDim.x);
    const uint64_t blk = reduce_detail::block_reduce(best, op_min{}, lds);
    if (threadIdx.x == 0 && blk != kNone)
        __hip_atomic_fetch_min(word, blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Ablation builds only (-DHPXHIP_FIND_WALK_BLOCKS=512, `make find-walk`): the
// other grid that was measured, a fixed number of blocks that walk the chunks
// in ascending order and read the word again before each (DESIGN.md has the
// figures).  Thread 0 reads the word and the block's own result goes the same
// way through LDS, so every branch around a barrier is block-uniform.
#ifndef HPXHIP_FIND_WALK_BLOCKS
#define HPXHIP_FIND_WALK_BLOCKS 0
#endif
#if HPXHIP_FIND_WALK_BLOCKS
template <typename TI, typename Src, bool BINARY, int V>
__global__ __launch_bounds__(kThreads) void k_find_first_walk(Src src, geom g, uint64_t nchunks,
                                                              uint64_t* __restrict__ word) {
    __shared__ uint64_t lds[kWaves];
    __shared__ uint64_t shared_word;
    for (uint64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        if (threadIdx.x == 0) shared_word = ld_agent(word);
        __syncthreads();
        if (shared_word < chunk_first<V>(g, c)) break;  // every later chunk of this block lies higher still
        const uint64_t best = find_in_chunk<TI, Src, BINARY, V>(src, g, c, nchunks);
        const uint64_t blk = reduce_detail::block_reduce(best, op_min{}, lds);
        if (threadIdx.x == 0) {
            if (blk != kNone) __hip_atomic_fetch_min(word, blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            shared_word = blk;
        }
        __syncthreads();
        if (shared_word != kNone) break;  // a hit of its own: later chunks cannot lower it
        __syncthreads();                  // shared_word is rewritten at the top
    }
}
#endif

template <typename TI, typename Src, bool BINARY, int V>
void launch_find_grid(const Src& src, const geom& g, uint64_t chunks, uint64_t* word, hipStream_t s) {
#if HPXHIP_FIND_WALK_BLOCKS
    const uint64_t blocks = chunks < HPXHIP_FIND_WALK_BLOCKS ? chunks : HPXHIP_FIND_WALK_BLOCKS;
    hipLaunchKernelGGL((k_find_first_walk<TI, Src, BINARY, V>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads),
                       0, s, src, g, chunks, word);
#else
    hipLaunchKernelGGL((k_find_first<TI, Src, BINARY, V>), dim3(static_cast<unsigned>(chunks)), dim3(kThreads), 0, s,
                       src, g, word);
#endif
}

// Queue "*word = smallest i in [0, n) with hit(i), else n" on s.  word is
// 8-byte aligned device memory.  Returns a hipError_t.
template <typename TI, typename Src, bool BINARY>
hipError_t launch_find(Src src, uint64_t n, uint64_t* word, hipStream_t s) {
    hipLaunchKernelGGL((reduce_detail::k_write_init<uint64_t>), dim3(1), dim3(64), 0, s, n, word);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    constexpr int V = 16 % sizeof(TI) == 0 ? 16 / sizeof(TI) : 1;
    const uint64_t per_block = static_cast<uint64_t>(kThreads) * kSteps;
    uint64_t ha = V > 1 ? head_to_align16(src.a, sizeof(TI)) : 0;
    const uint64_t hb = (BINARY && V > 1) ? head_to_align16(src.b, sizeof(TI)) : ha;
    if (ha != UINT64_MAX && ha == hb) {
        if (ha > n) ha = n;
        geom g;
        g.head = ha;
        g.nvec = (n - ha) / V;
        g.tail = n - ha - g.nvec * V;
        uint64_t blocks = (g.nvec + per_block - 1) / per_block;
        if (blocks == 0) blocks = 1;
        launch_find_grid<TI, Src, BINARY, V>(src, g, blocks, word, s);
    } else {
        // inputs that cannot be 16-B aligned together: element loads
        const geom g{0, n, 0};
        const uint64_t blocks = (n + per_block - 1) / per_block;
        launch_find_grid<TI, Src, BINARY, 1>(src, g, blocks, word, s);
    }
    return hipGetLastError();
}

// --------------------------------------------------------------- arg extreme
enum : int { kArgMin = 0, kArgMax = 1, kArgMinMax = 2 };            // HPXHIP_X_*
enum : int { kFirstSmallest = 0, kFirstLargest = 1, kLastLargest = 2 };  // tie rules

template <typename T>
struct arg_pair {
    T v;
    uint64_t i;  // kNone: no value
};

// true if x replaces the running best when elements are met in ASCENDING index order
template <int RULE, typename T, typename Comp>
__device__ __forceinline__ bool arg_takes(const Comp& comp, T x, T best) {
    if constexpr (RULE == kFirstSmallest) return comp(x, best);
    else if constexpr (RULE == kFirstLargest) return comp(best, x);
    else return !comp(x, best);
}

template <typename T, typename Comp, int RULE>
struct arg_op {
    Comp comp;
    template <typename X>
    __device__ __forceinline__ X operator()(X a, X b) const {
        if (b.i == kNone) return a;
        if (a.i == kNone) return b;
        const bool b_wins = RULE == kFirstSmallest ? comp(b.v, a.v) : comp(a.v, b.v);
        const bool a_wins = RULE == kFirstSmallest ? comp(a.v, b.v) : comp(b.v, a.v);
        if (b_wins) return b;
        if (a_wins) return a;
        return ((b.i < a.i) == (RULE != kLastLargest)) ? b : a;
    }
    template <typename X>
    __host__ __device__ static constexpr X identity() {
        X r{};
        r.i = kNone;
        return r;
    }
};

template <int WHICH>
struct arg_rules {
    static constexpr int n = WHICH == kArgMinMax ? 2 : 1;
    static constexpr int r0 = WHICH == kArgMax ? kFirstLargest : kFirstSmallest;
    static constexpr int r1 = kLastLargest;  // MINMAX's second
};

template <typename TI, typename Comp, int WHICH, int V>
__global__ __launch_bounds__(kThreads) void k_arg_extreme(const TI* __restrict__ in, geom g, Comp comp,
                                                          arg_pair<TI>* __restrict__ partials,
                                                          uint64_t* __restrict__ out) {
    using VI = vec<TI, V>;
    using P = arg_pair<TI>;
    using R = arg_rules<WHICH>;
    constexpr bool TWO = R::n == 2;
    __shared__ P lds[2][kWaves];

    const uint64_t tid = threadIdx.x;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kThreads * kSteps + tid;
    const arg_op<TI, Comp, R::r0> op0{comp};
    const arg_op<TI, Comp, R::r1> op1{comp};

    TI v0{}, v1{};
    uint32_t c0 = kNoCode, c1 = kNoCode;
    const VI* va = reinterpret_cast<const VI*>(in + g.head);
    if (base + static_cast<uint64_t>(kSteps - 1) * kThreads < g.nvec) {
        VI x[kSteps];
#pragma unroll
        for (int k = 0; k < kSteps; ++k) x[k] = ld_stream(&va[base + static_cast<uint64_t>(k) * kThreads]);
        v0 = v1 = x[0].v[0];
        c0 = c1 = 0;
#pragma unroll
        for (int k = 0; k < kSteps; ++k)
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (k == 0 && e == 0) continue;
                const TI xe = x[k].v[e];
                if (arg_takes<R::r0>(comp, xe, v0)) {
                    v0 = xe;
                    c0 = k * V + e;
                }
                if constexpr (TWO)
                    if (arg_takes<R::r1>(comp, xe, v1)) {
                        v1 = xe;
                        c1 = k * V + e;
                    }
            }
    } else {
#pragma unroll 2
        for (int k = 0; k < kSteps; ++k) {
            const uint64_t i = base + static_cast<uint64_t>(k) * kThreads;
            if (i < g.nvec) {
                const VI x = ld_stream(&va[i]);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const TI xe = x.v[e];
                    if (c0 == kNoCode || arg_takes<R::r0>(comp, xe, v0)) {
                        v0 = xe;
                        c0 = k * V + e;
                    }
                    if constexpr (TWO)
                        if (c1 == kNoCode || arg_takes<R::r1>(comp, xe, v1)) {
                            v1 = xe;
                            c1 = k * V + e;
                        }
                }
            }
        }
    }
    P p0{v0, c0 == kNoCode ? kNone : code_index<V>(g, base, c0)};
    P p1{v1, (TWO && c1 != kNoCode) ? code_index<V>(g, base, c1) : kNone};
    // scalar head (block 0) and tail (last block): the pair operator is
    // commutative, the index decides among equivalent values
    if (blockIdx.x == 0 && tid < g.head) {
        const P h{in[tid], tid};
        p0 = op0(p0, h);
        if constexpr (TWO) p1 = op1(p1, h);
    }
    if (blockIdx.x == gridDim.x - 1 && tid < g.tail) {
        const uint64_t i = g.head + g.nvec * V + tid;
        const P t{in[i], i};
        p0 = op0(p0, t);
        if constexpr (TWO) p1 = op1(p1, t);
    }

    const P b0 = reduce_detail::block_reduce(p0, op0, lds[0]);
    P b1 = b0;
    if constexpr (TWO) b1 = reduce_detail::block_reduce(p1, op1, lds[1]);
    if (tid == 0) {
        if (gridDim.x == 1) {
            out[0] = b0.i;
            if constexpr (TWO) out[1] = b1.i;
        } else {
            partials[blockIdx.x] = b0;
            if constexpr (TWO) partials[gridDim.x + blockIdx.x] = b1;
        }
    }
}

// Fold of the block partials (one block; the previous launch's stores are
// visible at the kernel boundary): thread t folds partials t, t + 1024, ...,
// then the block tree -- a fixed order for a given partial count.
template <typename TI, typename Comp, int WHICH>
__global__ __launch_bounds__(kThreads) void k_arg_partials(const arg_pair<TI>* __restrict__ partials, uint32_t count,
                                                           Comp comp, uint64_t* __restrict__ out) {
    using P = arg_pair<TI>;
    using R = arg_rules<WHICH>;
    constexpr bool TWO = R::n == 2;
    __shared__ P lds[2][kWaves];
    const arg_op<TI, Comp, R::r0> op0{comp};
    const arg_op<TI, Comp, R::r1> op1{comp};
    P p0 = op0.template identity<P>(), p1 = p0;
    for (uint32_t i = threadIdx.x; i < count; i += kThreads) {
        p0 = op0(p0, partials[i]);
        if constexpr (TWO) p1 = op1(p1, partials[count + i]);
    }
    const P b0 = reduce_detail::block_reduce(p0, op0, lds[0]);
    P b1 = b0;
    if constexpr (TWO) b1 = reduce_detail::block_reduce(p1, op1, lds[1]);
    if (threadIdx.x == 0) {
        out[0] = b0.i;
        if constexpr (TWO) out[1] = b1.i;
    }
}

// Scratch of launch_arg for n elements: one pair per block and extreme (the
// size for two extremes; every pair is 16 bytes).
__host__ __device__ inline size_t arg_scratch_bytes(uint64_t n) {
    return (reduce_detail::max_blocks(n) * 2 * 16 + 255) / 256 * 256;
}

// Queue the arg-extreme of [in, in + n) on s: out[0] (and out[1] for
// kArgMinMax) receive the indices; n == 0 writes 0.  partials:
// arg_scratch_bytes(n) bytes.  in must be aligned to its element.
template <typename TI, typename Comp, int WHICH>
hipError_t launch_arg(const TI* in, uint64_t n, Comp comp, uint64_t* out, void* partials, hipStream_t s) {
    static_assert(sizeof(arg_pair<TI>) == 16, "arg_pair: 4- or 8-byte element types");
    if (n == 0) {
        hipLaunchKernelGGL((reduce_detail::k_write_init<uint64_t>), dim3(1), dim3(64), 0, s, uint64_t(0), out);
        if (WHICH == kArgMinMax)
            hipLaunchKernelGGL((reduce_detail::k_write_init<uint64_t>), dim3(1), dim3(64), 0, s, uint64_t(0), out + 1);
        return hipGetLastError();
    }
    constexpr int V = 16 / sizeof(TI);
    const uint64_t per_block = static_cast<uint64_t>(kThreads) * kSteps;
    uint64_t ha = head_to_align16(in, sizeof(TI));
    if (ha == UINT64_MAX) return hipErrorInvalidValue;
    if (ha > n) ha = n;
    geom g;
    g.head = ha;
    g.nvec = (n - ha) / V;
    g.tail = n - ha - g.nvec * V;
    uint64_t blocks = (g.nvec + per_block - 1) / per_block;
    if (blocks == 0) blocks = 1;
    arg_pair<TI>* ps = static_cast<arg_pair<TI>*>(partials);
    hipLaunchKernelGGL((k_arg_extreme<TI, Comp, WHICH, V>), dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s,
                       in, g, comp, ps, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || blocks <= 1) return e;
    hipLaunchKernelGGL((k_arg_partials<TI, Comp, WHICH>), dim3(1), dim3(kThreads), 0, s, ps,
                       static_cast<uint32_t>(blocks), comp, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ count_if
// The element source of reduce_kernel.hpp that counts: elem(x) = pred(x) ? 1 : 0
// summed in uint64.
template <typename TI, typename Pred>
struct count_source {
    const TI* a;
    const TI* b;
    Pred pred;
    __device__ __forceinline__ uint64_t elem(TI x) const { return pred(x) ? 1u : 0u; }
};

template <typename TI, typename Pred>
hipError_t launch_count(const TI* in, uint64_t n, Pred pred, uint64_t* out, void* partials, hipStream_t s) {
    count_source<TI, Pred> src{in, nullptr, pred};
    return reduce_detail::launch<TI, uint64_t, count_source<TI, Pred>, op_plus, false>(
        src, n, op_plus{}, uint64_t(0), out, static_cast<uint64_t*>(partials), s);
}

}  // namespace search_detail
}  // namespace hpxhip
