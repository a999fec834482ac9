// hpx/parallel/detail/device_algorithms.hpp -- reduce / transform_reduce,
// the scans, copy_if and sort with ARBITRARY HPX_HOST_DEVICE callables, when
// the calling translation unit is compiled by hipcc.
//
// The reference accepts any conv / op / pred / comp (transform_reduce.hpp:254,
// inclusive_scan.hpp:288-606, copy.hpp:585, sort.hpp:364 with a projection).
// The library's precompiled entry points take an operator KIND, so a function
// object with a traits mapping goes there (algorithms.hpp); anything else
// lands here and instantiates the library's OWN kernel bodies with the
// caller's callable (include/hpxhip/kernels/):
//
//   reduce / transform_reduce  reduce_kernel.hpp   (128-KiB blocks, DPP tree,
//                                                   fixed-order partial fold)
//   scans                      scan_kernel.hpp     (single pass, decoupled
//                                                   look-back, 16-B tiles)
//   copy_if, partition_copy, stable_partition, remove_copy_if, remove_if
//   unique, unique_copy
//                              compaction_kernel.hpp (ballot ranks, look-back;
//                                                   one- and two-sided)
//   reduce_by_key              reduce_by_key_kernel.hpp (segmented look-back)
//   find_if, find_if_not, all_of, any_of, none_of, equal, mismatch, count_if,
//   min_element, max_element, minmax_element
//                              search_kernel.hpp   (first hit by atomic min with
//                                                   an early-exit hint; arg-extreme
//                                                   pairs; count on the reduce kernel)
//   replace_if, replace_copy_if, adjacent_difference
//                              device_closures.hpp (the transform closure kernels)
//   sort (comp, proj)          merge_kernel.hpp    (block sort in LDS, then
//                                                   merge-path passes)
//
// A user operator has no known identity, but every GPU tree and scan pads its
// inactive lanes with one: such an op is lifted to opt<T> (a value or "none",
// "none" being the identity; common.hpp lifted_op).  A built-in operator
// (std::plus, ...) with a user conv keeps the plain value type.
//
// Semantics: reduce / transform_reduce need an associative and commutative
// op (reduce.hpp: "the behavior is non-deterministic if binary_op is not
// associative or not commutative"); the scans need associativity only (the
// kernels combine in index order); copy_if is stable; the merge sort is
// stable (a valid std::sort order, ties in input order).
#pragma once

#include <hpx/compute/hip.hpp>
#include <hpx/compute/hip/detail/launch.hpp>
#include <hpx/compute/hip/functional.hpp>
#include <hpx/parallel/detail/device_closures.hpp>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include <utility>

#if HPX_HAVE_HIP_DEVICE_CLOSURES
#include <hpxhip/kernels/compaction_kernel.hpp>
#include <hpxhip/kernels/merge_kernel.hpp>
#include <hpxhip/kernels/set_kernel.hpp>
#include <hpxhip/kernels/reduce_by_key_kernel.hpp>
#include <hpxhip/kernels/reduce_kernel.hpp>
#include <hpxhip/kernels/scan_kernel.hpp>
#include <hpxhip/kernels/search_kernel.hpp>
#endif

namespace hpx { namespace parallel { inline namespace v1 { namespace detail {
namespace dev {

#if HPX_HAVE_HIP_DEVICE_CLOSURES
namespace K = ::hpxhip;
namespace tr = hpx::compute::hip::traits;

// built-in operator kinds -> the kernels' device functors (identity known)
template <int Kind> struct kind_op;
template <> struct kind_op<HPXHIP_PLUS> { using type = K::op_plus; };
template <> struct kind_op<HPXHIP_MULTIPLIES> { using type = K::op_multiplies; };
template <> struct kind_op<HPXHIP_MIN> { using type = K::op_min; };
template <> struct kind_op<HPXHIP_MAX> { using type = K::op_max; };
template <> struct kind_op<HPXHIP_BIT_AND> { using type = K::op_bit_and; };
template <> struct kind_op<HPXHIP_BIT_OR> { using type = K::op_bit_or; };
template <> struct kind_op<HPXHIP_BIT_XOR> { using type = K::op_bit_xor; };
template <typename Op>
using builtin_op_t = typename kind_op<tr::binop_t<Op>::kind>::type;
// the device operator of Op: its built-in functor, or Op lifted to opt<T>
template <typename Op, bool BUILTIN = tr::is_binop<Op>>
struct dev_op {
    using type = K::lifted_op<std::decay_t<Op>>;
};
template <typename Op>
struct dev_op<Op, true> {
    using type = builtin_op_t<Op>;
};

// the scans' device operator: a built-in kind, or the user operator without
// an identity (K::noid_op)
template <typename Op, bool = tr::is_binop<Op>>
struct scan_op {
    using type = K::noid_op<std::decay_t<Op>>;
};
template <typename Op>
struct scan_op<Op, true> {
    using type = builtin_op_t<Op>;
};

inline hipStream_t stream_of(compute::hip::target const& t) { return reinterpret_cast<hipStream_t>(t.stream()); }

inline void* scratch(compute::hip::target const& t, std::size_t bytes, char const* what) {
    void* p = nullptr;
    compute::hip::detail::check(hpxhip_stream_scratch(t.stream(), bytes, &p), what);
    return p;
}
inline uint32_t* error_word(compute::hip::target const& t) {
    uint32_t* w = nullptr;
    compute::hip::detail::check(hpxhip_device_error_word(t.stream(), &w), "device error word");
    return w;
}
inline void launched(char const* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw hpx::kernel_error(static_cast<int>(e), std::string(what) + ": " +
                                                                                 hipGetErrorString(e));
}

// ------------------------------------------------------------------ reduce
// Element sources of reduce_kernel.hpp: conv on one / two elements, plain
// (built-in op) or lifted to opt<TA> (user op).
template <typename TI, typename TA, typename Conv, bool LIFT>
struct source1 {
    const TI* a;
    const TI* b;
    Conv conv;
    using R = std::conditional_t<LIFT, K::opt<TA>, TA>;
    __device__ __forceinline__ R elem(TI x) const {
        if constexpr (LIFT) return R{static_cast<TA>(conv(x)), 1u};
        else return static_cast<TA>(conv(x));
    }
};
template <typename TI, typename TA, typename Comb, bool LIFT>
struct source2 {
    const TI* a;
    const TI* b;
    Comb comb;
    using R = std::conditional_t<LIFT, K::opt<TA>, TA>;
    __device__ __forceinline__ R elem(TI x, TI y) const {
        if constexpr (LIFT) return R{static_cast<TA>(comb(x, y)), 1u};
        else return static_cast<TA>(comb(x, y));
    }
};

// *out_dev (a result slot) <- init (red) conv(x_0) (red) ...; the TA value
// sits at the start of the slot in both forms (opt<TA>::v is its first member).
template <typename TA, bool BINARY, typename TI, typename Red, typename Conv>
void reduce(compute::hip::target const& t, TI const* a, TI const* b, uint64_t n, TA init, Red const& red,
            Conv const& conv, void* out_dev) {
    constexpr bool lift = !tr::is_binop<Red>;
    using X = std::conditional_t<lift, K::opt<TA>, TA>;
    using Src = std::conditional_t<BINARY, source2<TI, TA, std::decay_t<Conv>, lift>,
                                   source1<TI, TA, std::decay_t<Conv>, lift>>;
    static_assert(sizeof(X) <= compute::hip::detail::device_pool::kSlotBytes, "reduce: result larger than a slot");
    X* partials = n ? static_cast<X*>(scratch(t, K::reduce_detail::max_blocks(n) * sizeof(X), "reduce scratch"))
                    : nullptr;
    Src src{a, b, conv};
    hipError_t e;
    if constexpr (lift) {
        using Op = K::lifted_op<std::decay_t<Red>>;
        e = K::reduce_detail::launch<TI, X, Src, Op, BINARY>(src, n, Op{red}, X{init, 1u}, static_cast<X*>(out_dev),
                                                             partials, stream_of(t));
    } else {
        using Op = builtin_op_t<Red>;
        e = K::reduce_detail::launch<TI, X, Src, Op, BINARY>(src, n, Op{}, init, static_cast<X*>(out_dev), partials,
                                                             stream_of(t));
    }
    if (e != hipSuccess) throw hpx::kernel_error(static_cast<int>(e), "transform_reduce (device closure)");
}

// -------------------------------------------------------------------- scans
template <typename V, typename X, typename Conv>
struct scan_conv {
    Conv conv;
    __device__ __forceinline__ X operator()(V x) const {
        if constexpr (std::is_same<X, V>::value) return static_cast<V>(conv(x));
        else return X{static_cast<V>(conv(x)), 1u};
    }
};

template <typename V, typename X, typename Cv, typename Op, bool INCL, bool ALIGNED>
void scan_launch(compute::hip::target const& t, V const* in, V* out, uint64_t n, Cv cv, Op op, X init) {
    namespace S = K::scan_detail;
    // a user operator scans plain values (noid_op, no identity needed): the
    // built-in kinds' tile shape, except 14 rounds for aligned 8-byte
    // integers (the identity-free wave scan's selects: 16 rounds spill 12
    // VGPRs, 14 fit in 120)
    constexpr bool noid = K::is_noid_op<Op>::value;
    constexpr int R = (noid && ALIGNED && sizeof(V) == 8 && std::is_integral<V>::value) ? 14
                                                                                           : S::rounds_for<V, ALIGNED>();
    constexpr uint64_t tile = S::tile_elems<V, R>();
    const uint64_t ntiles = (n + tile - 1) / tile;
    const std::size_t state = (256 + ntiles * K::tile_state<X>::bytes_per_tile() + 255) / 256 * 256;
    char* ws = static_cast<char*>(scratch(t, state, "scan scratch"));
    compute::hip::detail::check(hpxhip_memset_async(ws, 0, state, t.stream()), "scan scratch");
    K::scan_detail::scan_state<X> st{reinterpret_cast<uint64_t*>(ws + 256), error_word(t)};
    hipLaunchKernelGGL((S::k_scan<V, Cv, Op, INCL, ALIGNED, R, S::kThreads, true, 1, false, 1, false, true, X>),
                       dim3(static_cast<unsigned>(ntiles)), dim3(S::kThreads), 0, stream_of(t), in, out, n, cv, op,
                       init, static_cast<X const*>(nullptr), reinterpret_cast<uint32_t*>(ws), st);
    launched("scan (device closure)");
}

template <typename V, typename Op, typename Conv, typename T>
void scan(compute::hip::target const& t, V const* in, V* out, uint64_t n, Op const& op, Conv const& conv, T init,
          bool inclusive) {
    static_assert(sizeof(V) == 4 || sizeof(V) == 8, "scan (device closure): 4- or 8-byte element types");
    if (n == 0) return;
    // A user operator has no known identity: round 3 lifted it to opt<V>
    // (flag + padding per element: 8 rounds instead of 16, 2^30 int64 3.43
    // vs 2.66 ms, profiles/r04_closure_timing_first.log); the kernel now runs
    // it on plain values with the identity-free scan (K::noid_op).
    constexpr bool lift = !tr::is_binop<Op>;
    using X = V;
    using Cv = scan_conv<V, X, std::decay_t<Conv>>;
    using OpD = typename scan_op<Op>::type;
    const OpD opd = [&] {
        if constexpr (lift) return OpD{op};
        else return OpD{};
    }();
    const X iv = static_cast<V>(init);
    const bool aligned = (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    Cv cv{conv};
    if (inclusive) {
        if (aligned) scan_launch<V, X, Cv, OpD, true, true>(t, in, out, n, cv, opd, iv);
        else scan_launch<V, X, Cv, OpD, true, false>(t, in, out, n, cv, opd, iv);
    } else {
        if (aligned) scan_launch<V, X, Cv, OpD, false, true>(t, in, out, n, cv, opd, iv);
        else scan_launch<V, X, Cv, OpD, false, false>(t, in, out, n, cv, opd, iv);
    }
}

// ----------------------------------- copy_if, partition and remove families
// copy.hpp:585, partition.hpp:1350 / remove_copy.hpp:350 with any predicate:
// the library's compaction kernel through the library's launcher
// (compaction_kernel.hpp), instantiated for the callable.  A misaligned range
// takes the head split and the vector kernel, as in the library.
template <typename T, typename Pred>
struct as_bool_pred {
    Pred pred;
    __device__ __forceinline__ bool operator()(T x) const { return static_cast<bool>(pred(x)); }
};

inline int cus_of(compute::hip::target const& t) {
    static std::atomic<int> cus[64];
    const int dev = t.device();
    int c = dev >= 0 && dev < 64 ? cus[dev].load(std::memory_order_relaxed) : 0;
    if (c <= 0) {
        c = static_cast<int>(t.native_handle().processing_units());
        if (dev >= 0 && dev < 64) cus[dev].store(c, std::memory_order_relaxed);
    }
    return c;
}

// ws: compaction_detail::state_bytes<T>(n) of scratch
template <bool TWO_SIDED, typename T, typename Pred>
void compact(compute::hip::target const& t, T const* in, T* out_true, T* out_false, uint64_t n, Pred const& pred,
             uint64_t* count_dev, void* ws, char const* what) {
    using P = as_bool_pred<T, std::decay_t<Pred>>;
    const hipError_t e = K::compaction_detail::launch<TWO_SIDED>(in, out_true, out_false, n, P{pred}, count_dev, ws,
                                                                 error_word(t), cus_of(t), false, stream_of(t));
    if (e != hipSuccess) throw hpx::kernel_error(static_cast<int>(e), std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T, typename Pred>
void copy_if(compute::hip::target const& t, T const* in, T* out, uint64_t n, Pred const& pred, uint64_t* count_dev) {
    static_assert(16 % sizeof(T) == 0, "copy_if (device closure): element size must divide 16 bytes");
    void* ws = scratch(t, K::compaction_detail::state_bytes<T>(n), "copy_if scratch");
    compact<false>(t, in, out, static_cast<T*>(nullptr), n, pred, count_dev, ws, "copy_if (device closure)");
}

// Either output may be null or the input itself.
template <typename T, typename Pred>
void partition_copy(compute::hip::target const& t, T const* in, T* out_true, T* out_false, uint64_t n,
                    Pred const& pred, uint64_t* count_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "partition (device closure): 4- or 8-byte element types");
    void* ws = scratch(t, K::compaction_detail::state_bytes<T>(n), "partition scratch");
    compact<true>(t, in, out_true, out_false, n, pred, count_dev, ws, "partition (device closure)");
}

// partition.hpp:292: accepted elements compacted in place, rejected ones to
// scratch, k_partition_tail copies them to [count, n) (count read on the
// device).
template <typename T, typename Pred>
void stable_partition(compute::hip::target const& t, T* data, uint64_t n, Pred const& pred, uint64_t* count_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "partition (device closure): 4- or 8-byte element types");
    namespace C = K::compaction_detail;
    const std::size_t state = C::state_bytes<T>(n);
    char* ws = static_cast<char*>(scratch(t, state + n * sizeof(T), "stable_partition scratch"));
    T* rejected = reinterpret_cast<T*>(ws + state);
    compact<true>(t, static_cast<T const*>(data), data, rejected, n, pred, count_dev, ws,
                  "stable_partition (device closure)");
    const hipError_t e = C::launch_tail(static_cast<T const*>(rejected), data, n, count_dev, cus_of(t), stream_of(t));
    if (e != hipSuccess) throw hpx::kernel_error(static_cast<int>(e), "stable_partition (device closure)");
}

// ------------------------------------------------------ unique / unique_copy
// unique.hpp:311,612 with any binary predicate and projection: the library's
// compaction kernel in its adjacent mode through the library's launcher.
// Element i is kept iff i == 0 or !pred(proj(in[i - 1]), proj(in[i])); out may
// be exactly in (unique).
template <typename T, typename Pred, typename Proj>
struct as_projected_rel {
    Pred pred;
    Proj proj;
    __device__ __forceinline__ bool operator()(T const& a, T const& b) const {
        return static_cast<bool>(pred(proj(a), proj(b)));
    }
};

template <typename T, typename Pred, typename Proj>
void unique_copy(compute::hip::target const& t, T const* in, T* out, uint64_t n, Pred const& pred, Proj const& proj,
                 uint64_t* count_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "unique (device closure): 4- or 8-byte element types");
    void* ws = scratch(t, K::compaction_detail::state_bytes<T>(n), "unique scratch");
    using R = as_projected_rel<T, std::decay_t<Pred>, std::decay_t<Proj>>;
    const hipError_t e = K::compaction_detail::launch<false, true>(in, out, static_cast<T*>(nullptr), n, R{pred, proj},
                                                                   count_dev, ws, error_word(t), cus_of(t), false,
                                                                   stream_of(t));
    if (e != hipSuccess)
        throw hpx::kernel_error(static_cast<int>(e), std::string("unique (device closure): ") + hipGetErrorString(e));
}

// ------------------------------------------------------------ reduce_by_key
// reduce_by_key.hpp:586 with any key comparator and any associative func
// (it needs no identity and need not commute): the library's kernel
// (reduce_by_key_kernel.hpp), instantiated for the callables.
template <typename KT, typename Comp>
struct as_key_equal {
    Comp comp;
    __device__ __forceinline__ bool operator()(KT const& a, KT const& b) const { return static_cast<bool>(comp(a, b)); }
};
template <typename V, typename Func>
struct as_value_op {
    Func func;
    __device__ __forceinline__ V operator()(V const& a, V const& b) const { return static_cast<V>(func(a, b)); }
};

template <typename KT, typename V, typename Eq, typename F, typename CT>
void reduce_by_key_launch(compute::hip::target const& t, KT const* keys, V const* vals, KT* keys_out, V* vals_out,
                          uint64_t n, Eq eq, F f, uint64_t* count_dev) {
    namespace R = K::reduce_by_key_detail;
    constexpr int E = R::lane_elems<KT, V>();
    const uint64_t ntiles = R::ntiles_for<KT, V>(n);
    const std::size_t state = (256 + ntiles * R::state_t<CT, V>::bytes_per_tile() + 255) / 256 * 256;
    char* ws = static_cast<char*>(scratch(t, state, "reduce_by_key scratch"));
    compute::hip::detail::check(hpxhip_memset_async(ws, 0, state, t.stream()), "reduce_by_key scratch");
    R::state_t<CT, V> st{reinterpret_cast<uint64_t*>(ws + 256), error_word(t)};
    const int vec_ok = reinterpret_cast<uintptr_t>(keys) % (E * sizeof(KT)) == 0 &&
                       reinterpret_cast<uintptr_t>(vals) % (E * sizeof(V)) == 0;
    hipLaunchKernelGGL((R::k_reduce_by_key<KT, V, Eq, F, CT>), dim3(static_cast<unsigned>(ntiles)), dim3(R::kThreads),
                       0, stream_of(t), keys, vals, keys_out, vals_out, n, eq, f, count_dev, st, vec_ok);
    launched("reduce_by_key (device closure)");
}

template <typename KT, typename V, typename Comp, typename Func>
void reduce_by_key(compute::hip::target const& t, KT const* keys, V const* vals, KT* keys_out, V* vals_out,
                   uint64_t n, Comp const& comp, Func const& func, uint64_t* count_dev) {
    static_assert((sizeof(KT) == 4 || sizeof(KT) == 8) && (sizeof(V) == 4 || sizeof(V) == 8),
                  "reduce_by_key (device closure): 4- or 8-byte key and value types");
    if (n == 0) {
        compute::hip::detail::check(hpxhip_memset_async(count_dev, 0, sizeof(uint64_t), t.stream()),
                                    "reduce_by_key count");
        return;
    }
    using Eq = as_key_equal<KT, std::decay_t<Comp>>;
    constexpr bool builtin = tr::is_binop<Func>;
    using F = std::conditional_t<builtin, typename scan_op<Func>::type, as_value_op<V, std::decay_t<Func>>>;
    const F f = [&] {
        if constexpr (builtin) return F{};
        else return F{func};
    }();
    if (n < (uint64_t{1} << 32))
        reduce_by_key_launch<KT, V, Eq, F, uint32_t>(t, keys, vals, keys_out, vals_out, n, Eq{comp}, f, count_dev);
    else
        reduce_by_key_launch<KT, V, Eq, F, uint64_t>(t, keys, vals, keys_out, vals_out, n, Eq{comp}, f, count_dev);
}

// --------------------------------------------------------------------- sort
// sort.hpp:364 -- comp(proj(a), proj(b)) (HPX_INVOKE of the projection).
template <typename T, typename Comp, typename Proj>
struct projected_less {
    Comp comp;
    Proj proj;
    __device__ __forceinline__ bool operator()(T const& a, T const& b) const {
        return static_cast<bool>(comp(proj(a), proj(b)));
    }
};

// Bottom-up merge sort: k_block_sort leaves sorted runs of kTile elements,
// then each pass merges run pairs (merge path) src -> dst, doubling the run
// width; the result is copied back if it ended in the scratch buffer.
template <typename T, typename Comp, typename Proj>
void merge_sort(compute::hip::target const& t, T* data, uint64_t n, Comp const& comp, Proj const& proj) {
    namespace M = K::merge_detail;
    if (n < 2) return;
    using L = projected_less<T, std::decay_t<Comp>, std::decay_t<Proj>>;
    const L less{comp, proj};
    const uint64_t ntiles = (n + M::kTile - 1) / M::kTile;
    hipLaunchKernelGGL((M::k_block_sort<T, L>), dim3(static_cast<unsigned>(ntiles)), dim3(M::kThreads), 0,
                       stream_of(t), data, n, less);
    launched("sort (device closure): block sort");
    if (ntiles == 1) return;
    const std::size_t buf = (n * sizeof(T) + 255) / 256 * 256;
    char* ws = static_cast<char*>(scratch(t, buf + (ntiles + 1) * sizeof(uint64_t), "sort scratch"));
    T* tmp = reinterpret_cast<T*>(ws);
    uint64_t* splits = reinterpret_cast<uint64_t*>(ws + buf);
    T* src = data;
    T* dst = tmp;
    // 16-B staging and stores when both buffers are 16-B aligned (the
    // scratch is; the data is unless the range starts inside a vector) and
    // n fills whole vectors (the staging reads whole vectors of each slice)
    const bool vec = reinterpret_cast<uintptr_t>(data) % 16 == 0 && reinterpret_cast<uintptr_t>(tmp) % 16 == 0 &&
                     n % M::vec_elems<T>() == 0;
    uint32_t* err = nullptr;  // a clamped split raises it (a caller racing the sort)
    compute::hip::detail::check(hpxhip_device_error_word(t.stream(), &err), "device error word");
    for (uint64_t w = M::kTile; w < n; w *= 2) {
        hipLaunchKernelGGL((M::k_pass_partition<T, L>), dim3(static_cast<unsigned>((ntiles + 255) / 256)), dim3(256),
                           0, stream_of(t), src, n, w, ntiles, less, splits);
        if (vec)
            hipLaunchKernelGGL((M::k_pass_merge<T, L, true>), dim3(static_cast<unsigned>(ntiles)), dim3(M::kThreads),
                               0, stream_of(t), src, n, w, splits, less, dst, err);
        else
            hipLaunchKernelGGL((M::k_pass_merge<T, L>), dim3(static_cast<unsigned>(ntiles)), dim3(M::kThreads), 0,
                               stream_of(t), src, n, w, splits, less, dst, err);
        launched("sort (device closure): merge pass");
        std::swap(src, dst);
    }
    if (src != data) compute::hip::detail::check(hpxhip_memcpy_async(data, src, n * sizeof(T), HPXHIP_D2D, t.stream()), "sort copy-back");
}
// ----------------------------------------------------------- set operations
// set_union.hpp:47 and its siblings, includes.hpp:129 with any comparator:
// the library's kernels (set_kernel.hpp) through the library's launcher,
// instantiated for the user's strict weak ordering.  out == nullptr counts.
template <typename T, typename Comp>
struct as_less {
    Comp comp;
    __device__ __forceinline__ bool operator()(T const& a, T const& b) const { return static_cast<bool>(comp(a, b)); }
};

template <typename T, typename Comp>
void set_operation(compute::hip::target const& t, int op, T const* a, uint64_t na, T const* b, uint64_t nb, T* out,
                   Comp const& comp, uint64_t* count_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "set operation (device closure): 4- or 8-byte element types");
    namespace S = K::set_detail;
    void* ws = scratch(t, S::scratch_bytes(na + nb), "set operation scratch");
    using L = as_less<T, std::decay_t<Comp>>;
    const hipError_t e = S::launch(a, na, b, nb, out, op, L{comp}, count_dev, ws, error_word(t), stream_of(t));
    if (e != hipSuccess)
        throw hpx::kernel_error(static_cast<int>(e),
                                std::string("set operation (device closure): ") + hipGetErrorString(e));
}

// -------------------------------------------- replace_if, adjacent_difference
// replace.hpp:326,683 with any predicate and adjacent_difference.hpp:194,275
// with any binary operation: the closure kernels of transform
// (device_closures.hpp) with the callable wrapped.  out may be exactly in for
// replace_if; adjacent_difference reads in[i] and in[i-1] as two ranges offset
// by one element, the first element is a one-element copy.  The overlaps the
// C ABI refuses are refused here the same way (INVALID_ARGUMENT, before any
// launch).
// [a, a + n) and [b, b + n) share a byte: the C ABI's refusal (permute.hip),
// made here too because these calls do not pass through it
template <typename T>
bool ranges_overlap(T const* a, T const* b, uint64_t n) {
    const std::uintptr_t x = reinterpret_cast<std::uintptr_t>(a), y = reinterpret_cast<std::uintptr_t>(b);
    const unsigned __int128 len = static_cast<unsigned __int128>(n) * sizeof(T);
    return x < y + len && y < x + len;
}

template <typename T, typename Pred>
struct replace_where {
    Pred pred;
    T nv;
    __device__ __forceinline__ T operator()(T const& x) const { return static_cast<bool>(pred(x)) ? nv : x; }
};

template <typename T, typename Pred>
void replace_if(compute::hip::target const& t, T const* in, T* out, uint64_t n, Pred const& pred, T nv) {
    if (n == 0) return;
    if (in != out && ranges_overlap(in, static_cast<T const*>(out), n))
        compute::hip::detail::check(HPXHIP_ERROR_INVALID_ARGUMENT, "replace_if (device closure): ranges overlap");
    device_transform(t, replace_where<T, std::decay_t<Pred>>{pred, nv}, in, out, n);
}

template <typename T, typename Op>
struct as_difference {
    Op op;
    __device__ __forceinline__ T operator()(T const& x, T const& y) const { return static_cast<T>(op(x, y)); }
};

template <typename T, typename Op>
void adjacent_difference(compute::hip::target const& t, T const* in, T* out, uint64_t n, Op const& op) {
    if (n == 0) return;
    if (ranges_overlap(in, static_cast<T const*>(out), n))
        compute::hip::detail::check(HPXHIP_ERROR_INVALID_ARGUMENT,
                                    "adjacent_difference (device closure): ranges overlap");
    compute::hip::detail::check(hpxhip_copy(compute::hip::dtype_of<T>::value, in, out, 1, t.stream()),
                                "adjacent_difference (device closure)");
    if (n > 1) device_transform2(t, as_difference<T, std::decay_t<Op>>{op}, in + 1, in, out + 1, n - 1);
}

// ------------------------------------------------------------ search family
// find.hpp, all_any_none.hpp, count.hpp, minmax.hpp, equal.hpp, mismatch.hpp
// with any predicate, comparator and projection: the library's kernels
// (search_kernel.hpp) through the library's launchers, instantiated for the
// callable.  Every result is a uint64 in a result slot.
template <typename T, typename Pred>
struct find_source {
    const T* a;
    const T* b;
    Pred pred;
    bool negate;
    __device__ __forceinline__ bool hit(T x) const { return static_cast<bool>(pred(x)) != negate; }
};
template <typename T, typename Pred>
struct mismatch_source {
    const T* a;
    const T* b;
    Pred pred;
    __device__ __forceinline__ bool hit(T x, T y) const { return !static_cast<bool>(pred(x, y)); }
};

inline void search_launched(hipError_t e, char const* what) {
    if (e != hipSuccess)
        throw hpx::kernel_error(static_cast<int>(e), std::string(what) + " (device closure): " + hipGetErrorString(e));
}

// *index_dev <- the smallest i with pred(in[i]) != negate, else n
template <typename T, typename Pred>
void find_if(compute::hip::target const& t, T const* in, uint64_t n, Pred const& pred, bool negate,
             uint64_t* index_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "find (device closure): 4- or 8-byte element types");
    using S = find_source<T, std::decay_t<Pred>>;
    search_launched(K::search_detail::launch_find<T, S, false>(S{in, nullptr, pred, negate}, n, index_dev, stream_of(t)),
                    "find_if");
}

// *index_dev <- the smallest i with !pred(a[i], b[i]), else n
template <typename T, typename Pred>
void mismatch(compute::hip::target const& t, T const* a, T const* b, uint64_t n, Pred const& pred,
              uint64_t* index_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "mismatch (device closure): 4- or 8-byte element types");
    using S = mismatch_source<T, std::decay_t<Pred>>;
    search_launched(K::search_detail::launch_find<T, S, true>(S{a, b, pred}, n, index_dev, stream_of(t)), "mismatch");
}

template <typename T, typename Pred>
void count_if(compute::hip::target const& t, T const* in, uint64_t n, Pred const& pred, uint64_t* count_dev) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "count_if (device closure): 4- or 8-byte element types");
    void* ws = n ? scratch(t, K::reduce_detail::max_blocks(n) * sizeof(uint64_t), "count_if scratch") : nullptr;
    using P = as_bool_pred<T, std::decay_t<Pred>>;
    search_launched(K::search_detail::launch_count<T>(in, n, P{pred}, count_dev, ws, stream_of(t)), "count_if");
}

// WHICH: HPXHIP_X_MIN / MAX / MINMAX; out: one index (two for MINMAX)
template <int WHICH, typename T, typename Comp, typename Proj>
void arg_extreme(compute::hip::target const& t, T const* in, uint64_t n, Comp const& comp, Proj const& proj,
                 uint64_t* out) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "min/max_element (device closure): 4- or 8-byte element types");
    void* ws = n ? scratch(t, K::search_detail::arg_scratch_bytes(n), "minmax_element scratch") : nullptr;
    using L = projected_less<T, std::decay_t<Comp>, std::decay_t<Proj>>;
    search_launched(K::search_detail::launch_arg<T, L, WHICH>(in, n, L{comp, proj}, out, ws, stream_of(t)),
                    "minmax_element");
}
#endif  // HPX_HAVE_HIP_DEVICE_CLOSURES

}  // namespace dev
}}}}  // namespace hpx::parallel::v1::detail
