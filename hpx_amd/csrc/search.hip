// search.hip -- the search family of the C ABI: hpxhip_find_if (find, find_if,
// find_if_not, all_of, any_of, none_of), hpxhip_mismatch (equal, mismatch),
// hpxhip_count_if (count, count_if) and hpxhip_minmax_element (min_element,
// max_element, minmax_element).
//
// The reference runs these on the host partitioner: find.hpp:70,216,382 walk
// chunks under a util::cancellation_token that carries the smallest hit so
// far, count.hpp sums per-chunk counts, minmax.hpp:46-66,277,513-541 fold
// per-chunk extremes.  Here every call reads each byte once at the geometry of
// the reduce kernel (include/hpxhip/kernels/search_kernel.hpp has the
// kernels, the early-exit argument, the tie rules and the NaN statement):
//   * find / mismatch: the result word is the caller's device uint64; blocks
//     fold their smallest hit in with one agent-scope atomic min and skip
//     their loads once a hit below them is known -- the cancellation token as
//     a hint that nothing waits on;
//   * count_if: the reduce kernel itself over `pred(x) ? 1 : 0`;
//   * min/max/minmax_element: (value, index) pairs, one partial per block, a
//     one-block fold in a fixed order.
// Part of reduce.hip's translation unit (included at its end): the family is
// a set of reductions over reduce_kernel.hpp, and the library keeps one code
// object per kernel family.
#include "internal.hpp"
#include <hpxhip/kernels/search_kernel.hpp>

namespace {

namespace sd = hpxhip::search_detail;

bool elem_aligned(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

// find's unary source: pred(x) != negate
template <typename T, typename Pred>
struct find_source {
    const T* a;
    const T* b;
    Pred pred;
    bool negate;
    __device__ __forceinline__ bool hit(T x) const { return pred(x) != negate; }
};
// mismatch's binary source: !(x == y) by value (a NaN differs from itself)
template <typename T>
struct mismatch_source {
    const T* a;
    const T* b;
    __device__ __forceinline__ bool hit(T x, T y) const { return !(x == y); }
};

struct cmp_less {
    template <typename T>
    __device__ __forceinline__ bool operator()(T a, T b) const { return a < b; }
};
struct cmp_greater {
    template <typename T>
    __device__ __forceinline__ bool operator()(T a, T b) const { return a > b; }
};

}  // namespace

namespace hpxhip {
size_t count_if_scratch_bytes(uint64_t n) { return reduce_scratch_bytes(n); }
size_t minmax_element_scratch_bytes(uint64_t n) { return search_detail::arg_scratch_bytes(n); }
}  // namespace hpxhip

extern "C" {

int hpxhip_find_if(int dtype, int pred_kind, const void* pred_arg, int negate, const void* in, uint64_t n,
                   uint64_t* index_dev, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_find_if");
    using namespace hpxhip;
    if (!index_dev || !elem_aligned(index_dev, 8) || (n && !in)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !elem_aligned(in, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        // the predicate is checked before the device is touched
        return with_pred<T>(pred_kind, pred_arg, [&](auto pred) -> int {
            hipStream_t s = reinterpret_cast<hipStream_t>(stream);
            device_guard g(s);
            if (g.status) return g.status;
            using S = find_source<T, decltype(pred)>;
            return static_cast<int>(
                sd::launch_find<T, S, false>(S{static_cast<const T*>(in), nullptr, pred, negate != 0}, n, index_dev, s));
        });
    });
}

int hpxhip_mismatch(int dtype, const void* in1, const void* in2, uint64_t n, uint64_t* index_dev,
                    hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_mismatch");
    using namespace hpxhip;
    if (!index_dev || !elem_aligned(index_dev, 8) || (n && (!in1 || !in2))) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !(elem_aligned(in1, es) && elem_aligned(in2, es))) return HPXHIP_ERROR_INVALID_ARGUMENT;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        device_guard g(s);
        if (g.status) return g.status;
        using S = mismatch_source<T>;
        return static_cast<int>(
            sd::launch_find<T, S, true>(S{static_cast<const T*>(in1), static_cast<const T*>(in2)}, n, index_dev, s));
    });
}

int hpxhip_count_if(int dtype, int pred_kind, const void* pred_arg, const void* in, uint64_t n, uint64_t* count_dev,
                    hpxhip_stream stream, void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_count_if");
    using namespace hpxhip;
    if (!count_dev || !elem_aligned(count_dev, 8) || (n && !in)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !elem_aligned(in, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        // the predicate and the scratch size are checked before the device is touched
        return with_pred<T>(pred_kind, pred_arg, [&](auto pred) -> int {
            if (n && scratch && scratch_bytes < count_if_scratch_bytes(n)) return HPXHIP_ERROR_INVALID_ARGUMENT;
            hipStream_t s = reinterpret_cast<hipStream_t>(stream);
            device_guard g(s);
            if (g.status) return g.status;
            void* ws = nullptr;
            if (n) {
                int rc = resolve_scratch(s, scratch, scratch_bytes, count_if_scratch_bytes(n), &ws);
                if (rc) return rc;
            }
            return static_cast<int>(sd::launch_count<T>(static_cast<const T*>(in), n, pred, count_dev, ws, s));
        });
    });
}

int hpxhip_minmax_element(int dtype, int which, int descending, const void* in, uint64_t n, uint64_t* index_dev,
                          hpxhip_stream stream, void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_minmax_element");
    using namespace hpxhip;
    if (!index_dev || !elem_aligned(index_dev, 8) || (n && !in)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (which != HPXHIP_X_MIN && which != HPXHIP_X_MAX && which != HPXHIP_X_MINMAX)
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !elem_aligned(in, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        if (n && scratch && scratch_bytes < minmax_element_scratch_bytes(n)) return HPXHIP_ERROR_INVALID_ARGUMENT;
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        device_guard g(s);
        if (g.status) return g.status;
        void* ws = nullptr;
        if (n) {
            int rc = resolve_scratch(s, scratch, scratch_bytes, minmax_element_scratch_bytes(n), &ws);
            if (rc) return rc;
        }
        const T* p = static_cast<const T*>(in);
        auto run = [&](auto comp) -> int {
            using C = decltype(comp);
            switch (which) {
                case HPXHIP_X_MIN: return static_cast<int>(sd::launch_arg<T, C, sd::kArgMin>(p, n, comp, index_dev, ws, s));
                case HPXHIP_X_MAX: return static_cast<int>(sd::launch_arg<T, C, sd::kArgMax>(p, n, comp, index_dev, ws, s));
                default: return static_cast<int>(sd::launch_arg<T, C, sd::kArgMinMax>(p, n, comp, index_dev, ws, s));
            }
        };
        return descending ? run(cmp_greater{}) : run(cmp_less{});
    });
}

}  // extern "C"
