// set.hip -- hpx::parallel::set_union, set_intersection, set_difference,
// set_symmetric_difference and includes on sorted ranges.  Included by
// merge.hip (one translation unit, one object file).
//
// Reference: set_union.hpp:47, set_intersection.hpp, set_difference.hpp,
// set_symmetric_difference.hpp (sequential forms: std::set_*),
// includes.hpp:129 (std::includes), detail/set_operation.hpp:72-193 (the
// parallel form: std::set_* per chunk into a len1 + len2 buffer, then a
// second copy).  Here: one pass over merge-path tiles with a decoupled
// look-back for the output offsets, see hpxhip/kernels/set_kernel.hpp.
// Keys are compared through the radix sort's ordered bit patterns
// (sort_kernel.hpp: integers as std::less, floats in IEEE total order), so
// sort + set operation agree on every dtype.  Traffic: each input read once,
// the kept elements written once.
#include "internal.hpp"
#include <hpxhip/kernels/set_kernel.hpp>

using namespace hpxhip;

namespace hpxhip {
size_t set_operation_scratch_bytes(uint64_t n) { return set_detail::scratch_bytes(n); }
}  // namespace hpxhip

namespace {

template <typename T, bool DESC>
int run_set(int op, const void* a, uint64_t na, const void* b, uint64_t nb, void* out, uint64_t* count_dev,
            hipStream_t s, void* scratch, size_t scratch_bytes) {
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;
    using C = merge_detail::key_less<ordered_bits<T, DESC>>;
    void* ws = nullptr;
    int rc = resolve_scratch(s, scratch, scratch_bytes, set_detail::scratch_bytes(na + nb), &ws);
    if (rc) return rc;
    HPXHIP_CHECK(set_detail::launch(static_cast<const U*>(a), na, static_cast<const U*>(b), nb, static_cast<U*>(out),
                                    op, C{}, count_dev, ws, device_error_word(s), s));
    return 0;
}

}  // namespace

extern "C" {

int hpxhip_set_operation(int dtype, int op, const void* in1, uint64_t n1, const void* in2, uint64_t n2, void* out,
                         int descending, uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                         size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_set_operation");
    if (!count_dev || (n1 && !in1) || (n2 && !in2)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (op < HPXHIP_SET_UNION || op > HPXHIP_SET_SYMMETRIC_DIFFERENCE) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (dtype_size(dtype) == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    if (n1 + n2 == 0) {
        HPXHIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
        return 0;
    }
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        if (descending) return run_set<T, true>(op, in1, n1, in2, n2, out, count_dev, s, scratch, scratch_bytes);
        return run_set<T, false>(op, in1, n1, in2, n2, out, count_dev, s, scratch, scratch_bytes);
    });
}

}  // extern "C"
