// compaction.hip -- stable stream compaction: copy_if, partition_copy,
// stable_partition and the remove family (hpx::parallel copy.hpp:401-494,
// partition.hpp:292,1063,1350, remove_copy.hpp:173,350, remove.hpp:290,367)
// over one single-pass kernel and one launcher (compaction_kernel.hpp, which
// also carries the algorithm notes and the aliasing argument).
//
// Reference copy_if: phase 1 writes a bool flag per element
// (boost::shared_array<bool>, copy.hpp:416) and counts hits per chunk, phase 2
// prefixes the counts, phase 3 re-reads input + flags and scatters.  Here: one
// pass, no flag array in HBM.  Traffic per int64 element: 8 B read + 8 B x
// selectivity written (copy_if), 8 B read + 8 B written (partition_copy), plus
// 16 B per rejected element for stable_partition's second step.
//
// hpxhip_copy_if: the one-sided kernel.
// hpxhip_partition_copy: the two-sided kernel; either output may be null or
// exactly the input.  remove_copy_if is the call without out_true, remove_if
// the one with out_false == in, copy_if-in-place the one with out_true == in.
// hpxhip_stable_partition: accepted elements compacted in place, rejected
// ones to scratch, then k_partition_tail reads the count from device memory
// and copies them to [count, n) -- no host round trip.
// hpxhip_unique_copy: the one-sided kernel in its adjacent mode (unique.hpp:
// 311,612).  The reference flags, scans and scatters in three passes; here the
// hit bit of an element is !rel(element before, element), with the element
// before taken from registers, a neighbouring lane or one extra load per wave.
// Traffic as copy_if's: 8 B read + 8 B per kept int64 element.  out == in is
// unique.
#include <cstdlib>

#include "internal.hpp"
#include <hpxhip/kernels/compaction_kernel.hpp>

using namespace hpxhip;
namespace C = hpxhip::compaction_detail;

namespace {

template <typename T>
size_t scratch_total(uint64_t n, bool stable) {
    return C::state_bytes<T>(n) + (stable ? align_up(n * sizeof(T), 256) : 0);
}

// NAME=1 forces the 64-bit look-back value at any n (tests; read per call).
bool env_flag(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}

bool natural(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

// Relations (hpxhip_eqrel).
template <int KIND, typename T>
struct eqrel_fn {
    int a;
    __host__ __device__ __forceinline__ bool operator()(T x, T y) const {
        if constexpr (KIND == HPXHIP_Q_EQUAL) return x == y;
        else return (x >> a) == (y >> a);
    }
};

template <typename T, typename F>
int with_eqrel(int kind, const void* arg, F&& f) {
    switch (kind) {
        case HPXHIP_Q_EQUAL: return f(eqrel_fn<HPXHIP_Q_EQUAL, T>{0});
        case HPXHIP_Q_EQUAL_SHR:
            if constexpr (std::is_integral_v<T>) {
                int32_t a = -1;
                if (arg) __builtin_memcpy(&a, arg, sizeof(a));
                if (a < 0 || a >= static_cast<int32_t>(8 * sizeof(T))) return HPXHIP_ERROR_INVALID_ARGUMENT;
                return f(eqrel_fn<HPXHIP_Q_EQUAL_SHR, T>{a});
            } else {
                return HPXHIP_ERROR_UNSUPPORTED;
            }
        default: return HPXHIP_ERROR_INVALID_ARGUMENT;
    }
}

}  // namespace

namespace hpxhip {
size_t copy_if_scratch_bytes(int dtype, uint64_t n) { return partition_scratch_bytes(dtype, n, false); }
size_t partition_scratch_bytes(int dtype, uint64_t n, bool stable) {
    return dtype_size(dtype) == 8 ? scratch_total<uint64_t>(n, stable) : scratch_total<uint32_t>(n, stable);
}
size_t unique_scratch_bytes(int dtype, uint64_t n) { return partition_scratch_bytes(dtype, n, false); }
}  // namespace hpxhip

extern "C" int hpxhip_copy_if(int dtype, int pred_kind, const void* pred_arg, const void* in, void* out, uint64_t n,
                              uint64_t* count_dev, hpxhip_stream stream, void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_copy_if");
    if (!count_dev || (n && (!in || !out))) return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    if (n == 0) {
        HPXHIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
        return 0;
    }
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return with_pred<T>(pred_kind, pred_arg, [&](auto p) -> int {
            void* ws = nullptr;
            int rc = resolve_scratch(s, scratch, scratch_bytes, scratch_total<T>(n, false), &ws);
            if (rc) return rc;
            return static_cast<int>(C::launch<false>(static_cast<const T*>(in), static_cast<T*>(out),
                                                     static_cast<T*>(nullptr), n, p, count_dev, ws,
                                                     device_error_word(s), current_device_info().cus,
                                                     env_flag("HPXHIP_COPY_IF_STATE64"), s));
        });
    });
}

extern "C" int hpxhip_partition_copy(int dtype, int pred_kind, const void* pred_arg, const void* in, void* out_true,
                                     void* out_false, uint64_t n, uint64_t* count_dev, hpxhip_stream stream,
                                     void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_partition_copy");
    if (!count_dev || (!out_true && !out_false) || out_true == out_false || (n && !in))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !(natural(in, es) && natural(out_true, es) && natural(out_false, es)))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    if (n == 0) {
        HPXHIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
        return 0;
    }
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return with_pred<T>(pred_kind, pred_arg, [&](auto p) -> int {
            void* ws = nullptr;
            int rc = resolve_scratch(s, scratch, scratch_bytes, scratch_total<T>(n, false), &ws);
            if (rc) return rc;
            return static_cast<int>(C::launch<true>(static_cast<const T*>(in), static_cast<T*>(out_true),
                                                    static_cast<T*>(out_false), n, p, count_dev, ws,
                                                    device_error_word(s), current_device_info().cus,
                                                    env_flag("HPXHIP_PARTITION_STATE64"), s));
        });
    });
}

extern "C" int hpxhip_stable_partition(int dtype, int pred_kind, const void* pred_arg, void* data, uint64_t n,
                                       uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                                       size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_stable_partition");
    if (!count_dev || (n && !data)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !natural(data, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    if (n == 0) {
        HPXHIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
        return 0;
    }
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return with_pred<T>(pred_kind, pred_arg, [&](auto p) -> int {
            void* ws = nullptr;
            int rc = resolve_scratch(s, scratch, scratch_bytes, scratch_total<T>(n, true), &ws);
            if (rc) return rc;
            T* d = static_cast<T*>(data);
            T* rej = reinterpret_cast<T*>(static_cast<char*>(ws) + C::state_bytes<T>(n));
            const int cus = current_device_info().cus;
            HPXHIP_CHECK(C::launch<true>(static_cast<const T*>(d), d, rej, n, p, count_dev, ws, device_error_word(s),
                                         cus, env_flag("HPXHIP_PARTITION_STATE64"), s));
            HPXHIP_CHECK(C::launch_tail(rej, d, n, count_dev, cus, s));
            return 0;
        });
    });
}

extern "C" int hpxhip_unique_copy(int dtype, int rel_kind, const void* rel_arg, const void* in, void* out, uint64_t n,
                                  uint64_t* count_dev, hpxhip_stream stream, void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_unique_copy");
    if (!count_dev || (n && (!in || !out))) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !(natural(in, es) && natural(out, es))) return HPXHIP_ERROR_INVALID_ARGUMENT;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        // the relation and the scratch size are checked before the device is touched
        return with_eqrel<T>(rel_kind, rel_arg, [&](auto rel) -> int {
            if (n && scratch && scratch_bytes < scratch_total<T>(n, false)) return HPXHIP_ERROR_INVALID_ARGUMENT;
            hipStream_t s = reinterpret_cast<hipStream_t>(stream);
            device_guard g(s);
            if (g.status) return g.status;
            if (n == 0) {
                HPXHIP_CHECK(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
                return 0;
            }
            void* ws = nullptr;
            int rc = resolve_scratch(s, scratch, scratch_bytes, scratch_total<T>(n, false), &ws);
            if (rc) return rc;
            return static_cast<int>(C::launch<false, true>(static_cast<const T*>(in), static_cast<T*>(out),
                                                           static_cast<T*>(nullptr), n, rel, count_dev, ws,
                                                           device_error_word(s), current_device_info().cus,
                                                           env_flag("HPXHIP_UNIQUE_STATE64"), s));
        });
    });
}
