// partition.hip -- partition_copy, stable_partition and the remove family
// (hpx::parallel partition.hpp:292,1063,1350, remove_copy.hpp:173,350,
// remove.hpp:290,367) over one single-pass two-sided compaction kernel
// (partition_kernel.hpp, which also carries the aliasing argument).
//
// hpxhip_partition_copy: one kernel; either output may be null or exactly
// the input.  remove_copy_if is the call without out_true, remove_if the one
// with out_false == in, copy_if-in-place the one with out_true == in.
// hpxhip_stable_partition: accepted elements compacted in place, rejected
// ones to scratch, then k_partition_tail reads the count from device memory
// and copies them to [count, n) -- no host round trip.
// Traffic per int64 element: 8 B read + 8 B written (partition_copy), plus
// 16 B per rejected element for stable_partition's second step.
// Misaligned inputs as in copy_if.hip: a split-off head (< 16 B) whose
// accepted count seeds tile 0 and whose length enters the rejected side's
// offset, or the element-wise form.
//
// Compiled as part of copy_if.hip's object (included at its end): the two
// compaction kernels share one offload bundle, and the library keeps one
// bundle per listed source.  Everything file-local lives in partition_impl
// and names the kernel header's namespace explicitly, so nothing here
// depends on what copy_if.hip brings into scope.
#include <cstdlib>

#include "internal.hpp"
#include <hpxhip/kernels/partition_kernel.hpp>

using namespace hpxhip;

namespace {
namespace partition_impl {

using hpxhip::tile_state;
namespace PD = hpxhip::partition_detail;

constexpr size_t kSlotsOff = 256;  // [counter | tile slots], zeroed per call

// [counter | tile slots | head count | stable_partition: n rejected elements]
template <typename T>
size_t head_count_off(uint64_t n) {
    return align_up(kSlotsOff + PD::ntiles_for<T>(n) * tile_state<uint64_t>::bytes_per_tile(), 256);
}
template <typename T>
size_t rejected_off(uint64_t n) {
    return head_count_off<T>(n) + 256;
}
template <typename T>
size_t scratch_total(uint64_t n, bool stable) {
    return rejected_off<T>(n) + (stable ? align_up(n * sizeof(T), 256) : 0);
}

template <typename T, bool ALIGNED, typename SV, typename P>
int launch_partition_sv(const T* in, T* out_true, T* out_false, uint64_t n, uint64_t head, P p, uint64_t* count_dev,
                        char* ws, hipStream_t s, const uint64_t* prefix0) {
    const uint64_t ntiles = PD::ntiles_for<T>(n);
    HPXHIP_CHECK(hipMemsetAsync(ws, 0, kSlotsOff + ntiles * tile_state<SV>::bytes_per_tile(), s));
    tile_state<SV> st{reinterpret_cast<uint64_t*>(ws + kSlotsOff), device_error_word(s)};
    // one persistent workgroup per CU (its stage is 128 of the CU's 160 KiB of LDS)
    const uint64_t grid = std::min<uint64_t>(ntiles, static_cast<uint64_t>(current_device_info().cus));
    hipLaunchKernelGGL((PD::k_partition<T, P, ALIGNED, SV>), dim3(static_cast<unsigned>(grid)), dim3(PD::kThreads), 0,
                       s, in, out_true, out_false, n, head, p, count_dev, reinterpret_cast<uint32_t*>(ws), st, ntiles,
                       prefix0);
    HPXHIP_CHECK_LAUNCH();
    return 0;
}

template <typename T, bool ALIGNED, typename P>
int launch_partition(const T* in, T* out_true, T* out_false, uint64_t n, uint64_t head, P p, uint64_t* count_dev,
                     char* ws, hipStream_t s, const uint64_t* prefix0 = nullptr) {
    // HPXHIP_PARTITION_STATE64=1 forces the 64-bit form at any n (tests; read per call).
    const char* e = getenv("HPXHIP_PARTITION_STATE64");
    const bool force64 = e && e[0] == '1';
    if (n + head < (uint64_t{1} << 32) && !force64)
        return launch_partition_sv<T, ALIGNED, uint32_t>(in, out_true, out_false, n, head, p, count_dev, ws, s,
                                                         prefix0);
    return launch_partition_sv<T, ALIGNED, uint64_t>(in, out_true, out_false, n, head, p, count_dev, ws, s, prefix0);
}

// n > 0; ws holds scratch_total<T>(n, ...) bytes.
template <typename T, typename P>
int partition_any(const T* ip, T* ot, T* of, uint64_t n, P p, uint64_t* count_dev, char* ws, hipStream_t s) {
    const uint64_t h = head_to_align16(ip, sizeof(T));
    if (h == 0) return launch_partition<T, true>(ip, ot, of, n, 0, p, count_dev, ws, s);
    if (n > 4 * h) {
        auto* hc = reinterpret_cast<uint64_t*>(ws + head_count_off<T>(n));
        hipLaunchKernelGGL((PD::k_partition_head<T, P>), dim3(1), dim3(64), 0, s, ip, ot, of, h, p, hc);
        HPXHIP_CHECK_LAUNCH();
        return launch_partition<T, true>(ip + h, ot, of, n - h, h, p, count_dev, ws, s, hc);
    }
    return launch_partition<T, false>(ip, ot, of, n, 0, p, count_dev, ws, s);
}

bool natural(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

}  // namespace partition_impl
}  // namespace

namespace hpxhip {
size_t partition_scratch_bytes(int dtype, uint64_t n, bool stable) {
    namespace I = partition_impl;
    return dtype_size(dtype) == 8 ? I::scratch_total<uint64_t>(n, stable) : I::scratch_total<uint32_t>(n, stable);
}
}  // namespace hpxhip

extern "C" int hpxhip_partition_copy(int dtype, int pred_kind, const void* pred_arg, const void* in, void* out_true,
                                     void* out_false, uint64_t n, uint64_t* count_dev, hpxhip_stream stream,
                                     void* scratch, size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_partition_copy");
    namespace I = partition_impl;
    if (!count_dev || (!out_true && !out_false) || out_true == out_false || (n && !in))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !(I::natural(in, es) && I::natural(out_true, es) && I::natural(out_false, es)))
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
            int rc = resolve_scratch(s, scratch, scratch_bytes, I::scratch_total<T>(n, false), &ws);
            if (rc) return rc;
            return I::partition_any<T>(static_cast<const T*>(in), static_cast<T*>(out_true),
                                       static_cast<T*>(out_false), n, p, count_dev, static_cast<char*>(ws), s);
        });
    });
}

extern "C" int hpxhip_stable_partition(int dtype, int pred_kind, const void* pred_arg, void* data, uint64_t n,
                                       uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                                       size_t scratch_bytes) {
    HPXHIP_ANNOTATE("hpxhip_stable_partition");
    namespace I = partition_impl;
    namespace PD = hpxhip::partition_detail;
    if (!count_dev || (n && !data)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    const size_t es = dtype_size(dtype);
    if (es && !I::natural(data, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
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
            int rc = resolve_scratch(s, scratch, scratch_bytes, I::scratch_total<T>(n, true), &ws);
            if (rc) return rc;
            char* base = static_cast<char*>(ws);
            T* d = static_cast<T*>(data);
            T* rej = reinterpret_cast<T*>(base + I::rejected_off<T>(n));
            rc = I::partition_any<T>(d, d, rej, n, p, count_dev, base, s);
            if (rc) return rc;
            const uint64_t nvec = n / (16 / sizeof(T)) + 1;
            const uint64_t blocks = std::min<uint64_t>((nvec + PD::kTailThreads - 1) / PD::kTailThreads,
                                                       static_cast<uint64_t>(current_device_info().cus) * 8);
            hipLaunchKernelGGL((PD::k_partition_tail<T>), dim3(static_cast<unsigned>(blocks)), dim3(PD::kTailThreads),
                               0, s, rej, d, n, count_dev);
            HPXHIP_CHECK_LAUNCH();
            return 0;
        });
    });
}
