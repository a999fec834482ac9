// permute.hip -- hpx::parallel::reverse, reverse_copy, rotate, rotate_copy,
// swap_ranges, replace(_if), replace_copy(_if) and adjacent_difference.
// Included by elementwise.hip (one translation unit, one object file): the
// cuts are that file's make_span / make_span_shifted, replace_if runs on its
// launch_unary.
//
// Reference: reverse.hpp:44-79,155,191; rotate.hpp:57-100 (rotate_helper:
// three reversals), 219-268; swap_ranges.hpp:128; replace.hpp:164,326,493,683;
// adjacent_difference.hpp:99,194,275.  The reference runs each through its
// partitioner with one loop iteration per element; here they are streaming
// kernels (hpxhip/kernels/permute_kernel.hpp).  Traffic per element of size
// s: reverse, reverse_copy, rotate_copy, replace_if, adjacent_difference
// s read + s written; swap_ranges 2 s + 2 s; rotate two launches of s + s.
// No entry point takes scratch.  Every argument is checked on the host before
// the first device call.
#include "internal.hpp"
#include <hpxhip/kernels/permute_kernel.hpp>

namespace {

namespace PK = hpxhip::permute_detail;
static_assert(PK::kThreads == kRwThreads, "permute kernels use the read + write block size");

inline bool elem_aligned(const void* p, size_t es) { return reinterpret_cast<uintptr_t>(p) % es == 0; }
// [a, a + bytes) and [b, b + bytes) share a byte
inline bool ranges_overlap(const void* a, const void* b, uint64_t n, size_t es) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    const unsigned __int128 len = static_cast<unsigned __int128>(n) * es;
    return x < y + len && y < x + len;
}

inline PK::cut to_cut(const span3& sp) { return PK::cut{sp.head, sp.nvec, sp.tail}; }
inline PK::cut scalar_cut(uint64_t n) { return PK::cut{n, 0, 0}; }  // one element per thread
// blocks of one job; two jobs share a grid of at most 2^31-1 blocks
inline unsigned job_blocks(uint64_t items) {
    if (items == 0) return 0;
    const uint64_t b = (items + kRwThreads - 1) / kRwThreads;
    return static_cast<unsigned>(b > 0x3fffffffull ? 0x3fffffffull : b);
}

template <typename T>
PK::copy_job<T> make_copy_job(const T* in, T* out, uint64_t len) {
    constexpr int V = 16 / sizeof(T);
    PK::copy_job<T> j{in, out, PK::cut{0, 0, 0}, 0, 0};
    if (len == 0) return j;
    span3 sp;
    int sh[1] = {0};
    if (make_span<V>(len, sizeof(T), &sp, {in, out})) j.c = to_cut(sp);
    else if (make_span_shifted<V>(len, sizeof(T), &sp, out, {in}, sh)) j.c = to_cut(sp), j.sh = sh[0];
    else j.c = scalar_cut(len);  // too short for the shifted path
    j.blocks = job_blocks(j.c.items());
    return j;
}

template <typename T>
PK::reverse_job<T> make_reverse_job(T* d, uint64_t n) {
    constexpr int V = 16 / sizeof(T);
    PK::reverse_job<T> j{d, n, PK::cut{0, 0, 0}, 0, 0};
    if (n < 2) return j;
    span3 sp;
    if (!make_span<V>(n / 2, sizeof(T), &sp, {d})) sp = span3{n / 2, 0, 0};
    j.c = to_cut(sp);
    j.back_vec = (reinterpret_cast<uintptr_t>(d) + (n - sp.head) * sizeof(T)) % 16 == 0;
    j.blocks = job_blocks(j.c.items());
    return j;
}

template <typename T>
int launch_reverse2(T* a, uint64_t na, T* b, uint64_t nb, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    const PK::reverse_job<T> ja = make_reverse_job(a, na), jb = make_reverse_job(b, nb);
    if (ja.blocks + jb.blocks == 0) return 0;
    hipLaunchKernelGGL((PK::k_reverse2<T, V>), dim3(ja.blocks + jb.blocks), dim3(kRwThreads), 0, s, ja, jb);
    HPXHIP_CHECK_LAUNCH();
    return 0;
}

template <typename P, typename T>
struct replace_fn {
    P pred;
    T nv;
    __host__ __device__ __forceinline__ T operator()(T x) const { return pred(x) ? nv : x; }
};

// dtype and kind checks that need no device: 0, INVALID_ARGUMENT or UNSUPPORTED
int check_pred(int dtype, int kind) {
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return with_pred<T>(kind, nullptr, [](auto) -> int { return 0; });
    });
}
int check_binary(int dtype, int kind) {
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return with_binary<T>(kind, nullptr, [](auto) -> int { return 0; });
    });
}

}  // namespace

extern "C" {

int hpxhip_reverse(int dtype, void* data, uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_reverse");
    const size_t es = dtype_size(dtype);
    if (es == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    if (!data || !elem_aligned(data, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        return launch_reverse2<T>(static_cast<T*>(data), n, nullptr, 0, s);
    });
}

int hpxhip_reverse_copy(int dtype, const void* in, void* out, uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_reverse_copy");
    const size_t es = dtype_size(dtype);
    if (es == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    if (!in || !out || !elem_aligned(in, es) || !elem_aligned(out, es) || ranges_overlap(in, out, n, es))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        constexpr int V = 16 / sizeof(T);
        span3 sp;
        PK::cut c = scalar_cut(n);
        int sh = 0;
        if (make_span<V>(n, sizeof(T), &sp, {out})) {
            // offset inside 16 B of the window that mirrors an output vector
            sh = static_cast<int>(((reinterpret_cast<uintptr_t>(in) + (n - sp.head) * sizeof(T)) % 16) / sizeof(T));
            if (sh == 0) c = to_cut(sp);
            else if (make_span_shifted<V>(n, sizeof(T), &sp, out, {}, nullptr)) c = to_cut(sp);
            else sh = 0;  // too short for the shifted path: one element per thread
        }
        hipLaunchKernelGGL((PK::k_reverse_copy<T, V>), dim3(grid_for(c.items(), kRwThreads)), dim3(kRwThreads), 0, s,
                           static_cast<const T*>(in), static_cast<T*>(out), n, c, sh);
        HPXHIP_CHECK_LAUNCH();
        return 0;
    });
}

int hpxhip_rotate(int dtype, void* data, uint64_t mid, uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_rotate");
    const size_t es = dtype_size(dtype);
    if (es == 0 || mid > n) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    if (!data || !elem_aligned(data, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (mid == 0 || mid == n) return 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        T* d = static_cast<T*>(data);
        // rotate.hpp:68-100: reverse [0, mid) and [mid, n) (one launch), then [0, n)
        if (int rc = launch_reverse2<T>(d, mid, d + mid, n - mid, s)) return rc;
        return launch_reverse2<T>(d, n, nullptr, 0, s);
    });
}

int hpxhip_rotate_copy(int dtype, const void* in, uint64_t mid, uint64_t n, void* out, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_rotate_copy");
    const size_t es = dtype_size(dtype);
    if (es == 0 || mid > n) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    if (!in || !out || !elem_aligned(in, es) || !elem_aligned(out, es) || ranges_overlap(in, out, n, es))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        constexpr int V = 16 / sizeof(T);
        const T* i = static_cast<const T*>(in);
        T* o = static_cast<T*>(out);
        // out[0, n - mid) = in[mid, n), out[n - mid, n) = in[0, mid)
        const PK::copy_job<T> ja = make_copy_job(i + mid, o, n - mid), jb = make_copy_job(i, o + (n - mid), mid);
        hipLaunchKernelGGL((PK::k_copy2<T, V>), dim3(ja.blocks + jb.blocks), dim3(kRwThreads), 0, s, ja, jb);
        HPXHIP_CHECK_LAUNCH();
        return 0;
    });
}

int hpxhip_swap_ranges(int dtype, void* a, void* b, uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_swap_ranges");
    const size_t es = dtype_size(dtype);
    if (es == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (n == 0) return 0;
    if (!a || !b || !elem_aligned(a, es) || !elem_aligned(b, es) || ranges_overlap(a, b, n, es))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        constexpr int V = 16 / sizeof(T);
        T* pa = static_cast<T*>(a);
        T* pb = static_cast<T*>(b);
        span3 sp;
        if (make_span<V>(n, sizeof(T), &sp, {a, b})) {
            hipLaunchKernelGGL((PK::k_swap<T, V, true>), dim3(grid_for(sp.head + sp.nvec + sp.tail, kRwThreads)),
                               dim3(kRwThreads), 0, s, pa, pb, to_cut(sp));
        } else {
            // the ranges differ in their offset inside 16 B: b in vectors, a element-wide
            if (!make_span<V>(n, sizeof(T), &sp, {b})) sp = span3{n, 0, 0};
            hipLaunchKernelGGL((PK::k_swap<T, V, false>), dim3(grid_for(sp.head + sp.nvec + sp.tail, kRwThreads)),
                               dim3(kRwThreads), 0, s, pa, pb, to_cut(sp));
        }
        HPXHIP_CHECK_LAUNCH();
        return 0;
    });
}

int hpxhip_replace_if(int dtype, int pred_kind, const void* pred_arg, const void* new_value, const void* in,
                      void* out, uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_replace_if");
    const size_t es = dtype_size(dtype);
    if (es == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (int rc = check_pred(dtype, pred_kind)) return rc;
    if (n == 0) return 0;
    if (!pred_arg || !new_value || !in || !out || !elem_aligned(in, es) || !elem_aligned(out, es))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (in != out && ranges_overlap(in, out, n, es)) return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        T nv;
        __builtin_memcpy(&nv, new_value, sizeof(T));
        return with_pred<T>(pred_kind, pred_arg, [&](auto p) -> int {
            return launch_unary<T, T, T>(static_cast<const T*>(in), static_cast<T*>(out), n,
                                         replace_fn<decltype(p), T>{p, nv}, s);
        });
    });
}

int hpxhip_adjacent_difference(int dtype, int binary_kind, const void* scalars, const void* in, void* out,
                               uint64_t n, hpxhip_stream stream) {
    HPXHIP_ANNOTATE("hpxhip_adjacent_difference");
    const size_t es = dtype_size(dtype);
    if (es == 0) return HPXHIP_ERROR_INVALID_ARGUMENT;
    if (int rc = check_binary(dtype, binary_kind)) return rc;
    if (n == 0) return 0;
    if (!in || !out || !elem_aligned(in, es) || !elem_aligned(out, es) || ranges_overlap(in, out, n, es))
        return HPXHIP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    device_guard g(s);
    if (g.status) return g.status;
    return with_dtype(dtype, [&](auto t) -> int {
        using T = typename decltype(t)::type;
        constexpr int V = 16 / sizeof(T);
        return with_binary<T>(binary_kind, scalars, [&](auto f) -> int {
            const T* i = static_cast<const T*>(in);
            T* o = static_cast<T*>(out);
            // the n - 1 differences out[1 + k] = f(in[k + 1], in[k]); out[0] rides along
            span3 sp;
            int sh[1] = {0};
            PK::cut c = scalar_cut(n - 1);
            if (make_span_shifted<V>(n - 1, sizeof(T), &sp, o + 1, {i}, sh)) c = to_cut(sp);
            else sh[0] = 0;
            hipLaunchKernelGGL((PK::k_adjacent_difference<T, decltype(f), V>),
                               dim3(grid_for(c.items(), kRwThreads)), dim3(kRwThreads), 0, s, i, o, c, sh[0], f);
            HPXHIP_CHECK_LAUNCH();
            return 0;
        });
    });
}

}  // extern "C"
