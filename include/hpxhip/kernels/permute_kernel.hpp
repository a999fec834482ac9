// permute_kernel.hpp -- the kernels behind reverse, reverse_copy, rotate,
// rotate_copy, swap_ranges and adjacent_difference (hpx/parallel/algorithms/
// reverse.hpp, rotate.hpp, swap_ranges.hpp, adjacent_difference.hpp).
//
// Pure bandwidth kernels in the shape of the elementwise ones (elementwise.hip):
// 64-thread blocks, one 16-B vector per thread per array, a flat grid that
// only strides past 2^31-1 blocks, 64-bit indices, nontemporal 16-B accesses.
// Every range is cut into [head | nvec vectors | tail] (`cut`): the head
// brings the array that is written with 16-B stores to a 1-KiB boundary, head
// and tail are done one element per thread by the first threads of the range's
// blocks.  A kernel that serves two ranges in one launch (rotate_copy's two
// copies, rotate's two reversals) gives each range its own run of blocks.
//
// What is new against the forward walks is the mirrored access:
//   * reverse_copy reads the window that mirrors an aligned output vector.
//     That window is 16-B aligned for one value of (in + n) % 16 only; else it
//     is composed from the two aligned vectors around it (ld_shifted), which
//     is safe because the input is only read;
//   * reverse in place cannot compose: the neighbouring vector is being
//     written by another thread.  Ownership rule: the pair (i, n-1-i),
//     i < n/2, belongs to the one thread whose front item holds i; a thread
//     reads both sides of all its pairs before it writes any of them, and no
//     element belongs to two threads, so no thread ever reads or writes
//     another thread's element.  The front side is always 16-B vectors at
//     1-KiB aligned wave runs.  The back side is 16-B vectors when the
//     mirrored window is aligned ((first + last + 1 element) % 16 == 0), and
//     element-wide loads and stores of exactly the owned elements otherwise.
//     The pairs left between the last whole front vector and the centre
//     (fewer than V) are done one pair per thread, for i < n/2 only; the
//     middle element of an odd range is never touched.
//   * swap_ranges writes both ranges: 16-B on both when they share their
//     offset inside 16 B, else 16-B on b and element-wide on a.
#pragma once

#include <hpxhip/kernels/common.hpp>

namespace hpxhip { namespace permute_detail {

constexpr int kThreads = 64;  // read + write streams, as elementwise.hip's kRwThreads

// [0, n) = [0, head) + nvec vectors of V + tail elements
struct cut {
    uint64_t head, nvec, tail;
    __host__ __device__ uint64_t items() const { return head + nvec + tail; }
};

// ---------------------------------------------------------------- copies
// One forward copy out[i] = in[i]: `sh` is the offset (in elements) of
// in + head inside 16 B; sh != 0 reads the aligned vector pair (i, i + 1), so
// the host keeps the last vector in the tail and head >= V (ld_shifted).
template <typename T>
struct copy_job {
    const T* in;
    T* out;
    cut c;
    int sh;
    unsigned blocks;  // blocks that serve this job
};

template <typename T, int V>
__device__ __forceinline__ void copy_range(const copy_job<T>& j, uint64_t tid, uint64_t stride) {
    using VT = vec<T, V>;
    if (tid < j.c.head) j.out[tid] = j.in[tid];
    const uint64_t tail0 = j.c.head + j.c.nvec * V;
    if (tid < j.c.tail) j.out[tail0 + tid] = j.in[tail0 + tid];
    const VT* vin = reinterpret_cast<const VT*>(j.in + j.c.head - j.sh);
    VT* vout = reinterpret_cast<VT*>(j.out + j.c.head);
    for (uint64_t i = tid; i < j.c.nvec; i += stride) st_stream(&vout[i], ld_shifted<T, V>(vin, i, j.sh));
}

// rotate_copy (rotate.hpp:219-268): two copies with different offsets in one
// launch; blocks [0, a.blocks) serve a, the rest b.
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void k_copy2(copy_job<T> a, copy_job<T> b) {
    if (blockIdx.x < a.blocks) {
        copy_range<T, V>(a, static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x,
                         static_cast<uint64_t>(a.blocks) * kThreads);
    } else {
        copy_range<T, V>(b, static_cast<uint64_t>(blockIdx.x - a.blocks) * kThreads + threadIdx.x,
                         static_cast<uint64_t>(b.blocks) * kThreads);
    }
}

// reverse_copy (reverse.hpp:155,191): out[i] = in[n-1-i].  c cuts the OUTPUT;
// output vector i mirrors the input window that starts at element
// n - head - (i + 1) V, i.e. vector nvec-1-i of the array that starts at
// in + tail - sh (16-B aligned), shifted by sh.  sh != 0: tail >= sh and
// head + sh >= V keep the pair inside the range (the host's shifted cut).
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void k_reverse_copy(const T* in, T* out, uint64_t n, cut c, int sh) {
    using VT = vec<T, V>;
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    if (tid < c.head) out[tid] = in[n - 1 - tid];
    const uint64_t tail0 = c.head + c.nvec * V;
    if (tid < c.tail) out[tail0 + tid] = in[n - 1 - (tail0 + tid)];
    const VT* vin = reinterpret_cast<const VT*>(in + c.tail - sh);
    VT* vout = reinterpret_cast<VT*>(out + c.head);
    for (uint64_t i = tid; i < c.nvec; i += stride) {
        const VT x = ld_shifted<T, V>(vin, c.nvec - 1 - i, sh);
        VT y;
#pragma unroll
        for (int e = 0; e < V; ++e) y.v[e] = x.v[V - 1 - e];
        st_stream(&vout[i], y);
    }
}

// ------------------------------------------------------- reverse in place
// One reversal of data[0, n): c cuts the FRONT HALF [0, n/2) (head to the
// 1-KiB boundary of data); back_vec says the mirrored windows are 16-B
// aligned.  See the ownership rule at the top of the file.
template <typename T>
struct reverse_job {
    T* data;
    uint64_t n;
    cut c;
    int back_vec;
    unsigned blocks;
};

template <typename T, int V>
__device__ __forceinline__ void reverse_range(const reverse_job<T>& j, uint64_t tid, uint64_t stride) {
    using VT = vec<T, V>;
    T* d = j.data;
    const uint64_t last = j.n - 1;
    if (tid < j.c.head) {
        const T x = d[tid], y = d[last - tid];
        d[tid] = y;
        d[last - tid] = x;
    }
    const uint64_t tail0 = j.c.head + j.c.nvec * V;
    if (tid < j.c.tail) {
        const uint64_t i = tail0 + tid;
        const T x = d[i], y = d[last - i];
        d[i] = y;
        d[last - i] = x;
    }
    VT* vf = reinterpret_cast<VT*>(d + j.c.head);
    if (j.back_vec) {
        // window of front vector i: elements [n - head - (i + 1) V, + V)
        for (uint64_t i = tid; i < j.c.nvec; i += stride) {
            VT* vb = reinterpret_cast<VT*>(d + (j.n - j.c.head - (i + 1) * V));
            const VT x = ld_stream(&vf[i]);
            const VT w = ld_stream(vb);
            VT y, r;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                y.v[e] = w.v[V - 1 - e];
                r.v[e] = x.v[V - 1 - e];
            }
            st_stream(&vf[i], y);
            st_stream(vb, r);
        }
    } else {
        for (uint64_t i = tid; i < j.c.nvec; i += stride) {
            T* b = d + (last - (j.c.head + i * V));  // mirror of the vector's element 0; element e at b[-e]
            const VT x = ld_stream(&vf[i]);
            VT y;
#pragma unroll
            for (int e = 0; e < V; ++e) y.v[e] = *(b - e);
            st_stream(&vf[i], y);
#pragma unroll
            for (int e = 0; e < V; ++e) *(b - e) = x.v[e];
        }
    }
}

// reverse (reverse.hpp:44-79) with b.blocks == 0; the first step of rotate
// (rotate.hpp:68-100: both parts reversed) with two jobs.
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void k_reverse2(reverse_job<T> a, reverse_job<T> b) {
    if (blockIdx.x < a.blocks) {
        reverse_range<T, V>(a, static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x,
                            static_cast<uint64_t>(a.blocks) * kThreads);
    } else {
        reverse_range<T, V>(b, static_cast<uint64_t>(blockIdx.x - a.blocks) * kThreads + threadIdx.x,
                            static_cast<uint64_t>(b.blocks) * kThreads);
    }
}

// ------------------------------------------------------------ swap_ranges
// swap_ranges.hpp:128: a[i] <-> b[i].  c cuts b (16-B stores at 1-KiB wave
// runs); A_VEC: a shares b's offset inside 16 B and is swapped in vectors
// too, else a thread swaps exactly its V elements of a element-wide.
template <typename T, int V, bool A_VEC>
__global__ __launch_bounds__(kThreads) void k_swap(T* a, T* b, cut c) {
    using VT = vec<T, V>;
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    if (tid < c.head) {
        const T x = a[tid], y = b[tid];
        a[tid] = y;
        b[tid] = x;
    }
    const uint64_t tail0 = c.head + c.nvec * V;
    if (tid < c.tail) {
        const T x = a[tail0 + tid], y = b[tail0 + tid];
        a[tail0 + tid] = y;
        b[tail0 + tid] = x;
    }
    VT* vb = reinterpret_cast<VT*>(b + c.head);
    for (uint64_t i = tid; i < c.nvec; i += stride) {
        const VT y = ld_stream(&vb[i]);
        if constexpr (A_VEC) {
            VT* va = reinterpret_cast<VT*>(a + c.head);
            const VT x = ld_stream(&va[i]);
            st_stream(&va[i], y);
            st_stream(&vb[i], x);
        } else {
            T* pa = a + c.head + i * V;
            VT x;
#pragma unroll
            for (int e = 0; e < V; ++e) x.v[e] = pa[e];
#pragma unroll
            for (int e = 0; e < V; ++e) pa[e] = y.v[e];
            st_stream(&vb[i], x);
        }
    }
}

// ---------------------------------------------------- adjacent_difference
// adjacent_difference.hpp:99,194,275: out[0] = in[0], out[i] = op(in[i],
// in[i-1]).  c cuts out + 1 (n - 1 elements).  Both operands of output
// vector i come from ONE aligned vector pair of `in`: with sh the offset of
// in + head inside 16 B, in[k .. k+V] for k = head + i V is elements
// [sh, sh + V] of the pair, so the range is read once from memory and the
// pair's second vector is the next lane's first (a cache hit).  sh is
// wave-uniform: one branch picks the instantiation, no per-element selects.
template <typename T, int V, int SH, typename F>
__device__ __forceinline__ vec<T, V> adjacent_apply(const vec<T, V>& p0, const vec<T, V>& p1, F f) {
    vec<T, V> z;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const T y = (SH + e) < V ? p0.v[(SH + e) % V] : p1.v[(SH + e) % V];              // in[i - 1]
        const T x = (SH + e + 1) < V ? p0.v[(SH + e + 1) % V] : p1.v[(SH + e + 1) % V];  // in[i]
        z.v[e] = static_cast<T>(f(x, y));
    }
    return z;
}

template <typename T, typename F, int V>
__global__ __launch_bounds__(kThreads) void k_adjacent_difference(const T* in, T* out, cut c, int sh, F f) {
    using VT = vec<T, V>;
    const uint64_t tid = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
    T* o = out + 1;  // o[k] = f(in[k + 1], in[k])
    if (tid == 0) out[0] = in[0];
    if (tid < c.head) o[tid] = static_cast<T>(f(in[tid + 1], in[tid]));
    const uint64_t tail0 = c.head + c.nvec * V;
    if (tid < c.tail) o[tail0 + tid] = static_cast<T>(f(in[tail0 + tid + 1], in[tail0 + tid]));
    const VT* vin = reinterpret_cast<const VT*>(in + c.head - sh);
    VT* vout = reinterpret_cast<VT*>(o + c.head);
    for (uint64_t i = tid; i < c.nvec; i += stride) {
        const VT p0 = vin[i], p1 = vin[i + 1];
        VT z;
        if constexpr (V == 4) {
            if (sh == 0) z = adjacent_apply<T, V, 0>(p0, p1, f);
            else if (sh == 1) z = adjacent_apply<T, V, 1>(p0, p1, f);
            else if (sh == 2) z = adjacent_apply<T, V, 2>(p0, p1, f);
            else z = adjacent_apply<T, V, 3>(p0, p1, f);
        } else {
            static_assert(V == 2, "4- and 8-byte elements");
            if (sh == 0) z = adjacent_apply<T, V, 0>(p0, p1, f);
            else z = adjacent_apply<T, V, 1>(p0, p1, f);
        }
        st_stream(&vout[i], z);
    }
}

}}  // namespace hpxhip::permute_detail
