// Tile-shape probe of k_reduce_by_key (reduce_by_key_kernel.hpp): the shipped
// kernel body at other thread counts, rounds (16-B vectors per lane) and
// occupancy bounds, 2^28 uint64 keys / uint64 values with plus, on runs of
// exactly 128 keys and on all keys distinct.  Median [min, max] of 10 launches
// after 3 warm-up ones, the memset of the tile slots included.
// Results: profiles/reduce_by_key_ubench.log, section 3.
// build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude \
//            scripts/ubench/reduce_by_key_shapes.hip -o scripts/ubench/reduce_by_key_shapes
#include <hpxhip/kernels/reduce_by_key_kernel.hpp>
#include <cstdio>
#include <vector>
#include <algorithm>
using namespace hpxhip;
namespace R = hpxhip::reduce_by_key_detail;
struct keq { __device__ bool operator()(uint64_t a, uint64_t b) const { return a == b; } };
__global__ void k_init(uint64_t* k, uint64_t* v, uint64_t n, int mode) {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    k[i] = mode == 0 ? i / 128 : (mode == 1 ? i : 7);
    v[i] = (i * 2654435761u) % 513;
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
template <int TH, int RO, int MW>
int run(const uint64_t* k, const uint64_t* v, uint64_t* ko, uint64_t* vo, uint64_t n, uint64_t* cnt, char* ws, const char* what) {
    using CT = uint32_t;
    const uint64_t ntiles = n / R::tile_elems<uint64_t, uint64_t, RO, TH>() + 1;
    const size_t bytes = ntiles * R::state_t<CT, uint64_t>::bytes_per_tile();
    R::state_t<CT, uint64_t> st{reinterpret_cast<uint64_t*>(ws), nullptr};
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> ms;
    for (int it = 0; it < 13; ++it) {
        CK(hipEventRecord(a));
        CK(hipMemsetAsync(ws, 0, bytes));
        hipLaunchKernelGGL((R::k_reduce_by_key<uint64_t, uint64_t, keq, op_plus, CT, RO, TH, MW>), dim3((unsigned)ntiles), dim3(TH), 0, 0,
                           k, v, ko, vo, n, keq{}, op_plus{}, cnt, st, 1);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
        float t; CK(hipEventElapsedTime(&t, a, b)); if (it >= 3) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    uint64_t c; CK(hipMemcpy(&c, cnt, 8, hipMemcpyDeviceToHost));
    printf("%-10s threads %4d rounds %d minw %d: median %.4f [%.4f, %.4f] ms  count %llu\n", what, TH, RO, MW, ms[ms.size() / 2], ms.front(), ms.back(), (unsigned long long)c);
    return 0;
}
int main() {
    const uint64_t n = 1ull << 28;
    uint64_t *k, *v, *ko, *vo, *cnt; char* ws;
    CK(hipMalloc(&k, n * 8)); CK(hipMalloc(&v, n * 8)); CK(hipMalloc(&ko, n * 8)); CK(hipMalloc(&vo, n * 8)); CK(hipMalloc(&cnt, 64));
    CK(hipMalloc(&ws, 64 << 20));
    for (int mode = 0; mode < 2; ++mode) {
        k_init<<<(unsigned)(n / 256), 256>>>(k, v, n, mode); CK(hipDeviceSynchronize());
        const char* w = mode == 0 ? "runs128" : "distinct";
        if (run<1024, 4, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<1024, 8, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<512, 4, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<512, 8, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;  // shipped
        if (run<512, 8, 3>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<512, 8, 2>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<256, 8, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<256, 8, 2>(k, v, ko, vo, n, cnt, ws, w)) return 1;
        if (run<256, 4, 4>(k, v, ko, vo, n, cnt, ws, w)) return 1;
    }
    return 0;
}
