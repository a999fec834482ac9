/*
 * hpxhip.h -- C ABI of the MI355X (gfx950) backend for HPX's data-parallel
 * algorithm layer.
 *
 * Every entry point is extern "C", takes plain pointers/sizes/enums, and
 * returns an int status: 0 on success, a hipError_t value for a HIP runtime
 * failure, or one of the HPXHIP_ERROR_* codes below.  No function frees
 * caller memory.  All algorithm calls are asynchronous on the given stream
 * (stream order = HPX's sequencing of the algorithm's effects); completion is
 * observed with hpxhip_stream_synchronize / hpxhip_stream_add_callback /
 * events, which the C++ and Python layers turn into hpx::future.
 *
 * What each call replaces in the reference (HPX 1.4.0, /root/reference):
 *   - device/stream/completion  -> hpx/compute/cuda/target.hpp:36-200,
 *       src/compute/cuda/cuda_target.cpp:97-142 (stream callback -> future),
 *       :255-317 (lazy non-blocking stream, synchronize),
 *       src/compute/cuda/get_cuda_targets.cpp:30-65 (enumeration)
 *   - memory                    -> hpx/compute/cuda/allocator.hpp:108-160,
 *       hpx/compute/cuda/transfer.hpp:188-348 (H2D/D2H/D2D copies)
 *   - fill/copy/for_each/transform -> the generic launch_function kernel the
 *       CUDA default_executor instantiates per closure
 *       (hpx/compute/cuda/detail/launch.hpp:32-137,
 *        default_executor.hpp:87-136) for fill.hpp:86, copy.hpp:88-114,
 *        for_each.hpp:369-423, transform.hpp:138-182,411-461,643-694
 *   - reduce/transform_reduce   -> host-only partitioner path
 *       hpx/parallel/algorithms/reduce.hpp:40-89,
 *       transform_reduce.hpp:43-113, transform_reduce_binary.hpp:323,432
 *   - inclusive/exclusive_scan  -> inclusive_scan.hpp:90-173,
 *       exclusive_scan.hpp:100-175 + util/scan_partitioner.hpp:62-156
 *   - copy_if                   -> copy.hpp:401-494
 *   - find / count / min_element / equal / mismatch -> find.hpp:70-382,
 *       count.hpp:259,451, minmax.hpp:46-541, equal.hpp:229, mismatch.hpp:227
 *   - reverse / rotate / swap_ranges / replace / adjacent_difference ->
 *       reverse.hpp:44-191, rotate.hpp:57-268, swap_ranges.hpp:128,
 *       replace.hpp:164-683, adjacent_difference.hpp:99-275
 *   - sort / sort_by_key        -> sort.hpp:182-276, sort_by_key.hpp:42-78
 *   - 1d_stencil heat step      -> examples/1d_stencil/1d_stencil_1.cpp:41-72,
 *       1d_stencil_4_parallel.cpp:87-118
 *
 * The reference has no C ABI (its CUDA calls are inline templates); these
 * entry points are what an FFI or the header-only C++ layer binds.
 */
#ifndef HPXHIP_H
#define HPXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPXHIP_ABI_VERSION 1

/* ---------------------------------------------------------------- status */
enum hpxhip_status {
    HPXHIP_SUCCESS = 0,
    /* 1..999: hipError_t values passed through unchanged */
    HPXHIP_ERROR_INVALID_ARGUMENT = 10001,
    HPXHIP_ERROR_UNSUPPORTED = 10002,     /* dtype/op combination not built */
    HPXHIP_ERROR_DEVICE_TIMEOUT = 10003,  /* a kernel gave up a bounded spin */
    HPXHIP_ERROR_OUT_OF_MEMORY = 10004,
    HPXHIP_ERROR_NOT_READY = 10005
};

/* ----------------------------------------------------------------- types */
enum hpxhip_dtype {
    HPXHIP_I32 = 0,
    HPXHIP_U32 = 1,
    HPXHIP_I64 = 2,
    HPXHIP_U64 = 3,
    HPXHIP_F32 = 4,
    HPXHIP_F64 = 5
};

/* Binary reduction / scan operators (std::plus, std::multiplies, ...). */
enum hpxhip_binop {
    HPXHIP_PLUS = 0,
    HPXHIP_MULTIPLIES = 1,
    HPXHIP_MIN = 2,
    HPXHIP_MAX = 3,
    HPXHIP_BIT_AND = 4,
    HPXHIP_BIT_OR = 5,
    HPXHIP_BIT_XOR = 6
};

/* Unary element functors y = f(x); s0, s1 are scalars of the compute dtype. */
enum hpxhip_unary {
    HPXHIP_U_IDENTITY = 0,   /* x                      (copy)                  */
    HPXHIP_U_SCALE = 1,      /* x * s0                 (stream.cpp:224 multiply_step) */
    HPXHIP_U_ADD_SCALAR = 2, /* x + s0                 (for_each_compute.cu:40 i += 5) */
    HPXHIP_U_AFFINE = 3,     /* x * s0 + s1                                    */
    HPXHIP_U_NEGATE = 4,     /* -x                                             */
    HPXHIP_U_ABS = 5,        /* |x|                                            */
    HPXHIP_U_SQUARE = 6      /* x * x                                          */
};

/* Binary element functors z = f(x, y). */
enum hpxhip_binary {
    HPXHIP_B_ADD = 0,   /* x + y        (stream.cpp:243 add_step)              */
    HPXHIP_B_TRIAD = 1, /* x + y * s0   (stream.cpp:257 triad_step;
                           transform_compute.cu:36 a + 3.0*b)                  */
    HPXHIP_B_SUB = 2,   /* x - y                                               */
    HPXHIP_B_MUL = 3,   /* x * y        (inner product's conv)                 */
    HPXHIP_B_AXPY = 4,  /* x * s0 + y                                          */
    HPXHIP_B_MIN = 5,   /* (y < x) ? y : x                                     */
    HPXHIP_B_MAX = 6    /* (x < y) ? y : x                                     */
};

/* Predicates for copy_if: pred(x) against scalar a of the element dtype. */
enum hpxhip_pred {
    HPXHIP_P_LT = 0,     /* x < a                                              */
    HPXHIP_P_LE = 1,     /* x <= a                                             */
    HPXHIP_P_GT = 2,     /* x > a                                              */
    HPXHIP_P_GE = 3,     /* x >= a                                             */
    HPXHIP_P_EQ = 4,     /* x == a                                             */
    HPXHIP_P_NE = 5,     /* x != a                                             */
    HPXHIP_P_NOT_LT = 6, /* !(x < a)   (copyif_random.cpp:45 `!(i < 0)`)       */
    HPXHIP_P_BITS = 7    /* (x & a) != 0, integers only                        */
};

/* Relations for unique_copy: rel(x, y) on neighbouring elements. */
enum hpxhip_eqrel {
    HPXHIP_Q_EQUAL = 0,     /* x == y (std::equal_to; floats by value)                    */
    HPXHIP_Q_EQUAL_SHR = 1  /* (x >> a) == (y >> a): integers only, 0 <= a < bits of T;   */
};                          /* equal_to under the projection x >> a (same bucket)         */

enum hpxhip_memcpy_kind {
    HPXHIP_H2H = 0,
    HPXHIP_H2D = 1,
    HPXHIP_D2H = 2,
    HPXHIP_D2D = 3,
    HPXHIP_DEFAULT = 4
};

/* Algorithms whose scratch size can be queried. */
enum hpxhip_algo {
    HPXHIP_ALGO_REDUCE = 0,
    HPXHIP_ALGO_SCAN = 1,
    HPXHIP_ALGO_COPY_IF = 2,
    HPXHIP_ALGO_SORT = 3,
    HPXHIP_ALGO_SORT_BY_KEY = 4,
    HPXHIP_ALGO_MERGE = 5,  /* n = n1 + n2 */
    HPXHIP_ALGO_MERGE_RUNS = 6, /* n = the runs' total (hpxhip_merge_runs, up to 8 runs) */
    HPXHIP_ALGO_REDUCE_BY_KEY = 7, /* dtype = the key dtype, aux_dtype = the value dtype */
    HPXHIP_ALGO_PARTITION_COPY = 8,
    HPXHIP_ALGO_STABLE_PARTITION = 9, /* the tile state plus n elements */
    HPXHIP_ALGO_UNIQUE_COPY = 10,
    /* 11 is not assigned */
    HPXHIP_ALGO_COUNT_IF = 12,
    HPXHIP_ALGO_MINMAX_ELEMENT = 13, /* the size for HPXHIP_X_MINMAX, enough for each `which` */
    HPXHIP_ALGO_SET_OPERATION = 14 /* n = n1 + n2 */
};

typedef struct hpxhip_stream_opaque* hpxhip_stream; /* == hipStream_t */
typedef struct hpxhip_event_opaque* hpxhip_event;   /* == hipEvent_t  */
typedef void (*hpxhip_callback)(void* user, int status);

typedef struct hpxhip_device_props {
    char name[256];
    char arch[64];            /* "gfx950:sramecc+:xnack-" */
    int compute_units;        /* 256 on MI355X (cuda_target.cpp:145-184 analogue) */
    int wave_size;            /* 64 */
    int max_threads_per_block;
    int clock_khz;
    int memory_clock_khz;
    int memory_bus_width;
    size_t total_global_mem;
    size_t lds_per_block;
    int pci_bus_id;
    int pci_device_id;
} hpxhip_device_props;

/* ------------------------------------------------------ library / errors */
int hpxhip_abi_version(void);
const char* hpxhip_error_string(int status);
/* Reads and clears the device error word of `device` (kernel-side faults
   that must not hang the GPU, e.g. a look-back spin that gave up). */
int hpxhip_device_error(int device, uint32_t* code);
/* Fault injection for the error-path tests -- the role HPX's throw_always /
   throw_bad_alloc test functors play (tests/unit/parallel/algorithms/
   foreach_tests.hpp:120-205).  hpxhip_debug_inject_error: the next `count`
   algorithm entry points called on this host thread return `status` without
   enqueuing anything (count 0 cancels).  hpxhip_debug_raise_device_error:
   enqueues on `stream` a write of `code` into the device error word, as a
   kernel that gave up a bounded spin does, so the failure surfaces only when
   the queued work completes. */
int hpxhip_debug_inject_error(int status, int count);
int hpxhip_debug_raise_device_error(hpxhip_stream stream, uint32_t code);
/* The next `count` event waits or queries (hpxhip_event_synchronize /
   hpxhip_event_query) on this host thread return `status` -- a completion
   whose event wait fails, as after a kernel fault (count 0 cancels). */
int hpxhip_debug_inject_event_error(int status, int count);

/* ------------------------------------------------ devices (targets) */
int hpxhip_get_device_count(int* count);
int hpxhip_set_device(int device);
int hpxhip_get_device(int* device);
int hpxhip_device_props_get(int device, hpxhip_device_props* props);
int hpxhip_device_synchronize(int device);
int hpxhip_enable_peer_access(int device, int peer);
int hpxhip_can_access_peer(int device, int peer, int* can);

/* ------------------------------------------------ streams & completion */
int hpxhip_stream_create(int device, hpxhip_stream* stream);
int hpxhip_stream_destroy(hpxhip_stream stream);
int hpxhip_stream_synchronize(hpxhip_stream stream);
/* 0 if all work is complete, HPXHIP_ERROR_NOT_READY otherwise. */
int hpxhip_stream_query(hpxhip_stream stream);
/* fn(user, status) runs on a HIP runtime thread once all prior work on the
   stream is done; it must not call HIP (mirrors cuda_target.cpp:97-142). */
int hpxhip_stream_add_callback(hpxhip_stream stream, hpxhip_callback fn, void* user);

int hpxhip_event_create(hpxhip_event* event);
int hpxhip_event_destroy(hpxhip_event event);
/* An event created on `device` (timing 0: hipEventDisableTiming), so it can
   be recorded on that device's streams from any host thread -- the ordering
   event of a cross-device dependency in a multi-GPU process (the reference
   chains such dependencies through futures, segmented_algorithms/
   reduce.hpp:191-207; here hpxhip_stream_wait_event on the event). */
int hpxhip_event_create_on(int device, int timing, hpxhip_event* event);
/* The device a stream belongs to (NULL stream: the current device). */
int hpxhip_stream_device(hpxhip_stream stream, int* device);

int hpxhip_event_record(hpxhip_event event, hpxhip_stream stream);
int hpxhip_event_synchronize(hpxhip_event event);
int hpxhip_event_query(hpxhip_event event);
int hpxhip_event_elapsed_ms(hpxhip_event start, hpxhip_event stop, float* ms);
int hpxhip_stream_wait_event(hpxhip_stream stream, hpxhip_event event);

/* ------------------------------------------------------------- memory */
/* hip::allocator::allocate/deallocate (allocator.hpp:108-160): hipMalloc /
   hipFree; hipErrorOutOfMemory -> HPXHIP_ERROR_OUT_OF_MEMORY. */
int hpxhip_malloc(int device, void** ptr, size_t bytes);
int hpxhip_free(void* ptr);
int hpxhip_malloc_host(void** ptr, size_t bytes); /* pinned */
int hpxhip_free_host(void* ptr);
int hpxhip_mem_info(int device, size_t* free_bytes, size_t* total_bytes);

int hpxhip_memcpy_async(void* dst, const void* src, size_t bytes, int kind, hpxhip_stream stream);
int hpxhip_memcpy_peer_async(void* dst, int dst_device, const void* src, int src_device,
                             size_t bytes, hpxhip_stream stream);
int hpxhip_memset_async(void* dst, int value, size_t bytes, hpxhip_stream stream);
/* Bytes of scratch `algo` needs for n elements of dtype (sort_by_key and
   reduce_by_key: the value dtype is passed in `aux_dtype`, else ignored). */
int hpxhip_scratch_bytes(int algo, int dtype, int aux_dtype, uint64_t n, size_t* bytes);

/* The per-stream scratch cache itself (>= bytes of device memory, reused by
   later calls on the same stream, so valid for stream-ordered work queued
   before the next call that takes scratch on that stream), and the device
   error word the look-back kernels raise a bounded-spin timeout in.  For
   kernels instantiated outside the library -- the C++ layer's device
   closures (hpx/parallel/detail/device_algorithms.hpp), which run the same
   kernel bodies (include/hpxhip/kernels/) with user callables.  No reference
   counterpart: cuda::target's per-target scratch lives in the CUDA runtime. */
int hpxhip_stream_scratch(hpxhip_stream stream, size_t bytes, void** ptr);
int hpxhip_device_error_word(hpxhip_stream stream, uint32_t** word);

/* Scratch convention for every algorithm below: pass (NULL, 0) to let the
   library use a per-stream cached buffer (grown with hipMalloc, so not
   graph-capturable); or pass a caller-owned device buffer of at least
   hpxhip_scratch_bytes() bytes (capturable, no allocation). */

/* ------------------------------------------------ elementwise (for_each) */
/* fill.hpp:86: data[i] = *value (value: host pointer to one dtype element). */
int hpxhip_fill(int dtype, const void* value, void* data, uint64_t n, hpxhip_stream stream);
/* generate.hpp (hpx::parallel::generate / iota-style initialisation of the
   reference tests, e.g. std::iota in transform_reduce.cpp:29):
     GEN_IOTA : data[i] = lo + i
     GEN_BITS : data[i] = bits of splitmix64(seed ^ i) (upper 32 bits for 4-byte types)
     GEN_RANGE: data[i] = lo + splitmix64(seed ^ i) % (hi - lo + 1)   (integers)
     GEN_UNIT : data[i] = (splitmix64(seed ^ i) >> 11) * 2^-53 in [0,1)
                (float: >> 40, * 2^-24)                                  */
enum hpxhip_gen { HPXHIP_GEN_IOTA = 0, HPXHIP_GEN_BITS = 1, HPXHIP_GEN_RANGE = 2, HPXHIP_GEN_UNIT = 3 };
int hpxhip_generate(int dtype, int kind, uint64_t seed, int64_t lo, int64_t hi, void* data, uint64_t n,
                    hpxhip_stream stream);
/* Same with global indices i = index_base + j for data[j] (a partition of a
   partitioned_vector generates exactly its slice of the global sequence). */
int hpxhip_generate_at(int dtype, int kind, uint64_t seed, uint64_t index_base, int64_t lo, int64_t hi,
                       void* data, uint64_t n, hpxhip_stream stream);
/* copy.hpp:88-114: out[i] = in[i]. */
int hpxhip_copy(int dtype, const void* in, void* out, uint64_t n, hpxhip_stream stream);
/* for_each.hpp:369: data[i] = f(data[i]) in place (for_each_compute.cu `i += 5`). */
int hpxhip_for_each(int dtype, int unary_kind, const void* scalars, void* data, uint64_t n,
                    hpxhip_stream stream);
/* transform.hpp:138 (unary): out[i] = (out_t) f((compute_t) in[i]).
   Built combinations: in == out dtype, compute dtype == in dtype or F64. */
int hpxhip_transform(int in_dtype, int compute_dtype, int out_dtype, int unary_kind,
                     const void* scalars, const void* in, void* out, uint64_t n,
                     hpxhip_stream stream);
/* transform.hpp:411/643 (binary): out[i] = (out_t) f((compute_t) in1[i], (compute_t) in2[i]). */
int hpxhip_transform_binary(int in_dtype, int compute_dtype, int out_dtype, int binary_kind,
                            const void* scalars, const void* in1, const void* in2, void* out,
                            uint64_t n, hpxhip_stream stream);
/* for_loop_n with strided pointer inductions (for_loop_induction.hpp:210-219:
 * value at iteration i = base + stride * i):
 *   out[i*out_stride] = (out_t) f((compute_t) in[i*in_stride])              (unary)
 *   out[i*out_stride] = (out_t) f((compute_t) in1[i*s1], (compute_t) in2[i*s2]) (binary)
 * Strides are in elements and may be negative; an input stride may be 0.  An
 * output stride of 0 with n > 1 is HPXHIP_ERROR_INVALID_ARGUMENT (every
 * iteration would write one element), and so is a walk whose span
 * |stride| * (n-1) * size reaches 2^47 bytes.  Like the reference's raw
 * pointer inductions, the ABI does not know the allocations: a walk that
 * leaves its buffer within that span is the caller's error (the Python mirror
 * checks it against the vector; the C++ layer, pointer-based as HPX's
 * iterators are, does not). */
int hpxhip_transform_strided(int in_dtype, int compute_dtype, int out_dtype, int unary_kind,
                             const void* scalars, const void* in, int64_t in_stride, void* out,
                             int64_t out_stride, uint64_t n, hpxhip_stream stream);
int hpxhip_transform_binary_strided(int in_dtype, int compute_dtype, int out_dtype, int binary_kind,
                                    const void* scalars, const void* in1, int64_t in1_stride,
                                    const void* in2, int64_t in2_stride, void* out,
                                    int64_t out_stride, uint64_t n, hpxhip_stream stream);

/* ------------------------------------- rearranging / rewriting a range */
/* reverse.hpp, rotate.hpp, swap_ranges.hpp, replace.hpp and
   adjacent_difference.hpp.  Common to the seven calls below: all six dtypes;
   n == 0 returns 0 and touches nothing; no scratch.  Checked on the host
   before any device call, HPXHIP_ERROR_INVALID_ARGUMENT: an unknown dtype or
   kind, a NULL pointer with n > 0, a pointer that is not aligned to the
   element, mid > n, and ranges that overlap where the call names it (the
   standard's parallel overloads require disjoint ranges).  Pointers need no
   other alignment: ranges at any element offset keep the 16-B kernels. */
/* reverse.hpp:44-79: data[i] <-> data[n-1-i] for i < n/2; the middle element
   of an odd range is not written. */
int hpxhip_reverse(int dtype, void* data, uint64_t n, hpxhip_stream stream);
/* reverse.hpp:155,191: out[i] = in[n-1-i].  in and out must not overlap. */
int hpxhip_reverse_copy(int dtype, const void* in, void* out, uint64_t n, hpxhip_stream stream);
/* rotate.hpp:57-100: left rotation in place, data[mid] becomes data[0]
   (new[i] = old[(i + mid) % n]).  mid == 0 or mid == n launches nothing;
   mid > n is INVALID_ARGUMENT.  Built as the reference's rotate_helper
   (:68-100) from reversals: [0, mid) and [mid, n) reversed in one launch,
   then [0, n) -- two launches, 4 n sizeof(T) bytes. */
int hpxhip_rotate(int dtype, void* data, uint64_t mid, uint64_t n, hpxhip_stream stream);
/* rotate.hpp:219-268: out[i] = in[(i + mid) % n]: the copies in[mid, n) ->
   out[0, n-mid) and in[0, mid) -> out[n-mid, n) in one launch.  mid > n is
   INVALID_ARGUMENT; in and out must not overlap. */
int hpxhip_rotate_copy(int dtype, const void* in, uint64_t mid, uint64_t n, void* out, hpxhip_stream stream);
/* swap_ranges.hpp:128: a[i] <-> b[i].  a and b must not overlap. */
int hpxhip_swap_ranges(int dtype, void* a, void* b, uint64_t n, hpxhip_stream stream);
/* replace.hpp:164 (replace), 326 (replace_if), 493 (replace_copy), 683
   (replace_copy_if): out[i] = pred(in[i]) ? *new_value : in[i], pred an
   hpxhip_pred kind against *pred_arg with copy_if's meaning (pred_arg and
   new_value: host pointers to one dtype element).  replace(old) is
   HPXHIP_P_EQ, compared by value: 0.0 replaces -0.0, a NaN old replaces
   nothing.  *new_value is written bitwise (it may be a NaN).  out may be
   exactly in (the in-place forms); any other overlap is INVALID_ARGUMENT.
   HPXHIP_P_BITS on a float dtype: HPXHIP_ERROR_UNSUPPORTED. */
int hpxhip_replace_if(int dtype, int pred_kind, const void* pred_arg, const void* new_value,
                      const void* in, void* out, uint64_t n, hpxhip_stream stream);
/* adjacent_difference.hpp:99,194,275: out[0] = in[0], out[i] = op(in[i],
   in[i-1]) with op an hpxhip_binary kind (x = in[i], y = in[i-1]; scalars: s0
   of the dtype for TRIAD / AXPY, else may be NULL).  HPXHIP_B_SUB is
   std::adjacent_difference: integers wrap, floats are one IEEE operation
   (bit-exact), so it inverts hpxhip_scan's inclusive PLUS on integers.  in
   and out must not overlap (also not in == out).  One launch; in is read
   once from memory. */
int hpxhip_adjacent_difference(int dtype, int binary_kind, const void* scalars,
                               const void* in, void* out, uint64_t n, hpxhip_stream stream);

/* --------------------------------------------------------- reductions */
/* transform_reduce.hpp:254: *out_dev = init (op) conv(in[0]) (op) ... (op) conv(in[n-1]),
   accumulated in acc_dtype (== in dtype, or I64/F64 widening).  reduce.hpp:200
   is conv_kind = HPXHIP_U_IDENTITY.  out_dev is device memory; init is a
   host pointer to one acc_dtype value.  Integer results are exact; FP results
   use a fixed (run-to-run deterministic) tree, see DESIGN.md for tolerance. */
int hpxhip_transform_reduce(int in_dtype, int acc_dtype, int red_op, int conv_kind,
                            const void* conv_scalars, const void* init, const void* in,
                            uint64_t n, void* out_dev, hpxhip_stream stream, void* scratch,
                            size_t scratch_bytes);
/* transform_reduce_binary.hpp:323: init (op) f(in1[0], in2[0]) (op) ...
   (inner product: red_op = PLUS, binary_kind = B_MUL). */
int hpxhip_transform_reduce_binary(int in_dtype, int acc_dtype, int red_op, int binary_kind,
                                   const void* bin_scalars, const void* init, const void* in1,
                                   const void* in2, uint64_t n, void* out_dev,
                                   hpxhip_stream stream, void* scratch, size_t scratch_bytes);
/* Ordered fold of a short device array: *out_dev = init (op) v[0] (op) ... (op) v[count-1].
   Used for the segment-order combine of segmented reduce/scan carries
   (segmented_algorithms/reduce.hpp:191-207, detail/scan.hpp:667-677). */
int hpxhip_fold(int dtype, int op, const void* init, const void* values_dev, uint64_t count,
                void* out_dev, hpxhip_stream stream);
/* Every prefix of the same fold: out_dev[0] = init, out_dev[j + 1] = out_dev[j] (op) v[j]
   (count + 1 values) -- the carries of a segmented scan in segment order
   (segmented_algorithms/detail/scan.hpp:646-677), folded on the device. */
int hpxhip_fold_exclusive(int dtype, int op, const void* init, const void* values_dev, uint64_t count,
                          void* out_dev, hpxhip_stream stream);

/* -------------------------------------------------------------- scans */
/* inclusive_scan.hpp:288 / exclusive_scan.hpp:292 (+ transform_*_scan with
   conv_kind != IDENTITY).  inclusive: out[i] = P (op) conv(in[0]) ... conv(in[i]);
   exclusive: out[0] = P, out[i] = P (op) conv(in[0]) ... conv(in[i-1]).
   P = *prefix_dev if prefix_dev != NULL (device value; segmented carry),
   else *init (host pointer).  in may alias out (in-place, as
   exclusive_scan_validate.cpp tests).  Single pass, decoupled look-back. */
int hpxhip_scan(int dtype, int op, int inclusive, int conv_kind, const void* conv_scalars,
                const void* init, const void* prefix_dev, const void* in, void* out,
                uint64_t n, hpxhip_stream stream, void* scratch, size_t scratch_bytes);

/* ------------------------------------------------------------ copy_if */
/* copy.hpp:585: stable compaction of in[i] with pred(in[i], *pred_arg) into
   out; *count_dev (uint64, device) receives the number copied, so the
   returned dest iterator is out + count.  out must not overlap in. */
int hpxhip_copy_if(int dtype, int pred_kind, const void* pred_arg, const void* in, void* out,
                   uint64_t n, uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                   size_t scratch_bytes);

/* ---------------------------------------- partition / remove family */
/* partition.hpp:292,1063,1350, remove_copy.hpp:173,350, remove.hpp:290,367:
   one single-pass, stable, two-sided compaction.  The elements that satisfy
   the predicate go to out_true, the others (`!pred(x)`: a NaN under P_LT is
   rejected) to out_false, each side in input order; *count_dev (uint64,
   device) receives the number of accepted elements, the rejected count is
   n - *count_dev.  out_true or out_false may be NULL (that side is dropped;
   a NULL out_true is remove_copy_if), but not both.  Each output may be
   exactly `in` (same pointer: out_false == in is remove_if), but not both;
   the outputs must not overlap each other and partial overlap with `in` is
   not supported.  In place only [0, count) of the aliased output is written:
   the elements from the new end onward keep their values.  n == 0 writes
   *count_dev = 0 and nothing else.  Pointers are aligned to their element
   size.  INVALID_ARGUMENT: a null count, both outputs null,
   out_true == out_false (which covers both equal to `in`). */
int hpxhip_partition_copy(int dtype, int pred_kind, const void* pred_arg, const void* in,
                          void* out_true, void* out_false, uint64_t n, uint64_t* count_dev,
                          hpxhip_stream stream, void* scratch, size_t scratch_bytes);
/* Stable partition of data[0, n) in place: the accepted elements first, then
   the rejected ones, both in input order; *count_dev receives the accepted
   count.  The accepted elements are compacted in place, the rejected ones go
   to scratch, and a second kernel reads the count from device memory and
   copies them to [count, n) (no host round trip).  Scratch
   (HPXHIP_ALGO_STABLE_PARTITION): the tile state plus n elements. */
int hpxhip_stable_partition(int dtype, int pred_kind, const void* pred_arg, void* data, uint64_t n,
                            uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                            size_t scratch_bytes);

/* ------------------------------------------------- unique / unique_copy */
/* unique.hpp:311,612: element i of in[0, n) is kept iff i == 0 or
   !rel(in[i - 1], in[i]); the kept elements go to out in input order (the
   first element of each run survives) and *count_dev (uint64, device)
   receives their number, so unique_copy returns (in + n, out + count) and
   unique returns in + count, also for n <= 1.  One pass over the single-pass
   compaction kernel, no flag array in memory.  Every element is compared with
   its immediate predecessor: that is std::unique_copy and the reference's
   sequential_unique_copy (:333-356) for every equivalence relation and for
   every relation that implies value equality.  For other relations the
   reference compares with the last *kept* element (sequentially; under `par`
   with the element before each chunk, so its result depends on the chunking),
   this call with the predecessor.  HPXHIP_Q_EQUAL compares by value
   (std::equal_to: integers bitwise; floats by value, so -0.0 == +0.0
   collapses and keeps the first, and every NaN is kept).  HPXHIP_Q_EQUAL_SHR:
   rel_arg points to one int32 (host), the shift a; an arithmetic shift for
   signed types.  rel_arg is ignored for HPXHIP_Q_EQUAL.
   out may be exactly `in` (unique; partial overlap is not supported): then
   only [0, count) is written and the elements from the new end onward keep
   their values.  n == 0 writes *count_dev = 0 and nothing else.
   INVALID_ARGUMENT: a null count, null in / out with n > 0, pointers not
   aligned to the element, an unknown rel_kind, a shift outside [0, bits),
   scratch too small.  UNSUPPORTED: EQUAL_SHR on F32 / F64.
   HPXHIP_UNIQUE_STATE64=1 forces the 64-bit look-back value (read per call).
   Scratch: HPXHIP_ALGO_UNIQUE_COPY. */
int hpxhip_unique_copy(int dtype, int rel_kind, const void* rel_arg, const void* in, void* out,
                       uint64_t n, uint64_t* count_dev, hpxhip_stream stream,
                       void* scratch, size_t scratch_bytes);

/* ------------------------------------------------------ search family */
/* Questions asked of a range; every result is one device uint64 (two for
   HPXHIP_X_MINMAX), read back by the caller as copy_if's count is.  Each call
   reads every byte at most once, at the geometry of hpxhip_transform_reduce,
   and writes nothing but its result.  Predicates are the hpxhip_pred kinds
   with copy_if's meaning (a NaN fails P_LT, so negate = 1 finds it).
   INVALID_ARGUMENT: a null result pointer, a null input with n > 0, a pointer
   not aligned to its element (the result: 8 bytes), an unknown pred_kind /
   which, scratch too small.  UNSUPPORTED: P_BITS on F32 / F64. */

/* find.hpp:70,216,382 (find, find_if, find_if_not) and all_any_none.hpp:
   *index_dev = the smallest i in [0, n) with pred(in[i]) != (negate != 0),
   or n if there is none (n == 0 writes 0).  Blocks whose whole chunk lies
   above a hit that is already known skip their loads, so a hit near the
   front does not cost a pass over the range (the reference's
   util::cancellation_token); the result is exact whatever order blocks run
   in.  find(value) is P_EQ, find_if_not is negate = 1, any_of is
   `*index_dev != n`, all_of is `*index_dev == n` with negate = 1. */
int hpxhip_find_if(int dtype, int pred_kind, const void* pred_arg, int negate, const void* in,
                   uint64_t n, uint64_t* index_dev, hpxhip_stream stream);
/* mismatch.hpp:227,396 and equal.hpp:229,398: *index_dev = the smallest i in [0, n)
   with !(in1[i] == in2[i]) by value (-0.0 == +0.0; a NaN differs from
   itself), or n if the ranges are equal (n == 0 writes 0).  The same early
   exit.  in1 and in2 may be misaligned to each other (element loads). */
int hpxhip_mismatch(int dtype, const void* in1, const void* in2, uint64_t n, uint64_t* index_dev,
                    hpxhip_stream stream);
/* count.hpp:259,451: *count_dev = the number of i with pred(in[i]) -- the
   transform_reduce kernel over `pred(x) ? 1 : 0`.  count(value) is P_EQ (a
   NaN is never counted, 0.0 counts -0.0).  Scratch: HPXHIP_ALGO_COUNT_IF. */
int hpxhip_count_if(int dtype, int pred_kind, const void* pred_arg, const void* in, uint64_t n,
                    uint64_t* count_dev, hpxhip_stream stream, void* scratch, size_t scratch_bytes);
/* minmax.hpp:46-66 (min_element: the FIRST smallest), :277 (max_element: the
   FIRST largest), :513-541 (minmax_element: the FIRST smallest and the LAST
   largest, one pass), under std::less, or std::greater if descending != 0
   (then "smallest" is the largest value).  index_dev: one index (two for
   HPXHIP_X_MINMAX: min, then max); n == 0 writes 0 to each.  Floats compare by
   value, -0.0 and +0.0 tie.  With NaNs in the range the comparison is no
   strict weak order and the result is unspecified as in the standard: here it
   is a valid index in [0, n), bitwise reproducible run to run.
   Scratch: HPXHIP_ALGO_MINMAX_ELEMENT. */
enum hpxhip_extreme { HPXHIP_X_MIN = 0, HPXHIP_X_MAX = 1, HPXHIP_X_MINMAX = 2 };
int hpxhip_minmax_element(int dtype, int which, int descending, const void* in, uint64_t n,
                          uint64_t* index_dev /* 1 word; 2 for MINMAX */, hpxhip_stream stream,
                          void* scratch, size_t scratch_bytes);

/* ------------------------------------------------------ reduce_by_key */
/* reduce_by_key.hpp:586: a run is a maximal range of consecutive equal keys
   (std::equal_to: integers bitwise; floats by value, so -0.0 == +0.0 is one
   run and every NaN a run of its own).  Run j gives keys_out[j] = its first
   key and values_out[j] = its values folded left to right with `op`;
   *count_dev (uint64, device) receives the number of runs, so the returned
   iterators are keys_out + count and values_out + count.  One pass: the
   reference's key-state pass (:294-334), tuple scan (:360-390) and zipped
   copy_if (:399-411) fused over a segmented decoupled look-back; FP results
   are bitwise reproducible.  keys_out may be keys_in and values_out may be
   values_in (exactly aliased, as the reference's own test runs it,
   tests/unit/parallel/algorithms/reduce_by_key.cpp:162-168); partial overlap
   is not supported.  BIT_* ops need integer values (else UNSUPPORTED).
   Two deliberate differences from the reference:
   - n <= 1: the reference returns the un-advanced output iterators (and at
     n == 0 dereferences empty ranges, :604-609, FIXME at :302); here
     *count_dev = n, i.e. the ends of what was written (n == 0 writes nothing
     else).
   - only `count` elements of values_out are written; the reference scans
     into values_out over all n positions first, so its callers size it for n. */
int hpxhip_reduce_by_key(int key_dtype, int value_dtype, int op, const void* keys_in,
                         const void* values_in, void* keys_out, void* values_out, uint64_t n,
                         uint64_t* count_dev, hpxhip_stream stream, void* scratch,
                         size_t scratch_bytes);

/* --------------------------------------------------------------- sort */
/* sort.hpp:364: ascending (std::less) or descending (std::greater) sort of
   keys in place; LSD onesweep radix sort.  F32/F64 use the IEEE total order
   (-0.0 before +0.0; NaNs by sign/payload at the ends). */
int hpxhip_sort(int dtype, void* keys, uint64_t n, int descending, hpxhip_stream stream,
                void* scratch, size_t scratch_bytes);
/* sort_by_key.hpp:42: stable sort of keys with values permuted alongside
   (value dtype = any 4/8-byte dtype). */
int hpxhip_sort_by_key(int key_dtype, int value_dtype, void* keys, void* values, uint64_t n,
                       int descending, hpxhip_stream stream, void* scratch, size_t scratch_bytes);

/* -------------------------------------------------------------- merge */
/* merge.hpp:476: stable merge of the sorted ranges in1[0,n1) and in2[0,n2)
   into out[0,n1+n2) (equal keys: in1's first, merge.hpp:52-80), ascending
   (std::less) or descending (std::greater), in the same key order as
   hpxhip_sort.  out must not overlap the inputs. */
int hpxhip_merge(int dtype, const void* in1, uint64_t n1, const void* in2, uint64_t n2, void* out,
                 int descending, hpxhip_stream stream, void* scratch, size_t scratch_bytes);
/* The segmented sort's merge step (no reference counterpart: HPX 1.4 has no
   segmented sort; its local algorithm is sort.hpp:364): the nruns (1..8)
   sorted runs in[run_offsets[j], run_offsets[j+1]) (run_offsets: a HOST
   array of nruns+1 non-decreasing element offsets) merged into
   out[0, run_offsets[nruns] - run_offsets[0]) in one pass, in the key order
   of hpxhip_sort (keys only: equal keys are not told apart).  out must not
   overlap in.  Scratch: HPXHIP_ALGO_MERGE_RUNS with n = the total. */
int hpxhip_merge_runs(int dtype, const void* in, const uint64_t* run_offsets, int nruns, void* out,
                      int descending, hpxhip_stream stream, void* scratch, size_t scratch_bytes);
/* ----------------------------------------------------- set operations */
/* set_union.hpp:47, set_intersection.hpp, set_difference.hpp,
   set_symmetric_difference.hpp (exported by parallel_set_operations.hpp):
   std::set_* on the sorted ranges in1[0,n1) and in2[0,n2), as multisets.
   With cnt1 / cnt2 the elements equivalent to a value in in1 / in2 and k an
   element's index inside its own range's run of that value, kept are
     UNION                 in1: all          in2: k >= cnt1
     INTERSECTION          in1: k < cnt2     in2: none
     DIFFERENCE            in1: k >= cnt2    in2: none
     SYMMETRIC_DIFFERENCE  in1: k >= cnt2    in2: k >= cnt1
   written to out[0, count) in the order of the stable merge (by key, in1
   before in2 on ties, index order inside a range); *count_dev (uint64,
   device) receives count and is always written, also for n1 + n2 == 0.
   out == NULL: count only, nothing else is written -- includes(A, B)
   (includes.hpp:129) is DIFFERENCE with in1 = B, in2 = A and count == 0.
   Key order: hpxhip_sort's and hpxhip_merge's (integers as std::less, floats
   in IEEE total order: -0.0 and +0.0 are different keys, NaNs with the same
   bits the same key), descending as std::greater.  out must hold the result
   (at most n1 + n2 elements) and must not overlap the inputs.  One pass: each
   input is read once, only kept elements are written.  Unsorted input gives
   an unspecified selection inside out[0, n1 + n2) and may raise the device
   error word.  Scratch: HPXHIP_ALGO_SET_OPERATION with n = n1 + n2. */
enum hpxhip_set_op {
    HPXHIP_SET_UNION = 0,
    HPXHIP_SET_INTERSECTION = 1,
    HPXHIP_SET_DIFFERENCE = 2,
    HPXHIP_SET_SYMMETRIC_DIFFERENCE = 3
};
int hpxhip_set_operation(int dtype, int op, const void* in1, uint64_t n1, const void* in2, uint64_t n2,
                         void* out, int descending, uint64_t* count_dev, hpxhip_stream stream,
                         void* scratch, size_t scratch_bytes);

/* Batched binary search in a sorted range (the partition cut of the
   segmented sort; std::lower_bound / std::upper_bound semantics under the
   sort's key order): out_dev[i] = number of sorted[] elements ordered before
   values_dev[i] (upper != 0: before or equal).  All pointers are device
   memory; out_dev holds m uint64 counts. */
int hpxhip_sorted_bounds(int dtype, const void* sorted, uint64_t n, const void* values_dev, uint64_t m,
                         int upper, int descending, uint64_t* out_dev, hpxhip_stream stream);

/* is_sorted.hpp:40-120: *count_dev (uint64, device; overwritten) = the
   number of adjacent pairs with pred(keys[i+1], keys[i]), pred = std::less
   (std::greater if descending) on the values -- so -0.0/+0.0 are equal and
   NaN is never out of order, as in the reference (0 <=> sorted); full-size
   sort verification without a host copy. */
int hpxhip_unsorted_pairs(int dtype, const void* keys, uint64_t n, int descending, uint64_t* count_dev,
                          hpxhip_stream stream);

/* ---------------------------------------------------------- 1d_stencil */
/* One heat step of examples/1d_stencil: next[i] = heat(cur[i-1], cur[i], cur[i+1])
   with heat(l,m,r) = m + (k*dt/(dx*dx)) * (l - 2*m + r)  (1d_stencil_1.cpp:43-46).
   cur[-1] := *left_halo_dev, cur[n] := *right_halo_dev (device pointers;
   for one periodic partition pass cur+n-1 and cur). */
int hpxhip_stencil_heat_step(const double* cur, double* next, uint64_t n,
                             const double* left_halo_dev, const double* right_halo_dev,
                             double k, double dt, double dx, hpxhip_stream stream);
/* Temporal blocking: `steps` heat steps in one pass over HBM (steps = 1 or
   an even number up to HPXHIP_STENCIL_MAX_FUSED), writing next[out_lo,
   out_hi) from cur[0, n).  Points left of cur[0] are left_halo_dev[0..steps)
   (left_halo_dev[steps-1] = cur[-1]), points right of cur[n-1] are
   right_halo_dev[0..steps) (right_halo_dev[0] = cur[n]); device pointers.
   Bit-identical to `steps` calls of hpxhip_stencil_heat_step.  Replaces the
   per-step partition update of 1d_stencil_8.cpp:482-531 (the halo becomes
   `steps` points wide, exchanged once per pass). */
#define HPXHIP_STENCIL_MAX_FUSED 16
int hpxhip_stencil_heat_steps(const double* cur, double* next, uint64_t n, uint64_t out_lo, uint64_t out_hi,
                              const double* left_halo_dev, const double* right_halo_dev, int steps, double k,
                              double dt, double dx, hpxhip_stream stream);
/* nt periodic steps on one partition, ping-ponging u0/u1; the result is in
   u0 if nt is even, else in u1 (1d_stencil_1.cpp:58-70).  Runs fused passes
   of up to HPXHIP_STENCIL_MAX_FUSED steps for rings of >= 1024 points. */
int hpxhip_stencil_heat_run(double* u0, double* u1, uint64_t n, uint64_t nt, double k,
                            double dt, double dx, hpxhip_stream stream);
/* As hpxhip_stencil_heat_run with the fewest passes (nt = 16q + r -> q
   passes of 16, then r's); *result_in_u1 (set on return, host memory) tells which
   buffer holds the result. */
int hpxhip_stencil_heat_run_fused(double* u0, double* u1, uint64_t n, uint64_t nt, double k, double dt,
                                  double dx, int* result_in_u1, hpxhip_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* HPXHIP_H */
