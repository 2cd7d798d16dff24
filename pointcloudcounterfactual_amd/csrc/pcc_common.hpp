// Shared host/device helpers for libpcc_structural.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "pcc_structural.h"

// The device code assumes gfx950: wave64, the co-resident barrier's `s_waitcnt vmcnt(0)` and its memory model.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libpcc_structural is written for gfx950 (MI355X) only"
#endif

namespace pcc {

constexpr int kWave = 64;  // CDNA wavefront

// Per-thread last-error record behind pcc_last_error() / pcc_last_status().
void set_error(int status, const char *what);
void clear_error();

inline int check_launch(const char *what) {
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "HIP kernel failed : %d (%s) in %s", (int)err, hipGetErrorString(err), what);
        set_error((int)err, buf);
        return (int)err;
    }
    return PCC_OK;
}

inline int invalid(const char *what) {
    set_error(PCC_EINVAL, what);
    return PCC_EINVAL;
}
// ... with a printf-style message (256 bytes at the most), for checks shared under several entry points' names
__attribute__((format(printf, 1, 2))) int invalidf(const char *fmt, ...);

// The size checks of the ops along an index list idx[b,m,k] into n points with c channels (c = 1 where there are none),
// under the entry point's name: "bad size", "batch too large", "list too long (m * k >= 2^31)", in that order ...
int check_list_sizes(const char *name, int b, int c, int n, int m, int k);
// ... and of the channel slice out_c0 .. out_c0 + c - 1 of an output with out_c channels
int check_out_slice(const char *name, int c, int out_c, int out_c0);

// Stream-ordered zero fill.  PCC_OK, or the HIP error with `what` as the error message (the sticky error is cleared).
int zero_async(void *p, size_t bytes, hipStream_t st, const char *what);

// 16 bytes per lane: four floats for __builtin_nontemporal_load / store, two indices of an int64 list
typedef float v4f __attribute__((ext_vector_type(4)));
typedef long long v2l __attribute__((ext_vector_type(2)));

// No coordinate is an infinity or a NaN.
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    const unsigned e = 0x7f800000u;
    return (__float_as_uint(x) & e) != e && (__float_as_uint(y) & e) != e && (__float_as_uint(z) & e) != e;
}

// Squared norm of a difference vector, in the one rounding order shared with the CPU oracle
// (oracle/structural_oracle.c sqsum3 mode 0).  The translation unit is built with
// -ffp-contract=off, so `y * y` stays a rounded multiply and nothing else is fused.
__device__ __forceinline__ float sq3(float x, float y, float z) {
    return __builtin_fmaf(z, z, __builtin_fmaf(x, x, y * y));
}

// An index outside [0, n) is no point (the -1 of PCC_BALL_PAD_NONE, the pad of a short list): what the slot becomes is
// the caller's.
__device__ __forceinline__ bool in_range(long long v, int n) { return (unsigned long long)v < (unsigned long long)n; }

// The sign and payload of a generated NaN are the implementation's; the contracts fix the word.
__device__ __forceinline__ float canonical_nan(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v; }

// Nearest grid index on one axis of the grid of pcc_occupancy_grid and pcc_voxel_index (inv = (res - 1) / extent,
// top = res - 1): two roundings (the files are built with -ffp-contract=off), the clamp taken on the float.
__device__ __forceinline__ int axis_cell(float x, float lo, float inv, float top) {
    const float t = (x - lo) * inv;
    return (int)fminf(fmaxf(floorf(t + 0.5f), 0.f), top);
}

// pcc_knn's c <= 3 distance of the point (x, y, z) to (sx, sy, sz): df = x - s per coordinate, acc = df0 * df0, then
// fmaf(df, df, acc) in coordinate order (include/pcc_neighbour.h: pcc_knn, pcc_fps, pcc_ball_query).
__device__ __forceinline__ float sqdist(float x, float y, float z, float sx, float sy, float sz) {
    const float d0 = x - sx, d1 = y - sy, d2 = z - sz;
    return __builtin_fmaf(d2, d2, __builtin_fmaf(d1, d1, d0 * d0));
}

// A/B switches for measurements inside ONE process (include/pcc_test_hooks.h: pcc_test_set_tuning; inert without
// PCC_TEST_HOOKS=1): the value of switch `key` (0 = the product's behaviour).
int tuning(int key);

// Compute units of the CURRENT device (cached per device: a process may drive several); 0 if the query fails.
int device_cus();
int device_cus_or(int fallback);  // ... `fallback` instead of 0

// Optional hipEvent bracket around one kernel launch (pcc_profile_* in the C ABI).
bool profiling();
struct ProfScope {
    hipEvent_t start = nullptr;
    hipStream_t st;
    const char *name;
    // coarse scopes bracket a whole launch sequence and are recorded only in mode 2 (no per-launch events inside)
    ProfScope(const char *kernel, hipStream_t s, bool coarse = false, bool enabled = true);
    ~ProfScope();
};

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Stream-ordered workspace of the library: one PRIVATE memory pool per device (hipMemPoolCreate), so that nothing is
// configured on the device's default pool, which belongs to the application (PyTorch, RCCL ...).  Freed blocks stay
// cached in the pool up to kPoolKeepBytes between calls; more than that is handed back at the next synchronisation.
constexpr unsigned long long kPoolKeepBytes = 1ull << 30;
hipError_t ws_malloc(void **p, size_t bytes, hipStream_t st);
hipError_t ws_free(void *p, hipStream_t st);

// One block of that workspace, freed on its stream when the scope ends: behind the work enqueued so far.
struct WsBlock {
    void *p = nullptr;
    hipStream_t st;
    explicit WsBlock(hipStream_t s) : st(s) {}
    WsBlock(const WsBlock &) = delete;
    WsBlock &operator=(const WsBlock &) = delete;
    ~WsBlock() { (void)ws_free(p, st); }
    // PCC_OK, or PCC_ENOMEM with `what` as the error message
    int alloc(size_t bytes, const char *what) {
        if (ws_malloc(&p, bytes, st) != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            set_error(PCC_ENOMEM, what);
            return PCC_ENOMEM;
        }
        return PCC_OK;
    }
};

// Lets `Kernel` take up to `bytes` of dynamic LDS: one hipFuncSetAttribute per kernel and process (a kernel is always
// asked for the same size); a failure clears the sticky error and is returned on every call.
template <auto Kernel>
hipError_t allow_lds(size_t bytes) {
    static const hipError_t e = [bytes] {
        const hipError_t r =
            hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (r != hipSuccess) (void)hipGetLastError();
        return r;
    }();
    return e;
}

// The Chamfer half of pcc_chamfer_emd: computed inside the approximate-EMD call, on the clouds that call sorts
// (approxmatch.hip, nn_sorted.hip); the loss reduction rides in that call's finish launch (am_pair.hip).
struct ChamferOut {
    int mean;
    float *loss, *dist1, *dist2;
    int *idx1, *idx2;
};
int match_cost_with_chamfer(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *grad1,
                            float *grad2, hipStream_t st, const ChamferOut &chamfer);

// Logical block id such that the blocks of one XCD (equal blockIdx % 8: the dispatcher deals workgroups round-robin over the
// 8 XCDs) hold a contiguous run of logical ids.  Bijective on [0, nwg); consecutive logical ids -- the workgroups of one
// sample -- then share an L2.  Placement is a speed matter only: nothing may depend on it.
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    if (nwg <= 8) return bid;
    const int q = nwg / 8, r = nwg % 8, x = bid % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// Hilbert sort of one channels-major cloud per sample (cloud_sort.hip's am_sort_kernel) for the k-NN graph
// (knn_lowdim.hip; the other declarations the k-NN files share are in knn.hpp): aos [b][n]
// (x, y, z, original index as bits), box16 [b][ceil(n/kBox)][8] (lo xyz, pad, hi xyz, pad), perm [b][n] sorted -> original.
constexpr int kBox = 16;  // points per bounding-box block (sorted order)
int sort_cloud_cmajor(int b, int c, int n, const float *x, float4 *aos, float *box16, int *perm, hipStream_t st);

// true while `st` is being captured into a graph (a failed query counts as not capturing)
bool capturing(hipStream_t st);

// ---------------------------------------------------------------------------------------------------
// Co-resident launches (auction_cluster_kernel, am_fine_persist_kernel): every workgroup of the grid is on the device at
// once, because the workgroups of a sample meet at barriers in global memory instead of at kernel boundaries.  The
// caller sizes the grid to fit the device; CoresidentGate keeps other co-resident launches off it meanwhile.
// The barrier issues no cache-wide fence (cdna_hip_programming.md Guideline 16).  It is correct under this rule:
//   * every access to state the workgroups of a sample share is agent_ld / agent_st or an agent-scope atomic (served by
//     the L2 every CU sees);
//   * every wave waits for its own vector memory operations (s_waitcnt vmcnt(0)), then the workgroup barrier;
//   * one relaxed agent-scope fetch_add per workgroup arrives; one thread spins with relaxed agent-scope loads, SLEEP
//     s_sleep units between polls, until the count reaches `target` (the counter is never reset: barrier k of a sample of
//     W workgroups waits for k W);
//   * the spin gives up after BOUND polls or when the sample's error word is raised, reporting through coresident_fail;
//   * a second workgroup barrier hands the outcome to every thread.
// ---------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T agent_ld(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T>
__device__ __forceinline__ void agent_st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Raises the sample's error word; its first reporter also sets the sticky host word (if given, and still clear) to `code`.
__device__ __forceinline__ void coresident_fail(unsigned *err, unsigned *host_err, unsigned code) {
    const unsigned was = __hip_atomic_exchange(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned expected = 0;
    if (host_err && !was)
        __hip_atomic_compare_exchange_strong(host_err, &expected, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// false in every thread if the barrier failed; `code()` (the failure code for the host) runs only then
template <int SLEEP, unsigned BOUND, class Code>
__device__ __forceinline__ bool coresident_barrier(unsigned *ctr, unsigned target, unsigned *err, unsigned *host_err, Code code) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's agent-scope stores / atomics have left the CU
    __syncthreads();
    __shared__ int failed;
    if (threadIdx.x == 0) {
        failed = 0;
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        while (agent_ld(ctr) < target) {
            __builtin_amdgcn_s_sleep(SLEEP);
            if (++spins > BOUND || agent_ld(err)) {  // a partner never arrived, or one reported a failure
                coresident_fail(err, host_err, code());
                failed = 1;
                break;
            }
        }
    }
    __syncthreads();
    return failed == 0;
}

// kinds of co-resident launch; each has its own sticky failure word and test hook (include/pcc_test_hooks.h)
enum CoresidentKind { kAuctionCluster = 0, kFineResident = 1, kCoresidentKinds = 2 };

// Per-device gate taken around the co-resident launch(es) of one call on stream `st`.  `ok` is false while `st` is being
// captured into a graph (a replay would escape the order kept here) or if the device state could not be set up: the
// caller then runs its other schedule.  Otherwise the gate holds the lock, makes `st` wait for the last co-resident launch
// of EITHER kind when that went to another stream, and records the device's event on `st` when it ends.  `sticky`: the
// kind's word in mapped host memory, for coresident_fail; `inject`: the test hook asks this launch to fail.
struct CoresidentGate {
    CoresidentGate(CoresidentKind kind, hipStream_t st);
    ~CoresidentGate();
    bool ok = false, inject = false;
    unsigned *sticky = nullptr;
    struct CoresidentDevice *dev = nullptr;
    hipStream_t st;
};

// The failure code an earlier launch of `kind` left on the current device (0: none); clears it.
unsigned take_coresident_failure(CoresidentKind kind);

}  // namespace pcc
