// Farthest point sampling (pcc_fps, include/pcc_neighbour.h), gfx950, wave64.
//
// The algorithm is a chain of m dependent steps: lower every point's running minimum `mind` by its distance to the point
// selected last, then select the point with the largest `mind`.  One workgroup runs the whole chain of one cloud, so a
// step costs one workgroup barrier and no launch:
//   * fps_reg_kernel<BLOCK, P>: thread t keeps points t + p BLOCK, p < P, (x, y, z, mind) in registers for the whole call;
//   * fps_mem_kernel: clouds beyond BLOCK x P = 16384 points; xyz is re-read from global memory every step and mind lives
//     in workspace (each thread only ever touches its own elements, so the workspace needs no ordering of its own).
// Both share the step's selection (block_argmax): per lane the best of its points as a 64-bit key, the wave's maximum by
// DPP (wave_ops.hpp), lane 0 of each wave writes (key, x, y, z of the wave's winner) to the wave's LDS slot, one barrier,
// lane l < waves reads slot l, and a second DPP maximum leaves winner and coordinates in every thread.  The slots are
// double-buffered: a wave that runs ahead writes the other buffer, and comes back to this one only after the next
// barrier, which every wave passes after it has read this one.
//
// Key: (h << 32) | ~j with h = bits(mind) + 1 for a point that takes part (mind >= +0, so its bits order as an unsigned
// integer), h = 0 for an excluded point (a non-finite coordinate), and the whole key 0 for a slot past the end of the
// cloud.  One unsigned maximum is then "largest mind, lowest index; excluded points only when nothing else is left, and
// then index 0".  In registers the three classes are mind >= 0, -1 and -2: a distance is never below either marker, so
// the update `if (d < mind) mind = d` leaves them alone, as it leaves everything alone for a NaN d.
#include "pcc_common.hpp"
#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"
#include "wave_ops.hpp"

namespace {

typedef unsigned long long u64;

constexpr float kExcluded = -1.0f;  // mind of a point with a non-finite coordinate
constexpr float kPad = -2.0f;       // mind of a register slot past the end of the cloud
constexpr int kMemBlock = 1024;     // threads of fps_mem_kernel

struct Winner {
    u64 key;
    float x, y, z;
};

using pcc::finite3;
using pcc::sqdist;  // pcc_knn's c <= 3 distance of x_j to the selected point (include/pcc_neighbour.h)

__device__ __forceinline__ u64 fps_key(float mind, unsigned j) {
    if (mind == kPad) return 0;
    const unsigned h = mind >= 0.f ? __float_as_uint(mind) + 1u : 0u;
    return ((u64)h << 32) | ~j;
}
__device__ __forceinline__ unsigned key_index(u64 key) { return ~(unsigned)key; }
// mind of the point a key was made from; NaN for an excluded point
__device__ __forceinline__ float key_mind(u64 key) {
    const unsigned h = (unsigned)(key >> 32);
    return h ? __uint_as_float(h - 1u) : __builtin_nanf("");
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

struct Slots {
    u64 key[2][16];
    float4 xyz[2][16];
};

// The maximum key of the workgroup and the coordinates of its point, in every thread.  `key` is the lane's best;
// pick(j, x, y, z) gives, for the wave-uniform index j of the wave's winner, the coordinates held by the lane that owns j
// (the other lanes may return anything).  Point j belongs to thread j % BLOCK in both kernels.
template <int BLOCK, class Pick>
__device__ __forceinline__ Winner block_argmax(u64 key, Pick pick, Slots &s, int buf) {
    constexpr int NW = BLOCK / 64;
    const int lane = threadIdx.x & 63;
    Winner w;
    w.key = pcc::wave_max_u64(key);
    float cx, cy, cz;
    pick(key_index(w.key), cx, cy, cz);
    const int owner = key_index(w.key) & 63;  // (63 for the key 0 of a wave of empty slots: any lane will do)
    w.x = readlane_f(cx, owner);
    w.y = readlane_f(cy, owner);
    w.z = readlane_f(cz, owner);
    if constexpr (NW > 1) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (lane == 0) {
            s.key[buf][wave] = w.key;
            s.xyz[buf][wave] = make_float4(w.x, w.y, w.z, 0.f);
        }
        __syncthreads();
        const int l = lane < NW ? lane : 0;
        const u64 k = lane < NW ? s.key[buf][l] : 0;
        const float4 c = s.xyz[buf][l];
        w.key = pcc::readlane_u64(pcc::row_max16_u64(k), 0);
        const int ww = (key_index(w.key) & (BLOCK - 1)) >> 6;
        w.x = readlane_f(c.x, ww);
        w.y = readlane_f(c.y, ww);
        w.z = readlane_f(c.z, ww);
    }
    return w;
}

// a[p] for a wave-uniform p: a scalar branch tree, so that the register array is never indexed through memory
template <int P>
__device__ __forceinline__ void pick3(const float (&x)[P], const float (&y)[P], const float (&z)[P], int p, float &cx, float &cy,
                                      float &cz) {
    cx = x[0], cy = y[0], cz = z[0];
#define PCC_FPS_CASE(K)                             \
    case K:                                         \
        if constexpr (K < P) cx = x[K < P ? K : 0], cy = y[K < P ? K : 0], cz = z[K < P ? K : 0]; \
        break;
    switch (p) {
        PCC_FPS_CASE(1) PCC_FPS_CASE(2) PCC_FPS_CASE(3) PCC_FPS_CASE(4) PCC_FPS_CASE(5) PCC_FPS_CASE(6) PCC_FPS_CASE(7)
        PCC_FPS_CASE(8) PCC_FPS_CASE(9) PCC_FPS_CASE(10) PCC_FPS_CASE(11) PCC_FPS_CASE(12) PCC_FPS_CASE(13) PCC_FPS_CASE(14)
        PCC_FPS_CASE(15)
    default: break;
    }
#undef PCC_FPS_CASE
}

// The start index clamped into the cloud, its coordinates, and the first outputs.
__device__ __forceinline__ Winner first_pick(int n, const float *__restrict__ xb, const int32_t *__restrict__ start,
                                             int64_t *__restrict__ ib, float *__restrict__ db) {
    int s = start ? start[blockIdx.x] : 0;
    s = s < 0 ? 0 : (s > n - 1 ? n - 1 : s);
    Winner w;
    w.key = 0;
    w.x = xb[(size_t)s * 3], w.y = xb[(size_t)s * 3 + 1], w.z = xb[(size_t)s * 3 + 2];
    if (threadIdx.x == 0) {
        ib[0] = s;
        if (db) db[0] = finite3(w.x, w.y, w.z) ? __builtin_inff() : __builtin_nanf("");
    }
    return w;
}

__device__ __forceinline__ void store_pick(const Winner &w, int t, int64_t *__restrict__ ib, float *__restrict__ db) {
    if (threadIdx.x == 0) {
        ib[t] = (int64_t)key_index(w.key);
        if (db) db[t] = key_mind(w.key);
    }
}

template <int BLOCK, int P>
__global__ __launch_bounds__(BLOCK) void fps_reg_kernel(int n, int m, const float *__restrict__ xyz,
                                                        const int32_t *__restrict__ start, int64_t *__restrict__ idx,
                                                        float *__restrict__ dist) {
    static_assert(BLOCK % 64 == 0 && BLOCK <= 1024 && (BLOCK & (BLOCK - 1)) == 0 && P <= 16, "fps: variant out of range");
    __shared__ Slots slots;
    const int tid = threadIdx.x;
    const float *xb = xyz + (size_t)blockIdx.x * n * 3;
    int64_t *ib = idx + (size_t)blockIdx.x * m;
    float *db = dist ? dist + (size_t)blockIdx.x * m : nullptr;

    float x[P], y[P], z[P], mind[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int j = tid + p * BLOCK;
        x[p] = y[p] = z[p] = 0.f;
        mind[p] = kPad;
        if (j < n) {
            x[p] = xb[(size_t)j * 3], y[p] = xb[(size_t)j * 3 + 1], z[p] = xb[(size_t)j * 3 + 2];
            mind[p] = finite3(x[p], y[p], z[p]) ? __builtin_inff() : kExcluded;
        }
    }
    Winner w = first_pick(n, xb, start, ib, db);
    for (int t = 1; t < m; ++t) {
        float best = kPad - 1.f;
        int bp = 0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float d = sqdist(x[p], y[p], z[p], w.x, w.y, w.z);
            if (d < mind[p]) mind[p] = d;
            if (mind[p] > best) best = mind[p], bp = p;  // (p ascending = index ascending: the first maximum stays)
        }
        const u64 key = fps_key(best, (unsigned)(tid + bp * BLOCK));
        w = block_argmax<BLOCK>(
            key, [&](unsigned j, float &cx, float &cy, float &cz) { pick3<P>(x, y, z, (int)(j / BLOCK), cx, cy, cz); }, slots, t & 1);
        store_pick(w, t, ib, db);
    }
}

__global__ __launch_bounds__(kMemBlock) void fps_mem_kernel(int n, int m, const float *__restrict__ xyz,
                                                            const int32_t *__restrict__ start, int64_t *__restrict__ idx,
                                                            float *__restrict__ dist, float *__restrict__ mindw) {
    __shared__ Slots slots;
    const unsigned tid = threadIdx.x, un = (unsigned)n;
    const float *xb = xyz + (size_t)blockIdx.x * n * 3;
    float *mb = mindw + (size_t)blockIdx.x * n;
    int64_t *ib = idx + (size_t)blockIdx.x * m;
    float *db = dist ? dist + (size_t)blockIdx.x * m : nullptr;

    for (unsigned j = tid; j < un; j += kMemBlock)
        mb[j] = finite3(xb[(size_t)j * 3], xb[(size_t)j * 3 + 1], xb[(size_t)j * 3 + 2]) ? __builtin_inff() : kExcluded;
    Winner w = first_pick(n, xb, start, ib, db);
    for (int t = 1; t < m; ++t) {
        float best = kPad, bx = 0.f, by = 0.f, bz = 0.f;
        unsigned bj = tid;
        for (unsigned j = tid; j < un; j += kMemBlock) {
            const float px = xb[(size_t)j * 3], py = xb[(size_t)j * 3 + 1], pz = xb[(size_t)j * 3 + 2];
            float mn = mb[j];
            const float d = sqdist(px, py, pz, w.x, w.y, w.z);
            if (d < mn) mb[j] = mn = d;
            if (mn > best) best = mn, bj = j, bx = px, by = py, bz = pz;
        }
        w = block_argmax<kMemBlock>(
            fps_key(best, bj), [&](unsigned, float &cx, float &cy, float &cz) { cx = bx, cy = by, cz = bz; }, slots, t & 1);
        store_pick(w, t, ib, db);
    }
}

template <int BLOCK, int P>
void launch_reg(const char *name, int b, int n, int m, const float *xyz, const int32_t *start, int64_t *idx, float *dist,
                hipStream_t st) {
    pcc::ProfScope prof(name, st);
    hipLaunchKernelGGL((fps_reg_kernel<BLOCK, P>), dim3(b), dim3(BLOCK), 0, st, n, m, xyz, start, idx, dist);
}

// The variants, smallest first: value v of the fps_path switch forces kPaths[v - 1] (0 capacity = the memory path).  The
// product takes the first one that holds the cloud.
struct Path {
    int capacity;
    void (*launch)(const char *, int, int, int, const float *, const int32_t *, int64_t *, float *, hipStream_t);
    const char *name;  // the launch profile's: the instantiation, <BLOCK,P>
};
const Path kPaths[] = {{64 * 4, launch_reg<64, 4>, "fps_reg_kernel<64,4>"},
                       {256 * 4, launch_reg<256, 4>, "fps_reg_kernel<256,4>"},
                       {256 * 8, launch_reg<256, 8>, "fps_reg_kernel<256,8>"},
                       {512 * 8, launch_reg<512, 8>, "fps_reg_kernel<512,8>"},
                       {1024 * 8, launch_reg<1024, 8>, "fps_reg_kernel<1024,8>"},
                       {1024 * 16, launch_reg<1024, 16>, "fps_reg_kernel<1024,16>"},
                       {0, nullptr, nullptr}};
constexpr int kNumPaths = (int)(sizeof kPaths / sizeof kPaths[0]);

}  // namespace

extern "C" int pcc_fps(int b, int n, int m, const float *xyz, const int32_t *start, int64_t *idx, float *dist,
                       pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 1) return pcc::invalid("fps: bad size");
    if (m < 1 || m > n) return pcc::invalid("fps: m must be in [1, n]");
    if (b > 65535) return pcc::invalid("fps: batch too large");
    if (b == 0) return PCC_OK;
    if (!xyz || !idx) return pcc::invalid("fps: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int forced = pcc::tuning(PCC_TUNE_FPS_PATH);  // measurement switch: 1 .. 7 forces a variant that holds n
    int path = 0;
    while (kPaths[path].capacity && kPaths[path].capacity < n) ++path;
    if (forced >= 1 && forced <= kNumPaths && (!kPaths[forced - 1].capacity || kPaths[forced - 1].capacity >= n)) path = forced - 1;
    if (kPaths[path].capacity) {
        kPaths[path].launch(kPaths[path].name, b, n, m, xyz, start, idx, dist, st);
        return pcc::check_launch("fps");
    }
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc((size_t)b * n * sizeof(float), "fps: workspace allocation failed")) return rc;
    {
        pcc::ProfScope prof("fps_mem_kernel", st);
        hipLaunchKernelGGL(fps_mem_kernel, dim3(b), dim3(kMemBlock), 0, st, n, m, xyz, start, idx, dist, static_cast<float *>(ws.p));
    }
    return pcc::check_launch("fps(memory path)");
}
