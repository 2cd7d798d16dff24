// The point-voxel branch (pcc_voxel_index, pcc_voxelize / _bwd, pcc_devoxelize / _bwd, include/pcc_neighbour.h), gfx950,
// wave64: point features averaged into a dense res^3 grid and read back at the points by trilinear interpolation.  The
// grid is pcc_occupancy_grid's (occupancy.hip: both take their cells from pcc::axis_cell).
//   * vox_index_wave_kernel / vox_index_lds_kernel: one workgroup per cloud sorts the 64-bit keys (cell << 32 | point) --
//     distinct, so every sorting network gives one answer -- in registers (n <= kWaveSort, one wave, wave_sort.hpp) or in
//     LDS (the next power of two of keys, up to kMaxPoints: every wave sorts 64 E keys in registers and only the merge
//     steps between waves go through LDS, padded against bank conflicts).  A non-finite point keys as cell 0x7fffffff:
//     behind every cell, in index order.  The counts go into zeroed rows: integer atomics in the wave kernel (adds
//     commute), the lengths of the sorted runs in the LDS kernel.
//   * vox_start_kernel + vox_fwd_kernel: the first sorted position of every occupied cell goes to a workspace row, then a
//     thread owns P consecutive cells and kCb channels: it walks each cell's run of the order (ascending point index: the
//     contract's chain), divides once and stores -- 16 bytes per lane and channel where the row allows it, the empty cells
//     included, so every word of the grid is written exactly once and nothing is atomic.  A run longer than kLongRun is left
//     to vox_long_kernel: one wave per 64 channels of the run, a lane per channel, so a cell holding the whole cloud costs n
//     steps of a wave instead of n * kCb steps of one lane.
//   * vox_bwd_kernel, devox_fwd_kernel: gathers, a thread per point and kCb channels; the point's cell, or its eight
//     weights and its corner offset, are computed once for the block of channels.
//   * devox_bwd_lds_kernel (res <= 32: a row of res^3 floats fits kLdsRow): a workgroup per cloud and as many channels as
//     fit (8 up to res = 16, 4 to 20, 2 to 25, 1 above) adds into LDS bins and streams the rows out;
//     devox_bwd_global_kernel: global float atomics into a zero-filled grad_grid.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "pcc_neighbour.h"
#include "wave_sort.hpp"

namespace {

typedef unsigned long long u64;
using pcc::canonical_nan;
using pcc::v4f;
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));  // two k-adjacent corners: any 4-byte alignment

constexpr int kWaveSlots = 4;                  // keys per lane of the register sort
constexpr int kWaveSort = 64 * kWaveSlots;     // n up to here: vox_index_wave_kernel
constexpr int kMaxPoints = 16384;              // n up to here: vox_index_lds_kernel (8 bytes of LDS per key, 132 KB at the most)
constexpr int kSortThreads = 1024;             // threads of vox_index_lds_kernel at the most
constexpr int kT = 256;                        // threads of the gather and scatter kernels
constexpr int kCb = 8;                         // channels per thread of those
constexpr int kAhead = 4;                     // points of a run whose loads are in flight together
constexpr int kLongRun = 64;                   // a cell with more points than this goes to vox_long_kernel
constexpr int kMaxGridY = 65535;               // blocks of channels per launch; the kernels stride over the blocks beyond
constexpr int kBinThreads = 1024;              // threads of devox_bwd_lds_kernel
// LDS bins of devox_bwd_lds_kernel.  The cut behind res = 32 is the contract's (include/pcc_neighbour.h, and the tests walk
// it), not the hardware's: rows of res 33 and 34 would still fit pcc::kLdsWg, and must keep taking the global path.
constexpr size_t kLdsRow = 128 * 1024;
constexpr unsigned kNoCell = 0x7fffffffu;      // key of a non-finite point: above every cell (res <= 128: cell < 2^21)

struct Grid {
    int res;
    float lo, inv, top;  // inv = (res - 1) / extent, top = res - 1
};

// nearest grid index on one axis: pcc_occupancy_grid's rule
__device__ __forceinline__ int axis_cell(float x, const Grid &g) { return pcc::axis_cell(x, g.lo, g.inv, g.top); }

// The sort key of point p of the cloud at `xyz`; writes cell[p] and, if COUNT, adds the point to its cell's count.
template <bool COUNT>
__device__ __forceinline__ u64 index_point(const float *__restrict__ xyz, int p, const Grid &g, int32_t *__restrict__ cell,
                                           int32_t *__restrict__ counts) {
    const float x = xyz[(size_t)p * 3], y = xyz[(size_t)p * 3 + 1], z = xyz[(size_t)p * 3 + 2];
    if (!pcc::finite3(x, y, z)) {
        cell[p] = -1;
        return ((u64)kNoCell << 32) | (unsigned)p;
    }
    const int flat = (axis_cell(x, g) * g.res + axis_cell(y, g)) * g.res + axis_cell(z, g);
    cell[p] = flat;
    if (COUNT) atomicAdd(&counts[flat], 1);
    return ((u64)(unsigned)flat << 32) | (unsigned)p;
}

__global__ __launch_bounds__(64) void vox_index_wave_kernel(int n, const float *__restrict__ xyz, Grid g, int32_t *__restrict__ cell,
                                                            int32_t *__restrict__ order, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x, bins = g.res * g.res * g.res;
    const size_t smp = blockIdx.x;
    u64 v[kWaveSlots];
#pragma unroll
    for (int h = 0; h < kWaveSlots; h++) {
        const int e = lane * kWaveSlots + h;
        v[h] = e < n ? index_point<true>(xyz + smp * n * 3, e, g, cell + smp * n, counts + smp * bins) : ~0ull;
    }
    pcc::lane_major_bitonic(v, lane);
#pragma unroll
    for (int h = 0; h < kWaveSlots; h++) {
        const int e = lane * kWaveSlots + h;
        if (e < n) order[smp * n + e] = (int32_t)(unsigned)v[h];
    }
}

// E keys per thread, element i = tid * E + h in v[h]; npad = blockDim.x * E is the power of two >= n.  Every wave sorts its 64 E
// keys in registers (wave_sort.hpp), ascending in the even waves and descending in the odd ones (the complement of a key
// sorts the other way); of the merges behind that only the steps between waves go through LDS.
__host__ __device__ constexpr int padded(int i) { return i + (i >> 5); }

template <int E>
__global__ __launch_bounds__(kSortThreads) void vox_index_lds_kernel(int n, const float *__restrict__ xyz, Grid g, int32_t *__restrict__ cell,
                                                                     int32_t *__restrict__ order, int32_t *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) u64 lds_keys[];  // [padded(npad)]
    // key i sits at i + i / 32.  A lane's E keys are consecutive, so the lanes of a wave read keys E apart: at E = 16 that is
    // 128 bytes, and without the pad all 64 lanes would fall on the same 4 of the 64 four-byte banks
    auto keys = [&](int i) -> u64 & { return lds_keys[padded(i)]; };
    constexpr int kChunk = 64 * E;
    const int tid = threadIdx.x, lane = tid & 63, npad = blockDim.x * E, base = tid * E, bins = g.res * g.res * g.res;
    const size_t smp = blockIdx.x;
    // The points are read with consecutive lanes on consecutive points (coalesced) and their keys parked in LDS; each lane
    // then picks up its own E consecutive keys from there.
    for (int e = tid; e < npad; e += blockDim.x)
        keys(e) = e < n ? index_point<false>(xyz + smp * n * 3, e, g, cell + smp * n, counts) : ~0ull;
    __syncthreads();
    u64 v[E];
#pragma unroll
    for (int h = 0; h < E; h++) v[h] = keys(base + h);
    auto flip = [&](bool descending) {
        const u64 m = descending ? ~0ull : 0ull;
#pragma unroll
        for (int h = 0; h < E; h++) v[h] ^= m;
    };
    flip((base & kChunk) != 0);
    pcc::lane_major_bitonic(v, lane);
    flip((base & kChunk) != 0);
    for (int kk = 2 * kChunk; kk <= npad; kk <<= 1) {
        for (int j = kk >> 1; j >= kChunk; j >>= 1) {
            __syncthreads();  // (the previous step's reads are done)
#pragma unroll
            for (int h = 0; h < E; h++) keys(base + h) = v[h];
            __syncthreads();
#pragma unroll
            for (int h = 0; h < E; h++) {
                const int i = base + h;
                const u64 o = keys(i ^ j);
                const bool take_min = ((i & j) == 0) == ((i & kk) == 0);
                v[h] = take_min == (o < v[h]) ? o : v[h];
            }
        }
        flip((base & kk) != 0);  // (one direction for the whole wave: kk >= 2 * kChunk)
        pcc::lane_major_bitonic_steps(v, lane, 0, kChunk >> 1);
        flip((base & kk) != 0);
    }
    // The counts from run lengths (one store per occupied cell, no atomics): the sorted keys go to LDS once more, and the
    // first key of every cell finds the first key of a later cell by bisection.  The order leaves coalesced from there too.
    __syncthreads();
#pragma unroll
    for (int h = 0; h < E; h++) keys(base + h) = v[h];
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) {
        const u64 key = keys(i);
        order[smp * n + i] = (int32_t)(unsigned)key;
        const unsigned flat = (unsigned)(key >> 32);
        if (flat == kNoCell || (i > 0 && (unsigned)(keys(i - 1) >> 32) == flat)) continue;
        const u64 next = (u64)(flat + 1) << 32;  // (pads and non-finite points key above it)
        int lo = i + 1, hi = npad;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys(mid) < next) lo = mid + 1;
            else hi = mid;
        }
        counts[smp * bins + flat] = lo - i;
    }
}

// The cell of sorted position s of a cloud, -1 behind the finite points (or for an order that names no point).
__device__ __forceinline__ int cell_at(const int32_t *__restrict__ cell, const int32_t *__restrict__ order, int n, int s) {
    const unsigned p = (unsigned)order[s];
    return p < (unsigned)n ? cell[p] : -1;
}

// start[b, cell] = the first sorted position of the cell, for the occupied cells (the others are never read)
__global__ __launch_bounds__(kT) void vox_start_kernel(int n, int bins, const int32_t *__restrict__ cell, const int32_t *__restrict__ order,
                                                       int32_t *__restrict__ start) {
    const size_t smp = blockIdx.y;
    const int s = blockIdx.x * kT + threadIdx.x;
    if (s >= n) return;
    const int v = cell_at(cell + smp * n, order + smp * n, n, s);
    if ((unsigned)v >= (unsigned)bins) return;
    if (s == 0 || cell_at(cell + smp * n, order + smp * n, n, s - 1) != v) start[smp * bins + v] = s;
}

// The run of a cell clipped to the cloud: counts and start are the caller's, and no position past n - 1 is read.
__device__ __forceinline__ int clipped_run(int st, int m, int n) { return (unsigned)st < (unsigned)n ? min(m, n - st) : 0; }

// P consecutive cells and kCb channels per thread.  P = 4: bins % 4 == 0 and counts, start and grid are 16-byte aligned.
template <int P>
__global__ __launch_bounds__(kT) void vox_fwd_kernel(int c, int n, int bins, const float *__restrict__ x, const int32_t *__restrict__ order,
                                                     const int32_t *__restrict__ counts, const int32_t *__restrict__ start,
                                                     float *__restrict__ grid) {
    const size_t smp = blockIdx.z;
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0);
        const long long v0 = ((long long)blockIdx.x * kT + threadIdx.x) * P;
        if (v0 >= bins) return;
        int cnt[P], st[P];
        if constexpr (P == 4) {
            const v4i m4 = *reinterpret_cast<const v4i *>(counts + smp * bins + v0);
            cnt[0] = m4.x, cnt[1] = m4.y, cnt[2] = m4.z, cnt[3] = m4.w;
        } else {
            cnt[0] = counts[smp * bins + v0];
        }
        const float *xb = x + (smp * c + c0) * n;
        const int32_t *ob = order + smp * n;
        float acc[kCb][P];
        bool any_long = false;
#pragma unroll
        for (int q = 0; q < P; q++) {
#pragma unroll
            for (int cc = 0; cc < kCb; cc++) acc[cc][q] = 0.f;
            any_long |= cnt[q] > kLongRun;
            st[q] = cnt[q] > 0 && cnt[q] <= kLongRun ? start[smp * bins + v0 + q] : 0;
        }
#pragma unroll
        for (int q = 0; q < P; q++) {
            if (cnt[q] <= 0 || cnt[q] > kLongRun) continue;
            const int m = clipped_run(st[q], cnt[q], n);
            for (int r = 0; r < m; r += kAhead) {  // kAhead points in flight: their indices, then their kCb words each, then the chain
                unsigned p[kAhead];
                float xv[kAhead][kCb];
#pragma unroll
                for (int u = 0; u < kAhead; u++) p[u] = r + u < m ? (unsigned)ob[st[q] + r + u] : ~0u;
#pragma unroll
                for (int u = 0; u < kAhead; u++)
#pragma unroll
                    for (int cc = 0; cc < kCb; cc++) xv[u][cc] = p[u] < (unsigned)n && cc < cb ? xb[(size_t)cc * n + p[u]] : 0.f;
#pragma unroll
                for (int u = 0; u < kAhead; u++) {
                    if (p[u] >= (unsigned)n) continue;
#pragma unroll
                    for (int cc = 0; cc < kCb; cc++) acc[cc][q] = acc[cc][q] + xv[u][cc];
                }
            }
            const float d = (float)cnt[q];
#pragma unroll
            for (int cc = 0; cc < kCb; cc++) acc[cc][q] = canonical_nan(acc[cc][q] / d);
        }
        float *gb = grid + (smp * c + c0) * bins + v0;
        if (P == 4 && !any_long) {
#pragma unroll
            for (int cc = 0; cc < kCb; cc++) {
                if (cc < cb) {
                    const v4f o = {acc[cc][0], acc[cc][1], acc[cc][2], acc[cc][3]};
                    __builtin_nontemporal_store(o, reinterpret_cast<v4f *>(gb + (size_t)cc * bins));
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < P; q++) {
                if (cnt[q] > kLongRun) continue;  // vox_long_kernel's word
#pragma unroll
                for (int cc = 0; cc < kCb; cc++)
                    if (cc < cb) gb[(size_t)cc * bins + q] = acc[cc][q];
            }
        }
    }
}

// The cells with more than kLongRun points: such a run covers a sorted position that is a multiple of kLongRun, and the
// wave at the first of them takes the cell, a lane per channel (blockIdx.y: the block of 64 channels).
__global__ __launch_bounds__(64) void vox_long_kernel(int c, int n, int bins, const float *__restrict__ x, const int32_t *__restrict__ cell,
                                                      const int32_t *__restrict__ order, const int32_t *__restrict__ counts,
                                                      const int32_t *__restrict__ start, float *__restrict__ grid) {
    const size_t smp = blockIdx.z;
    const int s = blockIdx.x * kLongRun;
    const int v = cell_at(cell + smp * n, order + smp * n, n, s);
    if ((unsigned)v >= (unsigned)bins) return;
    const int cnt = counts[smp * bins + v];
    if (cnt <= kLongRun) return;
    const int st = start[smp * bins + v];
    if ((unsigned)st >= (unsigned)n || s < st || s - st >= kLongRun) return;  // (not the run's first multiple)
    const int32_t *ob = order + smp * n;
    const int m = clipped_run(st, cnt, n);
    for (int ch = blockIdx.y * 64 + threadIdx.x; ch < c; ch += gridDim.y * 64) {
        const float *xr = x + (smp * c + ch) * n;
        float acc = 0.f;
        for (int r = 0; r < m; r += 2 * kAhead) {
            unsigned p[2 * kAhead];
            float xv[2 * kAhead];
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++) p[u] = r + u < m ? (unsigned)ob[st + r + u] : ~0u;
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++) xv[u] = p[u] < (unsigned)n ? xr[p[u]] : 0.f;
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++)
                if (p[u] < (unsigned)n) acc = acc + xv[u];
        }
        grid[(smp * c + ch) * bins + v] = canonical_nan(acc / (float)cnt);
    }
}

__global__ __launch_bounds__(kT) void vox_bwd_kernel(int c, int n, int bins, const int32_t *__restrict__ cell,
                                                     const int32_t *__restrict__ counts, const float *__restrict__ g,
                                                     float *__restrict__ grad_x) {
    const size_t smp = blockIdx.z;
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0);
        const int p = blockIdx.x * kT + threadIdx.x;
        if (p >= n) return;
        const int v = cell[smp * n + p];
        const bool ok = (unsigned)v < (unsigned)bins;
        const float d = ok ? (float)counts[smp * bins + v] : 1.f;
        const float *gb = g + (smp * c + c0) * bins + (ok ? v : 0);
        float *ob = grad_x + (smp * c + c0) * n + p;
#pragma unroll
        for (int cc = 0; cc < kCb; cc++)
            if (cc < cb) ob[(size_t)cc * n] = ok ? gb[(size_t)cc * bins] / d : 0.f;
    }
}

// The eight corners of a point: the offset of corner 000 in a row of the grid and the weights in the order 000, 001, 010,
// ... 111 (di, dj, dk), each (wx * wy) * wz.  false for a non-finite point.
__device__ __forceinline__ void axis_weights(float x, const Grid &g, int &i0, float &w0, float &w1) {
    const float t = fminf(fmaxf((x - g.lo) * g.inv, 0.f), g.top);
    i0 = min((int)floorf(t), g.res - 2);
    w1 = t - (float)i0;  // exact
    w0 = 1.f - w1;
}
__device__ __forceinline__ bool corners_of(const float *__restrict__ xyz, size_t p, const Grid &g, int &off, float (&w)[8]) {
    const float x = xyz[p * 3], y = xyz[p * 3 + 1], z = xyz[p * 3 + 2];
    if (!pcc::finite3(x, y, z)) return false;
    int i, j, k;
    float wx[2], wy[2], wz[2];
    axis_weights(x, g, i, wx[0], wx[1]);
    axis_weights(y, g, j, wy[0], wy[1]);
    axis_weights(z, g, k, wz[0], wz[1]);
    off = (i * g.res + j) * g.res + k;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float wxy = wx[e >> 2] * wy[(e >> 1) & 1];
        w[e] = wxy * wz[e & 1];
    }
    return true;
}

__global__ __launch_bounds__(kT) void devox_fwd_kernel(int c, int n, Grid g, const float *__restrict__ grid, const float *__restrict__ xyz,
                                                       float *__restrict__ out) {
    const size_t smp = blockIdx.z;
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0), res = g.res, bins = res * res * res;
        const int p = blockIdx.x * kT + threadIdx.x;
        if (p >= n) return;
        int off = 0;
        float w[8];
        const bool ok = corners_of(xyz, smp * n + p, g, off, w);
        const float *gb = grid + (smp * c + c0) * bins + off;
        float *ob = out + (smp * c + c0) * n + p;
#pragma unroll
        for (int cc = 0; cc < kCb; cc++) {
            if (cc >= cb) continue;
            float acc = 0.f;
            if (ok) {
                const float *row = gb + (size_t)cc * bins;
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const f2u pair = *reinterpret_cast<const f2u *>(row + ((e >> 2) * res + ((e >> 1) & 1)) * res);
                    const float t0 = w[e] * pair.x, t1 = w[e + 1] * pair.y;
                    acc = acc + t0;
                    acc = acc + t1;
                }
            }
            ob[(size_t)cc * n] = canonical_nan(acc);
        }
    }
}

// CB channels of one cloud per workgroup (as many as fit kLdsRow, chan_block.hpp): bins[CB][res^3] in LDS, zeroed, added to,
// stored whole.  A point's corners are computed once for the CB channels; two points per thread are in flight.
template <int CB>
__global__ __launch_bounds__(kBinThreads) void devox_bwd_lds_kernel(int c, int n, Grid g, const float *__restrict__ xyz,
                                                                    const float *__restrict__ grad_out, float *__restrict__ grad_grid) {
    extern __shared__ __attribute__((aligned(16))) float binsf[];  // [CB][res^3]
    const size_t smp = blockIdx.y;
    const int c0 = blockIdx.x * CB, cb = min(CB, c - c0);
    const int tid = threadIdx.x, res = g.res, bins = res * res * res;
    for (int i = tid; i < cb * bins; i += kBinThreads) binsf[i] = 0.f;
    __syncthreads();
    const float *go = grad_out + (smp * c + c0) * n;
    for (int p0 = tid; p0 < n; p0 += 2 * kBinThreads) {
        int off[2] = {0, 0};
        float w[2][8], gv[2][CB];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int p = p0 + u * kBinThreads;
            ok[u] = p < n && corners_of(xyz, smp * n + (p < n ? p : 0), g, off[u], w[u]);
#pragma unroll
            for (int cc = 0; cc < CB; cc++) gv[u][cc] = ok[u] && cc < cb ? go[(size_t)cc * n + p] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            if (!ok[u]) continue;
#pragma unroll
            for (int cc = 0; cc < CB; cc++) {
                if (cc >= cb) continue;
#pragma unroll
                for (int e = 0; e < 8; e++)
                    atomicAdd(&binsf[cc * bins + off[u] + ((e >> 2) * res + ((e >> 1) & 1)) * res + (e & 1)], w[u][e] * gv[u][cc]);
            }
        }
    }
    __syncthreads();
    float *rows = grad_grid + (smp * c + c0) * bins;  // the cb rows are contiguous
    const int words = cb * bins;
    if ((words & 3) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0) {
        for (int i = tid * 4; i < words; i += kBinThreads * 4)
            __builtin_nontemporal_store(*reinterpret_cast<const v4f *>(binsf + i), reinterpret_cast<v4f *>(rows + i));
    } else {
        for (int i = tid; i < words; i += kBinThreads) rows[i] = binsf[i];
    }
}

// A thread per point and kCb channels: global atomics into grad_grid, zero-filled by the host.
__global__ __launch_bounds__(kT) void devox_bwd_global_kernel(int c, int n, Grid g, const float *__restrict__ xyz,
                                                              const float *__restrict__ grad_out, float *__restrict__ grad_grid) {
    const size_t smp = blockIdx.z;
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0), res = g.res;
        const size_t bins = (size_t)res * res * res;
        const int p = blockIdx.x * kT + threadIdx.x;
        if (p >= n) return;
        int off = 0;
        float w[8];
        if (!corners_of(xyz, smp * n + p, g, off, w)) return;
        const float *go = grad_out + (smp * c + c0) * n + p;
        float *gb = grad_grid + (smp * c + c0) * bins + off;
#pragma unroll
        for (int cc = 0; cc < kCb; cc++) {
            if (cc >= cb) continue;
            const float gv = go[(size_t)cc * n];
#pragma unroll
            for (int e = 0; e < 8; e++) atomicAdd(gb + cc * bins + ((e >> 2) * res + ((e >> 1) & 1)) * res + (e & 1), w[e] * gv);
        }
    }
}

// gridDim.y of a launch over blocks of `per` channels
unsigned grid_y(int c, int per) { return (unsigned)std::min(pcc::ceil_div(c, per), kMaxGridY); }

// The checks every entry point makes on its sizes (c = 1 where there are no channels); `with_scalars`: also lo and extent.
int check_args(const char *name, int b, int c, int n, int res, bool with_scalars, float lo, float extent, Grid &g) {
    pcc::clear_error();
    if (b < 0) return pcc::invalidf("%s: b must be >= 0", name);
    if (c < 1) return pcc::invalidf("%s: c must be >= 1", name);
    if (n < 1) return pcc::invalidf("%s: n must be >= 1", name);
    if (res < 2 || res > 128) return pcc::invalidf("%s: res must be in [2, 128]", name);
    g.res = res, g.lo = lo, g.top = (float)(res - 1);
    g.inv = g.top / extent;
    if (with_scalars) {
        if (!(extent > 0.f) || !std::isfinite(extent) || !std::isfinite(g.inv) || !(g.inv > 0.f))
            return pcc::invalidf("%s: extent must be finite and > 0", name);
        if (!std::isfinite(lo)) return pcc::invalidf("%s: lo must be finite", name);
    }
    if (b > 65535) return pcc::invalidf("%s: batch too large (b > 65535)", name);
    if ((long long)b * n > INT_MAX) return pcc::invalidf("%s: too many points (b * n > INT_MAX)", name);
    if ((long long)b * res * res * res > INT_MAX) return pcc::invalidf("%s: grid too large (b * res^3 > INT_MAX)", name);
    return PCC_OK;
}

}  // namespace

extern "C" {

int pcc_voxel_index(int b, int n, const float *xyz, int res, float lo, float extent, int32_t *cell, int32_t *order,
                    int32_t *counts, pcc_stream_t stream) {
    Grid g;
    if (int rc = check_args("voxel_index", b, 1, n, res, true, lo, extent, g)) return rc;
    if (n > kMaxPoints) return pcc::invalidf("voxel_index: n must be <= %d", kMaxPoints);
    if (b == 0) return PCC_OK;
    if (!xyz || !cell || !order || !counts) return pcc::invalid("voxel_index: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bins = (size_t)res * res * res;
    if (int rc = pcc::zero_async(counts, (size_t)b * bins * sizeof(int32_t), st, "voxel_index: cannot zero counts")) return rc;
    if (n <= kWaveSort) {
        pcc::ProfScope prof("vox_index_wave_kernel", st);
        hipLaunchKernelGGL(vox_index_wave_kernel, dim3((unsigned)b), dim3(64), 0, st, n, xyz, g, cell, order, counts);
    } else {
        int npad = 2 * kWaveSort;
        while (npad < n) npad <<= 1;
        const int slots = npad / kSortThreads < 2 ? 2 : npad / kSortThreads;  // keys per thread: 2 up to 2048 keys, then 4, 8, 16
        hipError_t attr = hipSuccess;
        static const char *const kNames[] = {"vox_index_lds_kernel<2>", "vox_index_lds_kernel<4>",
                                             "vox_index_lds_kernel<8>", "vox_index_lds_kernel<16>"};
        pcc::ProfScope prof(kNames[pcc::cb_index(slots) - 1], st);
        pcc::dispatch_cb<16>(slots, [&](auto E) {
            if constexpr (E >= 2) {
                attr = pcc::allow_lds<vox_index_lds_kernel<E>>((size_t)padded(kMaxPoints) * sizeof(u64));
                if (attr == hipSuccess)
                    hipLaunchKernelGGL((vox_index_lds_kernel<E>), dim3((unsigned)b), dim3((unsigned)(npad / E)), (size_t)padded(npad) * sizeof(u64), st,
                                       n, xyz, g, cell, order, counts);
            }
        });
        if (attr != hipSuccess) {
            pcc::set_error((int)attr, "voxel_index: cannot reserve the sort's LDS");
            return (int)attr;
        }
    }
    return pcc::check_launch("voxel_index");
}

int pcc_voxelize(int b, int c, int n, int res, const float *x, const int32_t *cell, const int32_t *order, const int32_t *counts,
                 float *grid, pcc_stream_t stream) {
    Grid g;
    if (int rc = check_args("voxelize", b, c, n, res, false, 0.f, 1.f, g)) return rc;
    if (b == 0) return PCC_OK;
    if (!x || !cell || !order || !counts || !grid) return pcc::invalid("voxelize: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int bins = res * res * res;
    pcc::WsBlock ws(st);  // start[b, res^3]: the first sorted position of every occupied cell
    if (int rc = ws.alloc((size_t)b * bins * sizeof(int32_t), "voxelize: workspace allocation failed")) return rc;
    int32_t *start = static_cast<int32_t *>(ws.p);
    {
        pcc::ProfScope prof("vox_start_kernel", st);
        hipLaunchKernelGGL(vox_start_kernel, dim3((unsigned)pcc::ceil_div(n, kT), (unsigned)b), dim3(kT), 0, st, n, bins, cell, order, start);
    }
    const unsigned cblocks = grid_y(c, kCb);
    const bool wide = (bins & 3) == 0 && ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(grid)) & 15) == 0;
    {
        pcc::ProfScope prof(wide ? "vox_fwd_kernel<4>" : "vox_fwd_kernel<1>", st);
        if (wide)
            hipLaunchKernelGGL(vox_fwd_kernel<4>, dim3((unsigned)pcc::ceil_div(bins / 4, kT), cblocks, (unsigned)b), dim3(kT), 0, st, c, n,
                               bins, x, order, counts, start, grid);
        else
            hipLaunchKernelGGL(vox_fwd_kernel<1>, dim3((unsigned)pcc::ceil_div(bins, kT), cblocks, (unsigned)b), dim3(kT), 0, st, c, n, bins,
                               x, order, counts, start, grid);
    }
    if (n > kLongRun) {
        pcc::ProfScope prof("vox_long_kernel", st);
        hipLaunchKernelGGL(vox_long_kernel, dim3((unsigned)pcc::ceil_div(n, kLongRun), grid_y(c, 64), (unsigned)b), dim3(64),
                           0, st, c, n, bins, x, cell, order, counts, start, grid);
    }
    return pcc::check_launch("voxelize");
}

int pcc_voxelize_bwd(int b, int c, int n, int res, const int32_t *cell, const int32_t *counts, const float *grad_grid,
                     float *grad_x, pcc_stream_t stream) {
    Grid g;
    if (int rc = check_args("voxelize_bwd", b, c, n, res, false, 0.f, 1.f, g)) return rc;
    if (b == 0) return PCC_OK;
    if (!cell || !counts || !grad_grid || !grad_x) return pcc::invalid("voxelize_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    pcc::ProfScope prof("vox_bwd_kernel", st);
    hipLaunchKernelGGL(vox_bwd_kernel, dim3((unsigned)pcc::ceil_div(n, kT), grid_y(c, kCb), (unsigned)b), dim3(kT), 0, st, c,
                       n, res * res * res, cell, counts, grad_grid, grad_x);
    return pcc::check_launch("voxelize_bwd");
}

int pcc_devoxelize(int b, int c, int n, int res, float lo, float extent, const float *grid, const float *xyz, float *out,
                   pcc_stream_t stream) {
    Grid g;
    if (int rc = check_args("devoxelize", b, c, n, res, true, lo, extent, g)) return rc;
    if (b == 0) return PCC_OK;
    if (!grid || !xyz || !out) return pcc::invalid("devoxelize: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    pcc::ProfScope prof("devox_fwd_kernel", st);
    hipLaunchKernelGGL(devox_fwd_kernel, dim3((unsigned)pcc::ceil_div(n, kT), grid_y(c, kCb), (unsigned)b), dim3(kT), 0, st,
                       c, n, g, grid, xyz, out);
    return pcc::check_launch("devoxelize");
}

int pcc_devoxelize_bwd(int b, int c, int n, int res, float lo, float extent, const float *xyz, const float *grad_out,
                       float *grad_grid, pcc_stream_t stream) {
    Grid g;
    if (int rc = check_args("devoxelize_bwd", b, c, n, res, true, lo, extent, g)) return rc;
    if (b == 0) return PCC_OK;
    if (!xyz || !grad_out || !grad_grid) return pcc::invalid("devoxelize_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t row = (size_t)res * res * res * sizeof(float);
    if (row <= kLdsRow) {
        const int cb = pcc::fit_cb(kCb, row, kLdsRow);  // 8 channels up to res = 16, 4 to 20, 2 to 25, 1 to 32
        hipError_t attr = hipSuccess;
        static const char *const kNames[] = {"devox_bwd_lds_kernel<1>", "devox_bwd_lds_kernel<2>",
                                             "devox_bwd_lds_kernel<4>", "devox_bwd_lds_kernel<8>"};
        pcc::ProfScope prof(kNames[pcc::cb_index(cb)], st);
        pcc::dispatch_cb<kCb>(cb, [&](auto CB) {
            attr = pcc::allow_lds<devox_bwd_lds_kernel<CB>>(kLdsRow);
            if (attr == hipSuccess)
                hipLaunchKernelGGL((devox_bwd_lds_kernel<CB>), dim3((unsigned)pcc::ceil_div(c, CB), (unsigned)b), dim3(kBinThreads),
                                   (size_t)cb * row, st, c, n, g, xyz, grad_out, grad_grid);
        });
        if (attr != hipSuccess) {
            pcc::set_error((int)attr, "devoxelize_bwd: cannot reserve the bins' LDS");
            return (int)attr;
        }
    } else {
        if (int rc = pcc::zero_async(grad_grid, (size_t)b * c * row, st, "devoxelize_bwd: cannot zero grad_grid")) return rc;
        pcc::ProfScope prof("devox_bwd_global_kernel", st);
        hipLaunchKernelGGL(devox_bwd_global_kernel, dim3((unsigned)pcc::ceil_div(n, kT), grid_y(c, kCb), (unsigned)b),
                           dim3(kT), 0, st, c, n, g, xyz, grad_out, grad_grid);
    }
    return pcc::check_launch("devoxelize_bwd");
}

}  // extern "C"
