// Grid pooling (pcc_grid_cluster, pcc_segment_pool / _bwd, include/pcc_neighbour.h), gfx950, wave64: the sparse form of
// pcc_voxelize -- one output slot per OCCUPIED cell of pcc_voxel_index's grid, in ascending cell, instead of a dense res^3
// grid.  Integers and gathers only: nothing is atomic, every word is written once.
//   * grid_cluster_kernel: one workgroup per cloud.  The cells of the sorted positions go to LDS (coalesced), every thread
//     owns a contiguous run of up to 16 positions, counts the run starts (a cell that differs from the one before it) and
//     the finite points in it, and a workgroup scan (shuffles inside a wave, the wave totals through LDS) turns the counts
//     into the rank of every position's cell.  A start of rank r < m stores seg[r], a point stores its rank (or -1), and the
//     entries of seg behind the last kept run are filled with its end.
//   * seg_pool_lds_kernel (n <= kLdsMaxN: a row of x fits a workgroup's LDS): a workgroup owns CB channels of one cloud (as
//     many rows as fit half a CU's LDS, chan_block.hpp), streams those rows into LDS with 16-byte loads -- x is read once,
//     coalesced --, then a thread owns a slot: it walks the slot's run of the order (ascending point index: the contract's
//     chain) with kAhead points in flight, gathers from LDS and stores; consecutive lanes store consecutive slots.
//   * seg_pool_kernel (longer rows): vox_fwd_kernel's shape -- the same walk with a thread per slot and kCb channels, the
//     gathers going to global memory, 4 bytes each (what that costs).  In both a run longer than kLongRun is
//     left to
//   * seg_long_kernel: one wave per 64 channels of such a run, a lane per channel, so a cell holding the whole cloud costs n
//     steps of a wave.  The wave at the first multiple of kLongRun inside the run takes it (bisection over seg finds the run).
//   * seg_pool_bwd_lds_kernel (m <= kLdsMaxBwdM) / seg_pool_bwd_kernel: a gather along cluster, a thread per point; the rows
//     of grad_out (and of arg) of CB channels staged in LDS like the forward's, or kCb channels per thread from global memory.
#include <algorithm>
#include <climits>
#include <cstdint>

#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "pcc_neighbour.h"

namespace {

using pcc::canonical_nan;

constexpr int kMaxPoints = 16384;   // pcc_voxel_index's limit: 16 positions per thread of grid_cluster_kernel
constexpr int kScanThreads = 1024;  // threads of grid_cluster_kernel at the most
constexpr int kT = 256;             // threads of the kernels that gather from global memory
constexpr int kCb = 8;              // channels per thread of those, and per workgroup of the LDS kernels at the most
constexpr int kAhead = 4;           // points of a run whose loads are in flight together
constexpr int kLongRun = 64;        // a run with more points than this goes to seg_long_kernel
constexpr int kMaxGridY = 65535;    // blocks of channels per launch; the kernels stride over the blocks beyond
constexpr int kLdsThreads = 1024;   // threads of seg_pool_lds_kernel at the most
constexpr int kLdsMaxN = 40000;     // rows up to here are staged in LDS (one row and its alignment pad fit pcc::kLdsWgDyn)
constexpr int kLdsMaxBwdM = 20000;  // the backward stages rows of grad_out -- and of arg, for max -- up to this many slots
constexpr int kMean = 0, kSum = 1, kMax = 2;
static_assert((size_t)(kLdsMaxBwdM + 8) * 2 * sizeof(float) <= pcc::kLdsWgDyn, "a row of grad_out and one of arg must fit a workgroup's LDS");
static_assert((size_t)(kLdsMaxN + 3) * sizeof(float) <= pcc::kLdsWgDyn, "a row must fit a workgroup's LDS");

// cells[pos] = the cell of sorted position pos (-1 behind the finite points, or for an order that names no point), then
// [n .. n + 16): the wave totals of the scan.  A position packs (finite << 16) | start: both sums stay below 2^15.
__global__ __launch_bounds__(kScanThreads) void grid_cluster_kernel(int n, int m, const int32_t *__restrict__ cell,
                                                                    const int32_t *__restrict__ order, int32_t *__restrict__ cluster,
                                                                    int32_t *__restrict__ seg, int32_t *__restrict__ n_cells) {
    extern __shared__ int cells[];  // [n + 16]
    int *wave_tot = cells + n;
    const size_t smp = blockIdx.x;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
    const int32_t *cb = cell + smp * n, *ob = order + smp * n;
    int32_t *kb = cluster + smp * n, *sb = seg + smp * ((size_t)m + 1);
    for (int s = tid; s < n; s += T) {
        const unsigned p = (unsigned)ob[s];
        cells[s] = p < (unsigned)n ? cb[p] : -1;
    }
    __syncthreads();
    const int per = (n + T - 1) / T;  // every thread owns a contiguous run of positions
    const int beg = min(tid * per, n), end = min(beg + per, n);
    int mine = 0;
    for (int s = beg; s < end; s++) {
        const int v = cells[s];
        if (v >= 0) mine += (1 << 16) + (s == 0 || cells[s - 1] != v ? 1 : 0);
    }
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        incl += lane >= off ? v : 0;
    }
    if (lane == 63) wave_tot[w] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < nw; i++) {
        const int t = wave_tot[i];
        before += i < w ? t : 0;
        total += t;
    }
    const int u = total & 0xffff, f = total >> 16;  // the occupied cells and the finite points of the cloud
    int rank = ((before + incl - mine) & 0xffff) - 1;  // of the last run that starts before `beg`
    for (int s = beg; s < end; s++) {
        const int v = cells[s];
        const unsigned p = (unsigned)ob[s];
        if (v >= 0 && (s == 0 || cells[s - 1] != v)) {
            rank++;
            if (rank <= m) sb[rank] = s;  // (rank m: the end of the last kept run)
        }
        if (p < (unsigned)n) kb[p] = v >= 0 && rank < m ? rank : -1;
    }
    for (int r = u + tid; r <= m; r += T) sb[r] = f;  // the padded slots: empty runs at the end of the finite points
    if (tid == 0) n_cells[smp] = u;
}

// The run of slot r clipped to the cloud: seg is the caller's, and no position outside [0, n) is read.
__device__ __forceinline__ void run_of(const int32_t *__restrict__ sb, int r, int n, int &st, int &len) {
    st = sb[r];
    const int en = sb[r + 1];
    len = (unsigned)st < (unsigned)n && en > st ? min(en, n) - st : 0;
}

// One step of torch.max over a run in ascending point index: the first NaN stays; otherwise a greater value replaces,
// an equal one (-0 == +0) does not.  Selects, not a branch: the lanes of a wave walk runs of different lengths.
__device__ __forceinline__ void max_step(float &best, int &at, float v, int p) {
    const bool take = (at < 0) | ((best == best) & ((v != v) | (v > best)));
    best = take ? v : best;
    at = take ? p : at;
}

template <int MODE>
__global__ __launch_bounds__(kT) void seg_pool_kernel(int c, int n, int m, const float *__restrict__ x, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ seg, float *__restrict__ out, int32_t *__restrict__ arg) {
    const size_t smp = blockIdx.z;
    const int r = blockIdx.x * kT + threadIdx.x;
    if (r >= m) return;
    int st, len;
    run_of(seg + smp * ((size_t)m + 1), r, n, st, len);
    if (len > kLongRun) return;  // seg_long_kernel's words
    const int32_t *ob = order + smp * n + st;
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0);
        const float *xb = x + (smp * c + c0) * n;
        float acc[kCb];
        int at[kCb];
#pragma unroll
        for (int cc = 0; cc < kCb; cc++) acc[cc] = 0.f, at[cc] = -1;
        for (int q = 0; q < len; q += kAhead) {  // kAhead points in flight: their indices, then their kCb words each, then the chain
            unsigned p[kAhead];
            float xv[kAhead][kCb];
#pragma unroll
            for (int u = 0; u < kAhead; u++) p[u] = q + u < len ? (unsigned)ob[q + u] : ~0u;
#pragma unroll
            for (int u = 0; u < kAhead; u++)
#pragma unroll
                for (int cc = 0; cc < kCb; cc++) xv[u][cc] = p[u] < (unsigned)n && cc < cb ? xb[(size_t)cc * n + p[u]] : 0.f;
#pragma unroll
            for (int u = 0; u < kAhead; u++) {
                if (p[u] >= (unsigned)n) continue;
#pragma unroll
                for (int cc = 0; cc < kCb; cc++) {
                    if (MODE == kMax) max_step(acc[cc], at[cc], xv[u][cc], (int)p[u]);
                    else acc[cc] = acc[cc] + xv[u][cc];
                }
            }
        }
        float *orow = out + (smp * c + c0) * m + r;
#pragma unroll
        for (int cc = 0; cc < kCb; cc++) {
            if (cc >= cb) continue;
            if (MODE == kMean) orow[(size_t)cc * m] = len > 0 ? canonical_nan(acc[cc] / (float)len) : 0.f;
            if (MODE == kSum) orow[(size_t)cc * m] = canonical_nan(acc[cc]);
            if (MODE == kMax) {
                orow[(size_t)cc * m] = acc[cc];
                if (arg) arg[(smp * c + c0 + cc) * m + r] = at[cc];
            }
        }
    }
}

// `words` consecutive words of global memory into LDS, 16 bytes per lane: they sit in LDS at the same offset from a 16-byte
// boundary as in global memory (`lds` is 16-byte aligned and has room for words + 3), so that both sides of the copy are
// aligned.  A copy of bits: no arithmetic touches them.  Returns where word 0 went; the caller's barrier follows.
__device__ __forceinline__ const float *stage_rows(float *lds, const float *__restrict__ src, int words, int tid, int T) {
    const int a = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);
    float *rows = lds + a;
    const int head = min(words, (4 - a) & 3), body = (words - head) & ~3;
    if (tid < head) rows[tid] = src[tid];
    for (int i = head + tid * 4; i < head + body; i += T * 4)
        *reinterpret_cast<pcc::v4f *>(rows + i) = __builtin_nontemporal_load(reinterpret_cast<const pcc::v4f *>(src + i));
    if (tid < words - head - body) rows[head + body + tid] = src[head + body + tid];
    return rows;
}

// CB channels of one cloud per workgroup: their rows of x (contiguous in x) in LDS, then a slot per thread.
template <int MODE, int CB>
__global__ __launch_bounds__(kLdsThreads) void seg_pool_lds_kernel(int c, int n, int m, const float *__restrict__ x,
                                                                   const int32_t *__restrict__ order, const int32_t *__restrict__ seg,
                                                                   float *__restrict__ out, int32_t *__restrict__ arg) {
    extern __shared__ __attribute__((aligned(16))) float lds_rows[];  // [3 + CB * n]
    const auto [smp_i, c0] = pcc::chan_block<CB>(c);
    const size_t smp = smp_i;
    const int cb = min(CB, c - c0), tid = threadIdx.x, T = blockDim.x;
    const float *xb = x + (smp * c + c0) * n;
    const float *rows = stage_rows(lds_rows, xb, cb * n, tid, T);
    __syncthreads();
    const int32_t *sb = seg + smp * ((size_t)m + 1);
    for (int r = tid; r < m; r += T) {
        int st, len;
        run_of(sb, r, n, st, len);
        if (len > kLongRun) continue;  // seg_long_kernel's words
        const int32_t *ob = order + smp * n + st;
        float acc[CB];
        int at[CB];
#pragma unroll
        for (int cc = 0; cc < CB; cc++) acc[cc] = 0.f, at[cc] = -1;
        for (int q = 0; q < len; q += kAhead) {
            unsigned p[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; u++) p[u] = q + u < len ? (unsigned)ob[q + u] : ~0u;
#pragma unroll
            for (int u = 0; u < kAhead; u++) {
                if (p[u] >= (unsigned)n) continue;
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    const float v = cc < cb ? rows[cc * n + p[u]] : 0.f;
                    if (MODE == kMax) max_step(acc[cc], at[cc], v, (int)p[u]);
                    else acc[cc] = acc[cc] + v;
                }
            }
        }
        float *orow = out + (smp * c + c0) * m + r;
#pragma unroll
        for (int cc = 0; cc < CB; cc++) {
            if (cc >= cb) continue;
            if (MODE == kMean) orow[(size_t)cc * m] = len > 0 ? canonical_nan(acc[cc] / (float)len) : 0.f;
            if (MODE == kSum) orow[(size_t)cc * m] = canonical_nan(acc[cc]);
            if (MODE == kMax) {
                orow[(size_t)cc * m] = acc[cc];
                if (arg) arg[(smp * c + c0 + cc) * m + r] = at[cc];
            }
        }
    }
}

// The runs with more than kLongRun points: such a run covers a sorted position that is a multiple of kLongRun, and the wave
// at the first of them takes the run, a lane per channel (blockIdx.y: the block of 64 channels).
template <int MODE>
__global__ __launch_bounds__(64) void seg_long_kernel(int c, int n, int m, const float *__restrict__ x, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ seg, float *__restrict__ out, int32_t *__restrict__ arg) {
    const size_t smp = blockIdx.z;
    const int s = blockIdx.x * kLongRun;
    const int32_t *sb = seg + smp * ((size_t)m + 1);
    int lo = 0, hi = m;  // the last r in [0, m) with seg[r] <= s
    if (sb[0] > s) return;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sb[mid] <= s) lo = mid;
        else hi = mid;
    }
    const int r = lo;
    int st, len;
    run_of(sb, r, n, st, len);
    if (len <= kLongRun || s < st || s - st >= kLongRun || s >= st + len) return;  // (short, or not the run's first multiple)
    const int32_t *ob = order + smp * n + st;
    for (int ch = blockIdx.y * 64 + threadIdx.x; ch < c; ch += gridDim.y * 64) {
        const float *xr = x + (smp * c + ch) * n;
        float acc = 0.f;
        int at = -1;
        for (int q = 0; q < len; q += 2 * kAhead) {
            unsigned p[2 * kAhead];
            float xv[2 * kAhead];
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++) p[u] = q + u < len ? (unsigned)ob[q + u] : ~0u;
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++) xv[u] = p[u] < (unsigned)n ? xr[p[u]] : 0.f;
#pragma unroll
            for (int u = 0; u < 2 * kAhead; u++) {
                if (p[u] >= (unsigned)n) continue;
                if (MODE == kMax) max_step(acc, at, xv[u], (int)p[u]);
                else acc = acc + xv[u];
            }
        }
        const size_t o = (smp * c + ch) * m + r;
        if (MODE == kMean) out[o] = canonical_nan(acc / (float)len);
        if (MODE == kSum) out[o] = canonical_nan(acc);
        if (MODE == kMax) {
            out[o] = acc;
            if (arg) arg[o] = at;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kT) void seg_pool_bwd_kernel(int c, int n, int m, const int32_t *__restrict__ cluster,
                                                          const int32_t *__restrict__ seg, const int32_t *__restrict__ arg,
                                                          const float *__restrict__ g, float *__restrict__ grad_x) {
    const size_t smp = blockIdx.z;
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const int r = cluster[smp * n + p];
    const bool ok = (unsigned)r < (unsigned)m;
    float d = 1.f;
    if (MODE == kMean && ok) {
        const int32_t *sb = seg + smp * ((size_t)m + 1);
        d = (float)(sb[r + 1] - sb[r]);
    }
    for (int c0 = blockIdx.y * kCb; c0 < c; c0 += gridDim.y * kCb) {  // (once, unless c > kMaxGridY * kCb)
        const int cb = min(kCb, c - c0);
        const size_t row = (smp * c + c0) * m + (ok ? r : 0);
        float *ob = grad_x + (smp * c + c0) * n + p;
#pragma unroll
        for (int cc = 0; cc < kCb; cc++) {
            if (cc >= cb) continue;
            float v = 0.f;
            if (ok) {
                const float gv = g[row + (size_t)cc * m];
                if (MODE == kMean) v = gv / d;
                if (MODE == kSum) v = gv;
                if (MODE == kMax) v = arg[row + (size_t)cc * m] == p ? gv : 0.f;
            }
            ob[(size_t)cc * n] = v;
        }
    }
}

// m <= kLdsMaxBwdM: CB channels of one cloud per workgroup, their rows of grad_out (and, for max, of arg) in LDS, then a point
// per thread: the gathers along cluster hit LDS, grad_out is read once, coalesced, and consecutive lanes store consecutive
// points.
template <int MODE, int CB>
__global__ __launch_bounds__(kLdsThreads) void seg_pool_bwd_lds_kernel(int c, int n, int m, const int32_t *__restrict__ cluster,
                                                                       const int32_t *__restrict__ seg, const int32_t *__restrict__ arg,
                                                                       const float *__restrict__ g, float *__restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) float lds_rows[];  // [CB * m + 8] (max: twice that, the words of arg behind)
    const auto [smp_i, c0] = pcc::chan_block<CB>(c);
    const size_t smp = smp_i;
    const int cb = min(CB, c - c0), tid = threadIdx.x, T = blockDim.x;
    const float *rows = stage_rows(lds_rows, g + (smp * c + c0) * m, cb * m, tid, T);
    const int32_t *args = nullptr;
    if (MODE == kMax)
        args = reinterpret_cast<const int32_t *>(
            stage_rows(lds_rows + ((cb * m + 8) & ~3), reinterpret_cast<const float *>(arg + (smp * c + c0) * m), cb * m, tid, T));
    __syncthreads();
    const int32_t *sb = seg + smp * ((size_t)m + 1);
    for (int p = tid; p < n; p += T) {
        const int r = cluster[smp * n + p];
        const bool ok = (unsigned)r < (unsigned)m;
        const float d = MODE == kMean && ok ? (float)(sb[r + 1] - sb[r]) : 1.f;
        float *ob = grad_x + (smp * c + c0) * n + p;
#pragma unroll
        for (int cc = 0; cc < CB; cc++) {
            if (cc >= cb) continue;
            float v = 0.f;
            if (ok) {
                const float gv = rows[cc * m + r];
                if (MODE == kMean) v = gv / d;
                if (MODE == kSum) v = gv;
                if (MODE == kMax) v = args[cc * m + r] == p ? gv : 0.f;
            }
            ob[(size_t)cc * n] = v;
        }
    }
}

// gridDim.y of a launch over blocks of `per` channels
unsigned grid_y(int c, int per) { return (unsigned)std::min(pcc::ceil_div(c, per), kMaxGridY); }

// The size checks the three entry points share (c = 1 where there are no channels, mode = 0 where there is none).
int check_args(const char *name, int b, int c, int n, int m, int mode) {
    pcc::clear_error();
    if (b < 0) return pcc::invalidf("%s: b must be >= 0", name);
    if (c < 1) return pcc::invalidf("%s: c must be >= 1", name);
    if (n < 1) return pcc::invalidf("%s: n must be >= 1", name);
    if (m < 1 || m > n) return pcc::invalidf("%s: m must be in [1, n]", name);
    if (mode < kMean || mode > kMax) return pcc::invalidf("%s: mode must be 0 (mean), 1 (sum) or 2 (max)", name);
    if (b > 65535) return pcc::invalidf("%s: batch too large (b > 65535)", name);
    if ((long long)b * ((long long)n + 1) > INT_MAX) return pcc::invalidf("%s: too many points (b * (n + 1) >= 2^31)", name);
    return PCC_OK;
}

template <class F>
void dispatch_mode(int mode, F &&f) {
    if (mode == kMean) f(std::integral_constant<int, kMean>{});
    else if (mode == kSum) f(std::integral_constant<int, kSum>{});
    else f(std::integral_constant<int, kMax>{});
}

}  // namespace

extern "C" {

int pcc_grid_cluster(int b, int n, int m, const int32_t *cell, const int32_t *order, int32_t *cluster, int32_t *seg,
                     int32_t *n_cells, pcc_stream_t stream) {
    if (int rc = check_args("grid_cluster", b, 1, n, m, 0)) return rc;
    if (n > kMaxPoints) return pcc::invalidf("grid_cluster: n must be <= %d", kMaxPoints);
    if (b == 0) return PCC_OK;
    if (!cell || !order || !cluster || !seg || !n_cells) return pcc::invalid("grid_cluster: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t attr = pcc::allow_lds<grid_cluster_kernel>((size_t)(kMaxPoints + 16) * sizeof(int));
    if (attr != hipSuccess) {
        pcc::set_error((int)attr, "grid_cluster: cannot reserve the scan's LDS");
        return (int)attr;
    }
    const int threads = std::min(kScanThreads, pcc::ceil_div(n, 64) * 64);
    pcc::ProfScope prof("grid_cluster_kernel", st);
    hipLaunchKernelGGL(grid_cluster_kernel, dim3((unsigned)b), dim3((unsigned)threads), (size_t)(n + 16) * sizeof(int), st, n, m, cell,
                       order, cluster, seg, n_cells);
    return pcc::check_launch("grid_cluster");
}

int pcc_segment_pool(int b, int c, int n, int m, int mode, const float *x, const int32_t *order, const int32_t *seg, float *out,
                     int32_t *arg, pcc_stream_t stream) {
    if (int rc = check_args("segment_pool", b, c, n, m, mode)) return rc;
    if (b == 0) return PCC_OK;
    if (!x || !order || !seg || !out) return pcc::invalid("segment_pool: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t attr = hipSuccess;
    dispatch_mode(mode, [&](auto MODE) {
        if (n <= kLdsMaxN) {
            const int cb = pcc::fit_cb(kCb, (size_t)n * sizeof(float));  // 8 channels up to n = 2048, 4 to 4096, 2 to 8192, 1 above
            const long long blocks = (long long)b * pcc::ceil_div(c, cb);
            const int threads = std::min(kLdsThreads, pcc::ceil_div(std::max(m, pcc::ceil_div(cb * n, 4)), 64) * 64);
            static const char *const kNames[] = {"seg_pool_lds_kernel<1>", "seg_pool_lds_kernel<2>",
                                                 "seg_pool_lds_kernel<4>", "seg_pool_lds_kernel<8>"};
            pcc::ProfScope prof(kNames[pcc::cb_index(cb)], st);
            pcc::dispatch_cb<kCb>(cb, [&](auto CB) {
                attr = pcc::allow_lds<seg_pool_lds_kernel<MODE, CB>>(pcc::kLdsWgDyn);
                if (attr == hipSuccess)
                    hipLaunchKernelGGL((seg_pool_lds_kernel<MODE, CB>), dim3((unsigned)blocks), dim3((unsigned)threads),
                                       ((size_t)cb * n + 3) * sizeof(float), st, c, n, m, x, order, seg, out, arg);
            });
        } else {
            pcc::ProfScope prof("seg_pool_kernel", st);
            hipLaunchKernelGGL((seg_pool_kernel<MODE>), dim3((unsigned)pcc::ceil_div(m, kT), grid_y(c, kCb), (unsigned)b), dim3(kT), 0, st, c,
                               n, m, x, order, seg, out, arg);
        }
        if (n > kLongRun) {
            pcc::ProfScope prof("seg_long_kernel", st);
            hipLaunchKernelGGL((seg_long_kernel<MODE>), dim3((unsigned)pcc::ceil_div(n, kLongRun), grid_y(c, 64), (unsigned)b), dim3(64), 0,
                               st, c, n, m, x, order, seg, out, arg);
        }
    });
    if (attr != hipSuccess) {
        pcc::set_error((int)attr, "segment_pool: cannot reserve the rows' LDS");
        return (int)attr;
    }
    return pcc::check_launch("segment_pool");
}

int pcc_segment_pool_bwd(int b, int c, int n, int m, int mode, const int32_t *cluster, const int32_t *seg, const int32_t *arg,
                         const float *grad_out, float *grad_x, pcc_stream_t stream) {
    if (int rc = check_args("segment_pool_bwd", b, c, n, m, mode)) return rc;
    if (b == 0) return PCC_OK;
    if (!cluster || !seg || !grad_out || !grad_x || (mode == kMax && !arg)) return pcc::invalid("segment_pool_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t attr = hipSuccess;
    dispatch_mode(mode, [&](auto MODE) {
        if (m <= kLdsMaxBwdM) {
            const int per = MODE == kMax ? 2 : 1;  // rows of m words per channel
            const int cb = pcc::fit_cb(kCb, (size_t)m * per * sizeof(float));
            const int threads = std::min(kLdsThreads, pcc::ceil_div(n, 64) * 64);
            static const char *const kNames[] = {"seg_pool_bwd_lds_kernel<1>", "seg_pool_bwd_lds_kernel<2>",
                                                 "seg_pool_bwd_lds_kernel<4>", "seg_pool_bwd_lds_kernel<8>"};
            pcc::ProfScope prof(kNames[pcc::cb_index(cb)], st);
            pcc::dispatch_cb<kCb>(cb, [&](auto CB) {
                attr = pcc::allow_lds<seg_pool_bwd_lds_kernel<MODE, CB>>(pcc::kLdsWgDyn);
                if (attr == hipSuccess)
                    hipLaunchKernelGGL((seg_pool_bwd_lds_kernel<MODE, CB>), dim3((unsigned)((long long)b * pcc::ceil_div(c, cb))),
                                       dim3((unsigned)threads), ((size_t)cb * m + 8) * per * sizeof(float), st, c, n, m, cluster, seg, arg,
                                       grad_out, grad_x);
            });
            return;
        }
        pcc::ProfScope prof("seg_pool_bwd_kernel", st);
        hipLaunchKernelGGL((seg_pool_bwd_kernel<MODE>), dim3((unsigned)pcc::ceil_div(n, kT), grid_y(c, kCb), (unsigned)b), dim3(kT), 0, st,
                           c, n, m, cluster, seg, arg, grad_out, grad_x);
    });
    if (attr != hipSuccess) {
        pcc::set_error((int)attr, "segment_pool_bwd: cannot reserve the rows' LDS");
        return (int)attr;
    }
    return pcc::check_launch("segment_pool_bwd");
}

}  // extern "C"
