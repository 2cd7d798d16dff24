// Kernel point convolution along an index list (pcc_kpconv_aggregate / _bwd, include/pcc_neighbour.h), gfx950, wave64:
// out[b, t * c + ch, i] = sum_j h(i, j, t) * x[b, ch, idx[b, i, j]] with h the linear influence of kernel point t on
// neighbour j of centre i -- rigid KPConv's aggregation; the convolution proper is one GEMM over out.
//
// The influences are a function of the coordinates alone, about 25 instructions with a square root per (slot, kernel
// point), and with the usual extents most of them are exactly zero.
//   * forward: a workgroup owns a tile of centres of one sample -- kTileSlots slots of the list at the odd row stride k | 1
//     (pcc::padded_at, chan_block.hpp) -- and ALL channels, so an influence is computed once.  Pass 1, a lane per slot: the
//     slot's influences on a block of kKpBlock kernel points go to LDS.  Pass 2, a lane per (kernel point, centre): the
//     row's positive influences are packed to its front in slot order with their slot numbers.  Pass 3, a lane per (kernel
//     point, kChanLane channels, centre): the sum over the packed pairs alone, the feature words gathered from x through L2 -- as
//     many gathers as there are positive pairs.  The lanes of a wave are consecutive centres, so the stores are contiguous
//     along m (whole cache lines for k <= 32).  An accumulator is one register of its lane: there is no array indexed by
//     the kernel point, for any kp.
//   * backward: a block of CB channels of a sample per workgroup with the bins of grad_x in LDS (chan_block.hpp: the plan,
//     bins_clear / bins_store), or global atomics where they do not fit.  A lane per slot walks the kernel points in
//     ascending order; the runs of equal consecutive targets are summed inside the wave, then one atomic per run
//     (pcc::scatter_runs, wave_ops.hpp).
#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "wave_ops.hpp"

#include <cmath>
#include <cstdint>

#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"

namespace {

using pcc::canonical_nan;
using pcc::in_range;
using pcc::kCbDirect;

constexpr int kT = pcc::kWgThreads;
constexpr int kMaxK = 128;    // what the searches return
constexpr int kMaxKp = 32;    // kernel points of a call
constexpr int kKpBlock = 8;   // kernel points whose influences a pass of the forward holds in LDS
constexpr unsigned kMinChunkSlots = 8192;  // slots per workgroup below which the backward's direct path splits a list no further
// the forward: threads of a workgroup, slots of its tile, and the words of a plane of the tile: kTileSlots / k rows at the
// stride k | 1 (the most at k = 2: 512 rows of 3 words; k = 1: 1024 rows of 1)
constexpr int kFwdThreads = 512, kTileSlots = 1024, kTileWords = kTileSlots + kTileSlots / 2;
// its LDS: hs [kKpBlock][kTileWords] float, sidx [kTileWords] int, js [kKpBlock][kTileWords] and cn [kKpBlock][kTileSlots]
// bytes -- 74 KB, two workgroups to a compute unit
constexpr size_t kFwdLds = (size_t)(kKpBlock + 1) * kTileWords * 4 + (size_t)kKpBlock * (kTileWords + kTileSlots);
constexpr unsigned kChanSpan = 2048;  // channels of one sweep of pass 3 (keeps its item count in 32 bits for any c)
constexpr int kChanLane = 4;          // channels of a lane of pass 3: a packed pair is read once for them, their gathers overlap

// The influence of the kernel point q on the neighbour at r (relative to its centre), include/pcc_neighbour.h: every
// operation float32 and rounded (the file is built with -ffp-contract=off), a NaN or infinite distance gives +0.0.
__device__ __forceinline__ float influence(float rx, float ry, float rz, const float *__restrict__ q, float inv) {
    const float ex = rx - q[0], ey = ry - q[1], ez = rz - q[2];
    const float d2 = (ex * ex + ey * ey) + ez * ez;
    const float v = 1.0f - sqrtf(d2) * inv;
    return v > 0.f ? v : 0.f;
}

// Forward.  Unit u: tile u % tiles of sample u / tiles, the centres p0 .. p0 + np - 1.
__global__ __launch_bounds__(kFwdThreads) void kp_fwd_kernel(int c, int n, int m, int k, int kp, float inv, long long units, unsigned tiles,
                                                             const float *__restrict__ xyz, const float *__restrict__ centres,
                                                             const int64_t *__restrict__ idx, const float *__restrict__ x,
                                                             const float *__restrict__ kpts, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *hs = lds;                                                       // [kKpBlock][kTileWords] influences, then packed
    int *sidx = reinterpret_cast<int *>(hs + kKpBlock * kTileWords);       // [kTileWords] the slot's point (0 if it is none)
    unsigned char *js = reinterpret_cast<unsigned char *>(sidx + kTileWords);  // [kKpBlock][kTileWords] slot of a packed pair
    unsigned char *cn = js + kKpBlock * kTileWords;                        // [kKpBlock][kTileSlots] packed pairs of a row
    const unsigned tid = threadIdx.x, um = (unsigned)m, uk = (unsigned)k, ks = uk | 1u, pts = (unsigned)kTileSlots / uk;
    const size_t mk = (size_t)um * uk;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const long long smp = u / tiles;
        const unsigned p0 = (unsigned)(u - smp * tiles) * pts, np = min(pts, um - p0), ns = np * uk;
        const float *xb = x + (size_t)smp * c * n;
        const int64_t *ib = idx + (size_t)smp * mk + (size_t)p0 * uk;
        const float *pb = xyz + (size_t)smp * n * 3, *qb = centres + ((size_t)smp * um + p0) * 3;
        float *ob = out + (size_t)smp * kp * c * um + p0;  // kernel point t, channel ch, centre p0 + row: ob[(t * c + ch) * m + row]
        for (int t0 = 0; t0 < kp; t0 += kKpBlock) {
            const unsigned tb = (unsigned)min(kKpBlock, kp - t0);
            __syncthreads();  // (the previous block's sums are taken)
            for (unsigned sl = tid; sl < ns; sl += kFwdThreads) {
                const long long raw = ib[sl];
                const bool ok = in_range(raw, n);
                const int t = ok ? (int)raw : 0;
                const unsigned row = sl / uk, at = pcc::padded_at(sl, uk, row);
                sidx[at] = t;
                const float *pt = pb + (size_t)t * 3, *ct = qb + (size_t)row * 3;
                const float rx = pt[0] - ct[0], ry = pt[1] - ct[1], rz = pt[2] - ct[2];
                for (unsigned tl = 0; tl < tb; tl++)  // (a slot that is no point costs no root)
                    hs[tl * kTileWords + at] = ok ? influence(rx, ry, rz, kpts + (size_t)(t0 + (int)tl) * 3, inv) : 0.f;
            }
            __syncthreads();
            // pack a row's positive influences to its front, in slot order (in place: a pair moves down or stays)
            for (unsigned it = tid; it < tb * np; it += kFwdThreads) {
                const unsigned tl = it / np, row = it - tl * np;
                float *hr = hs + tl * kTileWords + row * ks;
                unsigned char *jr = js + tl * kTileWords + row * ks;
                unsigned cnt = 0;
                for (unsigned j = 0; j < uk; j++) {
                    const float h = hr[j];
                    if (h > 0.f) {
                        hr[cnt] = h;
                        jr[cnt] = (unsigned char)j;
                        cnt++;
                    }
                }
                cn[tl * kTileSlots + row] = (unsigned char)cnt;
            }
            __syncthreads();
            // acc from +0.0 over the packed pairs: the pairs with h = +0.0 are left out whatever their feature word
            for (unsigned tl = 0; tl < tb; tl++) {
                const float *hp = hs + tl * kTileWords;
                const unsigned char *jp = js + tl * kTileWords, *cp = cn + tl * kTileSlots;
                for (unsigned c0 = 0; c0 < (unsigned)c; c0 += kChanSpan) {
                    const unsigned cw = (min(kChanSpan, (unsigned)c - c0) + kChanLane - 1) / kChanLane;  // groups of kChanLane channels
                    for (unsigned it = tid; it < cw * np; it += kFwdThreads) {
                        const unsigned cg = it / np, row = it - cg * np, base = row * ks, cnt = cp[row];
                        const unsigned ch = c0 + cg * kChanLane, nch = min((unsigned)kChanLane, (unsigned)c - ch);
                        const float *xc = xb + (size_t)ch * n;
                        float acc[kChanLane];
#pragma unroll
                        for (int a = 0; a < kChanLane; a++) acc[a] = 0.f;
                        for (unsigned q = 0; q < cnt; q++) {
                            const float h = hp[base + q];
                            const float *xt = xc + sidx[base + jp[base + q]];
#pragma unroll
                            for (int a = 0; a < kChanLane; a++) {
                                if ((unsigned)a < nch) {
                                    const float p = h * xt[(size_t)a * n];
                                    acc[a] = acc[a] + p;
                                }
                            }
                        }
                        float *op = ob + ((size_t)(t0 + (int)tl) * c + ch) * um + row;
#pragma unroll
                        for (int a = 0; a < kChanLane; a++)
                            if ((unsigned)a < nch) op[(size_t)a * um] = canonical_nan(acc[a]);
                    }
                }
            }
        }
    }
}

// grad_x[smp, c0 + cc, u] += p over the slots with idx == u, p = the sum over the kernel points in ascending order of
// h * grad_out[smp, t * c + c0 + cc, i], the pairs with h = +0.0 left out.  A lane per slot, whole waves (the unit's bounds are
// multiples of 64 slots); the runs of equal consecutive targets among a wave's 64 slots are summed first and the last lane
// of a run adds.  LDS path: the bins of the unit live in LDS (zeroed, ds_add_f32, written out whole: every element of grad_x
// is written); direct path: global atomics into grad_x, zero-filled by the host.
template <int CB, bool DIRECT>
__global__ __launch_bounds__(kT) void kp_bwd_kernel(int c, int n, int m, int k, int kp, float inv, long long units, int nsplit,
                                                    unsigned chunk, const float *__restrict__ xyz,
                                                    const float *__restrict__ centres, const int64_t *__restrict__ idx,
                                                    const float *__restrict__ kpts, const float *__restrict__ go,
                                                    float *__restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) float bins[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    const unsigned um = (unsigned)m, uk = (unsigned)k, mk = um * uk;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, mk, nsplit, chunk);
        if (!DIRECT) pcc::bins_clear(bins, w.cb * n, tid, nt);
        const int64_t *ib = idx + (size_t)w.smp * mk;
        const float *pb = xyz + (size_t)w.smp * n * 3, *qb = centres + (size_t)w.smp * um * 3;
        const float *gb = go + ((size_t)w.smp * kp * c + w.c0) * um;  // kernel point t, channel c0 + cc: gb + (t * c + cc) * m
        float *gx = grad_x + ((size_t)w.smp * c + w.c0) * n;
        for (unsigned base = w.lo + (unsigned)(tid & ~63); base < w.hi; base += (unsigned)nt) {
            const unsigned e = base + (unsigned)lane;
            const long long raw = e < w.hi ? ib[e] : -1;
            const int t = in_range(raw, n) ? (int)raw : -1;  // (slots without a point form runs of -1: summed, never added)
            const unsigned i = t >= 0 ? e / uk : 0;
            float rx = 0.f, ry = 0.f, rz = 0.f;
            if (t >= 0) {
                const float *pt = pb + (size_t)t * 3, *ct = qb + (size_t)i * 3;
                rx = pt[0] - ct[0], ry = pt[1] - ct[1], rz = pt[2] - ct[2];
            }
            float v[CB];
#pragma unroll
            for (int cc = 0; cc < CB; cc++) v[cc] = 0.f;
            for (int kt = 0; kt < kp; kt++) {
                const float h = t >= 0 ? influence(rx, ry, rz, kpts + (size_t)kt * 3, inv) : 0.f;
                if (h > 0.f) {  // (the gradient words of a kernel point are read only where its influence is positive)
                    const float *gt = gb + (size_t)kt * c * um + i;
#pragma unroll
                    for (int cc = 0; cc < CB; cc++) {
                        if (cc < w.cb) {
                            const float p = h * gt[(size_t)cc * um];
                            v[cc] = v[cc] + p;
                        }
                    }
                }
            }
            pcc::scatter_runs(v, w.cb, t, lane, [&](int cc, float sum) {
                if constexpr (DIRECT) {
                    atomicAdd(gx + (size_t)cc * n + t, sum);
                } else {
                    atomicAdd(&bins[cc * n + t], sum);
                }
            });
        }
        if (!DIRECT) pcc::bins_store(gx, bins, w.cb * n, tid, nt);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

// The checks of both entry points, sizes before pointers.
int check_sizes(const char *name, int b, int c, int n, int m, int k, int kp, float sigma) {
    pcc::clear_error();
    if (int rc = pcc::check_list_sizes(name, b, c, n, m, k)) return rc;
    if (kp < 1 || kp > kMaxKp) return pcc::invalidf("%s: kernel points must be 1..%d", name, kMaxKp);
    if (k > kMaxK) return pcc::invalidf("%s: k > %d", name, kMaxK);
    if (!(sigma > 0.f) || !std::isfinite(sigma)) return pcc::invalidf("%s: sigma must be finite and > 0", name);
    return PCC_OK;
}

}  // namespace

extern "C" {

int pcc_kpconv_aggregate(int b, int c, int n, int m, int k, int kp, const float *xyz, const float *centres, const int64_t *idx,
                         const float *x, const float *kernel_points, float sigma, float *out, pcc_stream_t stream) {
    if (int rc = check_sizes("kpconv_aggregate", b, c, n, m, k, kp, sigma)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!xyz || !centres || !idx || !x || !kernel_points || !out) return pcc::invalid("kpconv_aggregate: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float inv = 1.0f / sigma;
    const unsigned tiles = (unsigned)pcc::ceil_div(m, kTileSlots / k);
    const long long units = (long long)b * tiles;
    pcc::ProfScope prof("kp_fwd_kernel", st);
    (void)pcc::allow_lds<kp_fwd_kernel>(kFwdLds);
    hipLaunchKernelGGL(kp_fwd_kernel, dim3(pcc::grid_for(units)), dim3(kFwdThreads), kFwdLds, st, c, n, m, k, kp, inv, units, tiles, xyz,
                       centres, idx, x, kernel_points, out);
    return pcc::check_launch("kpconv_aggregate");
}

int pcc_kpconv_aggregate_bwd(int b, int c, int n, int m, int k, int kp, const float *xyz, const float *centres,
                             const int64_t *idx, const float *kernel_points, float sigma, const float *grad_out, float *grad_x,
                             pcc_stream_t stream) {
    if (int rc = check_sizes("kpconv_aggregate_bwd", b, c, n, m, k, kp, sigma)) return rc;
    if (b == 0) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t gx_bytes = (size_t)b * c * n * sizeof(float);
    const char *cannot_zero = "kpconv_aggregate_bwd: cannot zero grad_x";
    if (m == 0)  // an empty list: nothing points anywhere
        return grad_x ? pcc::zero_async(grad_x, gx_bytes, st, cannot_zero) : pcc::invalid("kpconv_aggregate_bwd: null pointer");
    if (!xyz || !centres || !idx || !kernel_points || !grad_out || !grad_x) return pcc::invalid("kpconv_aggregate_bwd: null pointer");
    const float inv = 1.0f / sigma;
    const unsigned mk = (unsigned)m * (unsigned)k;
    pcc::ListPlan p = pcc::make_list_plan(b, c, n, mk, false, kMinChunkSlots, pcc::tuning(PCC_TUNE_INTERP_PATH));
    p.spread_bins(b, c);
    if (!p.lds)
        if (int rc = pcc::zero_async(grad_x, gx_bytes, st, cannot_zero)) return rc;
    const dim3 block(p.threads(mk, 1));  // a lane per slot
    if (p.lds) {
        // (the profile's name says which channel block ran: the tests read it to know what they covered)
        static const char *const kNames[] = {"kp_bwd_kernel<lds> cb=1", "kp_bwd_kernel<lds> cb=2", "kp_bwd_kernel<lds> cb=4",
                                             "kp_bwd_kernel<lds> cb=8"};
        pcc::ProfScope prof(kNames[p.cb >= 8 ? 3 : p.cb >= 4 ? 2 : p.cb >= 2 ? 1 : 0], st);
        pcc::dispatch_cb(p.cb, [&](auto CB) {
            (void)pcc::allow_lds<kp_bwd_kernel<CB, false>>(pcc::kLdsWg);
            hipLaunchKernelGGL((kp_bwd_kernel<CB, false>), dim3(p.grid()), block, p.lds_bytes, st, c, n, m, k, kp, inv, p.units, p.nsplit,
                               p.chunk, xyz, centres, idx, kernel_points, grad_out, grad_x);
        });
    } else {
        pcc::ProfScope prof("kp_bwd_kernel<direct>", st);
        hipLaunchKernelGGL((kp_bwd_kernel<kCbDirect, true>), dim3(p.grid()), block, 0, st, c, n, m, k, kp, inv, p.units, p.nsplit, p.chunk,
                           xyz, centres, idx, kernel_points, grad_out, grad_x);
    }
    return pcc::check_launch("kpconv_aggregate_bwd");
}

}  // extern "C"
