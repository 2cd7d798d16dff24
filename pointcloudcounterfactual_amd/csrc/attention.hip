// Vector attention along an index list (pcc_neighbour_softmax / _bwd, pcc_aggregate_points / _bwd, include/pcc_neighbour.h),
// gfx950, wave64: a softmax over the k slots of every row of logits[b,g,m,k] that leaves out the slots the list has padded,
// and out[b,ch,i] = sum_j w[b,ch/S,i,j] * (x[b,ch,idx[b,i,j]] + rel[b,ch,i,j]) with S = c / g channels sharing a weight --
// Point Transformer's aggregation, the values gathered inside the kernel.
//
// The [b,c,m,k] streams (rel in, grad_rel out) are the dominant traffic, so in every kernel that touches them consecutive
// lanes take consecutive SLOTS of the list: whole cache lines per wave instruction.  What has to walk the k slots of a row
// in order (the forward's sum, the softmax's sum and d) does so out of LDS, where a tile of rows lies at the odd row stride
// k | 1: the lanes of a wave, each on its own row, hit distinct banks (pcc::padded_at, chan_block.hpp).
//   * aggregation forward and grad_x: a workgroup owns CB channels of one sample (chan_block.hpp) with their rows of x or
//     their gradient bins in LDS, or the direct path (global gathers, global float atomics) where they do not fit; a slot's
//     index is loaded once for the CB channels, a weight word once per group among them;
//   * grad_x sums the runs of equal consecutive indices inside a wave before one atomic per run (pcc::wave_runs): the lanes
//     of a wave are consecutive slots of a row here, and a ball_query(pad='first') row repeats one index;
//   * grad_rel rides in the grad_x kernel (the same products) unless that launch is too narrow to stream it;
//   * grad_w: a thread per (group, slot) walking the group's channels in ascending order, no atomics.
#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "wave_ops.hpp"

#include <cstdint>

#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"

namespace {

using pcc::canonical_nan;
using pcc::in_range;
using pcc::kCbDirect;

constexpr int kT = pcc::kWgThreads;
constexpr int kMaxK = 128;               // what the searches return
// dense points (forward), resp. slots (backward), per workgroup below which the list of a sample is not split further
constexpr unsigned kMinChunkPts = 1024, kMinChunkSlots = 8192;
// slots of one pass of the forward, and the words of its tile per channel: kTileSlots / k rows at the stride k | 1
// (the most at k = 2: 512 rows of 3 words)
constexpr int kTileSlots = 1024, kTileWords = kTileSlots + kTileSlots / 2;
// the same for a workgroup of the softmax kernels
constexpr int kSmThreads = 256, kSmSlots = 2048, kSmWords = kSmSlots + kSmSlots / 2;

// ---- aggregation ----------------------------------------------------------------------------------------------------------

// Forward.  Pass 1, a lane per slot: prod[cc][row * (k | 1) + j] = w * (x + rel) for the CB channels, +0.0 for a slot that
// is no point.  Pass 2, a lane per (channel, dense point): acc = acc + prod over j in order, a coalesced store.  Adding the
// +0.0 of an invalid slot is skipping it: acc starts at +0.0 and a float sum is -0.0 only if both terms are, so acc never
// is, and acc + +0.0 is acc.  LDS path: rows[cc][p] = x[smp, c0 + cc, p] in front of the tile; direct path: x read in place.
template <int CB, bool DIRECT>
__global__ __launch_bounds__(kT) void agg_fwd_kernel(int c, int s, int n, int m, int k, long long units, int nsplit, unsigned chunk,
                                                     const float *__restrict__ x, const int64_t *__restrict__ idx,
                                                     const float *__restrict__ wgt, const float *__restrict__ rel,
                                                     float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // rows [CB][n] (LDS path), prod [CB][kTileWords]
    float *rows = lds, *prod = lds + (DIRECT ? 0 : (size_t)CB * n);
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    const unsigned um = (unsigned)m, uk = (unsigned)k, ks = uk | 1u, pts = (unsigned)kTileSlots / uk;
    const size_t mk = (size_t)um * uk;
    const int g = c / s;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, um, nsplit, chunk);
        const float *xb = x + ((size_t)w.smp * c + w.c0) * n;  // channel c0 + cc: xb + cc * n
        if (!DIRECT) {
            __syncthreads();  // (the previous unit's gathers are done)
            for (int i = tid; i < w.cb * n; i += nt) rows[i] = xb[i];
        }
        int grp[CB];  // the group of channel c0 + cc: at most ceil(CB / S) + 1 different ones
#pragma unroll
        for (int cc = 0; cc < CB; cc++) grp[cc] = (w.c0 + min(cc, w.cb - 1)) / s;
        const int64_t *ib = idx + (size_t)w.smp * mk;
        const float *wb = wgt + (size_t)w.smp * g * mk;                          // group gi: wb + gi * mk
        const float *rb = rel ? rel + ((size_t)w.smp * c + w.c0) * mk : nullptr;  // channel c0 + cc: rb + cc * mk
        float *ob = out + ((size_t)w.smp * c + w.c0) * um;
        for (unsigned p0 = w.lo; p0 < w.hi; p0 += pts) {
            const unsigned np = min(pts, w.hi - p0), ns = np * uk;
            const size_t e0 = (size_t)p0 * uk;
            __syncthreads();  // (the rows are staged; the previous pass's sums are taken)
            for (unsigned sl = (unsigned)tid; sl < ns; sl += (unsigned)nt) {
                const size_t e = e0 + sl;
                const long long raw = ib[e];
                const bool ok = in_range(raw, n);
                const int t = ok ? (int)raw : 0;
                const unsigned at = pcc::padded_at(sl, uk);
                int gi = -1;
                float wv = 0.f;
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        if (grp[cc] != gi) {
                            gi = grp[cc];
                            wv = wb[(size_t)gi * mk + e];
                        }
                        float v;
                        if constexpr (DIRECT) {
                            v = xb[(size_t)cc * n + t];
                        } else {
                            v = rows[cc * n + t];
                        }
                        if (rb) v = v + rb[(size_t)cc * mk + e];
                        const float p = wv * v;
                        prod[cc * kTileWords + at] = ok ? p : 0.f;
                    }
                }
            }
            __syncthreads();
            for (unsigned it = (unsigned)tid; it < (unsigned)w.cb * np; it += (unsigned)nt) {
                const unsigned cc = it / np, row = it - cc * np;
                const float *pr = prod + cc * kTileWords + row * ks;
                float acc = 0.f;
                for (unsigned j = 0; j < uk; j++) acc = acc + pr[j];
                ob[(size_t)cc * um + p0 + row] = canonical_nan(acc);
            }
        }
    }
}

// grad_rel[smp, c0 + cc, e] = w * g[smp, c0 + cc, i] for every slot e = (i, j), +0.0 where the slot is no point, and
// grad_x[smp, c0 + cc, t] += the same products over the slots with idx[e] == t; either may be null.  A lane per slot, whole
// waves (the unit's bounds are multiples of 64 slots): the runs of equal consecutive targets among a wave's 64 slots are
// summed first (a segmented prefix sum, the run structure shared by the CB channels) and the last lane of a run adds.
// LDS path: the bins of the unit live in LDS (zeroed, ds_add_f32, written out whole: every element of grad_x is written);
// direct path: global atomics into grad_x, zero-filled by the host.
template <int CB, bool DIRECT>
__global__ __launch_bounds__(kT) void agg_bwd_kernel(int c, int s, int n, int m, int k, long long units, int nsplit, unsigned chunk,
                                                     const int64_t *__restrict__ idx, const float *__restrict__ wgt,
                                                     const float *__restrict__ go, float *__restrict__ grad_x,
                                                     float *__restrict__ grad_rel) {
    extern __shared__ __attribute__((aligned(16))) float bins[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    const unsigned um = (unsigned)m, uk = (unsigned)k, mk = um * uk;
    const int g = c / s;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, mk, nsplit, chunk);
        if (!DIRECT) pcc::bins_clear(bins, w.cb * n, tid, nt);
        int grp[CB];
#pragma unroll
        for (int cc = 0; cc < CB; cc++) grp[cc] = (w.c0 + min(cc, w.cb - 1)) / s;
        const int64_t *ib = idx + (size_t)w.smp * mk;
        const float *wb = wgt + (size_t)w.smp * g * mk;
        const float *gb = go + ((size_t)w.smp * c + w.c0) * um;
        float *gx = grad_x ? grad_x + ((size_t)w.smp * c + w.c0) * n : nullptr;
        float *gr = grad_rel ? grad_rel + ((size_t)w.smp * c + w.c0) * mk : nullptr;
        for (unsigned base = w.lo + (unsigned)(tid & ~63); base < w.hi; base += (unsigned)nt) {
            const unsigned e = base + (unsigned)lane;
            const bool valid = e < w.hi;
            const long long raw = valid ? ib[e] : -1;
            const int t = in_range(raw, n) ? (int)raw : -1;  // (slots without a point form runs of -1: summed, never added)
            const unsigned i = valid ? e / uk : 0;
            float v[CB];
            int gi = -1;
            float wv = 0.f;
#pragma unroll
            for (int cc = 0; cc < CB; cc++) {
                v[cc] = 0.f;
                if (cc < w.cb && valid) {
                    if (grp[cc] != gi) {
                        gi = grp[cc];
                        wv = wb[(size_t)gi * mk + e];
                    }
                    const float p = wv * gb[(size_t)cc * um + i];
                    v[cc] = t >= 0 ? p : 0.f;
                    if (gr) gr[(size_t)cc * mk + e] = canonical_nan(v[cc]);
                }
            }
            if (!gx) continue;  // (the same in every lane)
            const pcc::WaveRuns runs = pcc::wave_runs(t, lane);
#pragma unroll
            for (int cc = 0; cc < CB; cc++) v[cc] = pcc::seg_prefix_sum(v[cc], runs.masks);
            if (runs.tail) {
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        if constexpr (DIRECT) {
                            atomicAdd(gx + (size_t)cc * n + t, v[cc]);
                        } else {
                            atomicAdd(&bins[cc * n + t], v[cc]);
                        }
                    }
                }
            }
        }
        if (!DIRECT) pcc::bins_store(gx, bins, w.cb * n, tid, nt);
    }
}

// grad_w[smp, gi, e] = sum over the channels ch of group gi, ascending, of g[smp, ch, i] * (x[smp, ch, idx[e]] + rel[smp, ch, e]),
// acc = acc + (g * v) from +0.0: a thread per (group, slot), consecutive lanes consecutive slots (rel is read in whole
// lines, the k lanes of a point read one gradient word, the gathers hit the sample's x in L2).  +0.0 for a slot that is no
// point.
__global__ __launch_bounds__(256) void agg_bwd_w_kernel(int c, int s, int n, int m, int k, long long total, const float *__restrict__ x,
                                                        const int64_t *__restrict__ idx, const float *__restrict__ rel,
                                                        const float *__restrict__ go, float *__restrict__ grad_w) {
    const long long mk = (long long)m * k, stride = (long long)gridDim.x * 256;
    const int g = c / s;
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < total; f += stride) {
        const long long sg = f / mk, e = f - sg * mk;  // sg = smp * g + gi
        const long long smp = sg / g;
        const int gi = (int)(sg - smp * g);
        const unsigned i = (unsigned)(e / k);
        const long long raw = idx[smp * mk + e];
        float acc = 0.f;
        if (in_range(raw, n)) {
            const size_t ch0 = (size_t)smp * c + (size_t)gi * s;
            const float *xp = x + ch0 * n + (size_t)raw;
            const float *gp = go + ch0 * m + i;
            const float *rp = rel ? rel + ch0 * mk + e : nullptr;
            for (int ch = 0; ch < s; ch++) {
                float v = xp[(size_t)ch * n];
                if (rp) v = v + rp[(size_t)ch * mk];
                const float p = gp[(size_t)ch * m] * v;
                acc = acc + p;
            }
        }
        grad_w[f] = canonical_nan(acc);
    }
}

// ---- the softmax over the valid slots of a row ---------------------------------------------------------------------------

// A tile: the rows r0 .. r0 + nr - 1 of the [b * g * m] rows of k slots, contiguous in memory.  Slot q of the tile is word
// r0 * k + q of logits / attn, belongs to row r0 + q / k, and lies in LDS at pcc::padded_at(q, k).
struct SmTile {
    long long r0;
    unsigned nr, ns;
};
__device__ __forceinline__ SmTile sm_tile(long long tile, long long rows, unsigned per, unsigned k) {
    const long long r0 = tile * per;
    const unsigned nr = (unsigned)min((long long)per, rows - r0);
    return {r0, nr, nr * k};
}
// is slot q of the tile a point?  (the list is shared by the g groups of a sample)
__device__ __forceinline__ bool sm_valid(const int64_t *__restrict__ idx, const SmTile &t, unsigned q, unsigned row, int g, int n, int m,
                                         unsigned k) {
    const long long r = t.r0 + row, gm = (long long)g * m, smp = r / gm;
    const long long i = (r - smp * gm) % m;
    return in_range(idx[(smp * m + i) * k + (q - row * k)], n);
}

// attn = exp(l - mx) / sum over the valid slots of the row, the sum in slot order from +0.0; +0.0 at a slot that is no point.
// A NaN logit, a +inf maximum (inf - inf) and a row of -inf make the sum NaN and with it the row; a -inf slot beside a
// finite maximum gives exp(-inf) = 0.
__global__ __launch_bounds__(kSmThreads) void softmax_fwd_kernel(int g, int n, int m, int k, long long rows, long long tiles,
                                                                 const int64_t *__restrict__ idx, const float *__restrict__ logits,
                                                                 float *__restrict__ attn) {
    __shared__ float val[kSmWords];
    __shared__ int okf[kSmWords];
    const unsigned tid = threadIdx.x, uk = (unsigned)k, ks = uk | 1u, per = (unsigned)kSmSlots / uk;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const SmTile t = sm_tile(tile, rows, per, uk);
        const size_t w0 = (size_t)t.r0 * uk;
        __syncthreads();  // (the previous tile is written out)
        for (unsigned q = tid; q < t.ns; q += kSmThreads) {
            const unsigned row = q / uk, at = row * ks + (q - row * uk);  // (pcc::padded_at written out: 1 % slower through it)
            val[at] = logits[w0 + q];
            okf[at] = sm_valid(idx, t, q, row, g, n, m, uk);
        }
        __syncthreads();
        for (unsigned row = tid; row < t.nr; row += kSmThreads) {
            float *v = val + row * ks;
            const int *ok = okf + row * ks;
            float mx = -INFINITY;
            for (unsigned j = 0; j < uk; j++)
                if (ok[j]) mx = fmaxf(mx, v[j]);
            float sum = 0.f;
            for (unsigned j = 0; j < uk; j++) {
                if (ok[j]) {
                    const float ex = expf(v[j] - mx);
                    v[j] = ex;
                    sum = sum + ex;
                }
            }
            for (unsigned j = 0; j < uk; j++) v[j] = ok[j] ? canonical_nan(v[j] / sum) : 0.f;
        }
        __syncthreads();
        for (unsigned q = tid; q < t.ns; q += kSmThreads) {
            const unsigned row = q / uk;
            attn[w0 + q] = val[row * ks + (q - row * uk)];
        }
    }
}

// d = sum over the valid slots of attn * ga in slot order from +0.0, grad_logits = attn * (ga - d); +0.0 at a slot that is
// no point.
__global__ __launch_bounds__(kSmThreads) void softmax_bwd_kernel(int g, int n, int m, int k, long long rows, long long tiles,
                                                                 const int64_t *__restrict__ idx, const float *__restrict__ attn,
                                                                 const float *__restrict__ ga, float *__restrict__ gl) {
    __shared__ float av[kSmWords], gv[kSmWords];
    __shared__ int okf[kSmWords];
    const unsigned tid = threadIdx.x, uk = (unsigned)k, ks = uk | 1u, per = (unsigned)kSmSlots / uk;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const SmTile t = sm_tile(tile, rows, per, uk);
        const size_t w0 = (size_t)t.r0 * uk;
        __syncthreads();
        for (unsigned q = tid; q < t.ns; q += kSmThreads) {
            const unsigned row = q / uk, at = pcc::padded_at(q, uk, row);
            av[at] = attn[w0 + q];
            gv[at] = ga[w0 + q];
            okf[at] = sm_valid(idx, t, q, row, g, n, m, uk);
        }
        __syncthreads();
        for (unsigned row = tid; row < t.nr; row += kSmThreads) {
            const float *a = av + row * ks;
            float *gq = gv + row * ks;
            const int *ok = okf + row * ks;
            float d = 0.f;
            for (unsigned j = 0; j < uk; j++) {
                if (ok[j]) {
                    const float p = a[j] * gq[j];
                    d = d + p;
                }
            }
            for (unsigned j = 0; j < uk; j++) {
                const float df = gq[j] - d;
                gq[j] = ok[j] ? canonical_nan(a[j] * df) : 0.f;
            }
        }
        __syncthreads();
        for (unsigned q = tid; q < t.ns; q += kSmThreads) {
            gl[w0 + q] = gv[pcc::padded_at(q, uk)];
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------

// The checks of the four entry points, sizes before pointers (c = g for the softmax, which has no channels).
int check_sizes(const char *name, int b, int c, int g, int n, int m, int k) {
    pcc::clear_error();
    if (int rc = pcc::check_list_sizes(name, b, c, n, m, k)) return rc;
    if (g < 1 || c % g != 0) return pcc::invalidf("%s: g must be >= 1 and divide c", name);
    if (k > kMaxK) return pcc::invalidf("%s: k > %d", name, kMaxK);
    return PCC_OK;
}

// The plan of interpolate.hip over `len` entries of a sample's list (the interp_path switch forces either path), with
// `tile_words` more words of LDS per channel behind the rows: where those no longer fit beside a single row, the direct path.
pcc::ListPlan make_plan(int b, int c, int n, unsigned len, bool split_lds, unsigned min_chunk, size_t tile_words) {
    pcc::ListPlan p = pcc::make_list_plan(b, c, n, len, split_lds, min_chunk, pcc::tuning(PCC_TUNE_INTERP_PATH));
    if (p.lds && p.lds_bytes + (size_t)p.cb * tile_words * sizeof(float) > pcc::kLdsWg)
        p = pcc::make_list_plan(b, c, n, len, split_lds, min_chunk, 2);
    return p;
}

void launch_bwd(const pcc::ListPlan &p, hipStream_t st, int c, int s, int n, int m, int k, const int64_t *idx, const float *w,
                const float *grad_out, float *grad_x, float *grad_rel) {
    const dim3 block(p.threads((unsigned)m * (unsigned)k, 1));  // a lane per slot
    if (p.lds) {
        static const char *const kNames[] = {"agg_bwd_kernel<lds> cb=1", "agg_bwd_kernel<lds> cb=2",
                                             "agg_bwd_kernel<lds> cb=4", "agg_bwd_kernel<lds> cb=8"};
        pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
        pcc::dispatch_cb(p.cb, [&](auto CB) {
            (void)pcc::allow_lds<agg_bwd_kernel<CB, false>>(pcc::kLdsWg);
            hipLaunchKernelGGL((agg_bwd_kernel<CB, false>), dim3(p.grid()), block, p.lds_bytes, st, c, s, n, m, k, p.units, p.nsplit,
                               p.chunk, idx, w, grad_out, grad_x, grad_rel);
        });
    } else {
        pcc::ProfScope prof("agg_bwd_kernel<direct>", st);
        hipLaunchKernelGGL((agg_bwd_kernel<kCbDirect, true>), dim3(p.grid()), block, 0, st, c, s, n, m, k, p.units, p.nsplit, p.chunk,
                           idx, w, grad_out, grad_x, grad_rel);
    }
}

}  // namespace

extern "C" {

int pcc_neighbour_softmax(int b, int g, int n, int m, int k, const int64_t *idx, const float *logits, float *attn,
                          pcc_stream_t stream) {
    if (int rc = check_sizes("neighbour_softmax", b, g, g, n, m, k)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!idx || !logits || !attn) return pcc::invalid("neighbour_softmax: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long rows = (long long)b * g * m, per = kSmSlots / k, tiles = (rows + per - 1) / per;
    pcc::ProfScope prof("softmax_fwd_kernel", st);
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3(pcc::grid_for(tiles)), dim3(kSmThreads), 0, st, g, n, m, k, rows, tiles, idx, logits,
                       attn);
    return pcc::check_launch("neighbour_softmax");
}

int pcc_neighbour_softmax_bwd(int b, int g, int n, int m, int k, const int64_t *idx, const float *attn, const float *grad_attn,
                              float *grad_logits, pcc_stream_t stream) {
    if (int rc = check_sizes("neighbour_softmax_bwd", b, g, g, n, m, k)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!idx || !attn || !grad_attn || !grad_logits) return pcc::invalid("neighbour_softmax_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long rows = (long long)b * g * m, per = kSmSlots / k, tiles = (rows + per - 1) / per;
    pcc::ProfScope prof("softmax_bwd_kernel", st);
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(pcc::grid_for(tiles)), dim3(kSmThreads), 0, st, g, n, m, k, rows, tiles, idx, attn,
                       grad_attn, grad_logits);
    return pcc::check_launch("neighbour_softmax_bwd");
}

int pcc_aggregate_points(int b, int c, int g, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                         const float *rel, float *out, pcc_stream_t stream) {
    if (int rc = check_sizes("aggregate_points", b, c, g, n, m, k)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!x || !idx || !w || !out) return pcc::invalid("aggregate_points: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int s = c / g;
    const pcc::ListPlan p = make_plan(b, c, n, (unsigned)m, true, kMinChunkPts, kTileWords);
    const unsigned pts = p.chunk < (unsigned)m ? p.chunk : (unsigned)m, per_pass = (unsigned)(kTileSlots / k);
    const dim3 block(p.threads_for((unsigned long long)(pts < per_pass ? pts : per_pass) * k));  // a lane per slot of a pass
    if (p.lds) {
        static const char *const kNames[] = {"agg_fwd_kernel<lds> cb=1", "agg_fwd_kernel<lds> cb=2",
                                             "agg_fwd_kernel<lds> cb=4", "agg_fwd_kernel<lds> cb=8"};
        pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
        pcc::dispatch_cb(p.cb, [&](auto CB) {
            (void)pcc::allow_lds<agg_fwd_kernel<CB, false>>(pcc::kLdsWg);
            hipLaunchKernelGGL((agg_fwd_kernel<CB, false>), dim3(p.grid()), block, p.lds_bytes + (size_t)CB * kTileWords * sizeof(float),
                               st, c, s, n, m, k, p.units, p.nsplit, p.chunk, x, idx, w, rel, out);
        });
    } else {
        pcc::ProfScope prof("agg_fwd_kernel<direct>", st);
        hipLaunchKernelGGL((agg_fwd_kernel<kCbDirect, true>), dim3(p.grid()), block, (size_t)kCbDirect * kTileWords * sizeof(float), st,
                           c, s, n, m, k, p.units, p.nsplit, p.chunk, x, idx, w, rel, out);
    }
    return pcc::check_launch("aggregate_points");
}

int pcc_aggregate_points_bwd(int b, int c, int g, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                             const float *rel, const float *grad_out, float *grad_x, float *grad_w, float *grad_rel,
                             pcc_stream_t stream) {
    if (int rc = check_sizes("aggregate_points_bwd", b, c, g, n, m, k)) return rc;
    if (b == 0 || (!grad_x && !grad_w && !grad_rel)) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t gx_bytes = (size_t)b * c * n * sizeof(float);
    const char *cannot_zero = "aggregate_points_bwd: cannot zero grad_x";
    if (m == 0)  // an empty list: nothing points anywhere, and grad_w and grad_rel have no element
        return grad_x ? pcc::zero_async(grad_x, gx_bytes, st, cannot_zero) : PCC_OK;
    if (!idx || !w || !grad_out || (grad_w && !x)) return pcc::invalid("aggregate_points_bwd: null pointer");
    const int s = c / g;
    const unsigned mk = (unsigned)m * (unsigned)k;
    // the direct plan, its list split over workgroups: grad_rel alone, or beside the global atomics
    const auto direct_plan = [&] { return pcc::make_list_plan(b, c, n, mk, true, kMinChunkSlots, 2); };
    if (grad_x) {
        pcc::ListPlan p = make_plan(b, c, n, mk, false, kMinChunkSlots, 0);
        p.spread_bins(b, c);
        if (!p.lds)
            if (int rc = pcc::zero_async(grad_x, gx_bytes, st, cannot_zero)) return rc;
        // grad_rel rides along unless the bins tie this launch to fewer workgroups than there are compute units
        const bool fused = grad_rel && (!p.lds || p.units >= pcc::device_cus_or(256));
        launch_bwd(p, st, c, s, n, m, k, idx, w, grad_out, grad_x, fused ? grad_rel : nullptr);
        if (grad_rel && !fused) launch_bwd(direct_plan(), st, c, s, n, m, k, idx, w, grad_out, nullptr, grad_rel);
    } else if (grad_rel) {
        launch_bwd(direct_plan(), st, c, s, n, m, k, idx, w, grad_out, nullptr, grad_rel);
    }
    if (grad_w) {
        const long long total = (long long)b * g * m * k, wgs = (total + 255) / 256;
        pcc::ProfScope prof("agg_bwd_w_kernel", st);
        hipLaunchKernelGGL(agg_bwd_w_kernel, dim3(pcc::grid_for(wgs)), dim3(256), 0, st, c, s, n, m, k, total, x, idx, rel, grad_out,
                           grad_w);
    }
    return pcc::check_launch("aggregate_points_bwd");
}

}  // extern "C"
