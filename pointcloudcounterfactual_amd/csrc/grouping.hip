// Grouping along an index list that belongs to ANOTHER point set (pcc_group_points / pcc_group_points_bwd,
// include/pcc_neighbour.h), gfx950, wave64: idx[b,m,k] into a cloud of n points, m != n allowed -- the third step of a
// set-abstraction front end (pcc_fps -> pcc_ball_query -> here) and the gather along a pcc_knn_cross list.
//
// Like gather_lds_kernel / scatter_lds_kernel of graph_ops.hip, an HBM-bound index-driven copy: a workgroup owns CB
// channels of one sample (chan_block.hpp), streams the m*k index list coalesced and reuses one index load for its CB
// channels.  Two paths, chosen by n alone:
//   * LDS     the CB rows of x (forward) or the CB * n gradient bins (backward) live in LDS; the point-major layout is a
//             transposing load / store of that tile, not another kernel;
//   * direct  where one channel row does not fit a workgroup's LDS: gathers straight from global memory, and global float
//             atomics into a zero-filled grad_x.
// The forward writes 16 bytes per lane with non-temporal stores where m*k % 4 == 0 and the bases are 16-byte aligned
// (then every channel of the out_c0 slice is: its offset is a multiple of m*k floats); a scalar loop otherwise.
// The backward meets the duplicate structure of ball-query rows (ascending indices, then one index repeated to the end
// of the row; 64 lanes adding into one address serialise): every wave first sums the runs of equal consecutive targets
// among its 64 consecutive slots -- a segmented prefix sum over DPP moves, the run structure computed once from a ballot
// and shared by the CB channels -- and only the last lane of a run issues the atomic.  A list without such runs pays six
// masked adds per channel for nothing; a pad-only row becomes one atomic per 64 slots.
#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "wave_ops.hpp"

#include <cstdint>

#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"

namespace {

// (a workgroup's unit -- its channels and its slots lo .. hi - 1 of the sample's m * k -- and the plan: chan_block.hpp.
// A slot that is not pcc::in_range is +0 forward and carries no gradient.)
using pcc::in_range;
using pcc::kCbDirect;
using pcc::v2l;
using pcc::v4f;

constexpr int kT = pcc::kWgThreads;   // threads per workgroup
constexpr unsigned kMinChunk = 8192;  // slots per workgroup below which the list of a sample is not split further

// Forward.  LDS path: rows[cc][p] = x[smp, c0 + cc, p], staged from either layout; direct path: x read in place.
template <int CB, bool DIRECT>
__global__ __launch_bounds__(kT) void group_fwd_kernel(int c, int n, int m, int k, int point_major, long long units, int nsplit,
                                                       unsigned chunk, const float *__restrict__ x,
                                                       const int64_t *__restrict__ idx, const float *__restrict__ centre,
                                                       float *__restrict__ out, int out_c, int out_c0) {
    extern __shared__ __attribute__((aligned(16))) float rows[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x;
    const unsigned mk = (unsigned)m * (unsigned)k;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, mk, nsplit, chunk);
        const float *xb = x + (size_t)w.smp * c * n;
        if (!DIRECT) {
            __syncthreads();  // (the previous unit's gathers are done)
            if (point_major) {
                // the transposing load: consecutive lanes take consecutive points of one channel (stride c in memory --
                // for xyz three lanes per 36 bytes), so the LDS stores are conflict-free
                for (int i = tid; i < w.cb * n; i += kT) {
                    const int cc = i / n, p = i - cc * n;
                    rows[i] = xb[(size_t)p * c + w.c0 + cc];
                }
            } else {
                const float *src = xb + (size_t)w.c0 * n;
                for (int i = tid; i < w.cb * n; i += kT) rows[i] = src[i];
            }
            __syncthreads();
        }
        // x[smp, c0 + cc, t]
        auto at = [&](int cc, int t) -> float {
            if constexpr (DIRECT) {
                return point_major ? xb[(size_t)t * c + w.c0 + cc] : xb[(size_t)(w.c0 + cc) * n + t];
            } else {
                return rows[cc * n + t];
            }
        };
        // centre[smp, c0 + cc, i]: neighbouring lanes read the same or the next word
        auto cen = [&](int cc, unsigned i) -> float {
            return point_major ? centre[((size_t)w.smp * m + i) * c + w.c0 + cc] : centre[((size_t)w.smp * c + w.c0 + cc) * m + i];
        };
        const int64_t *ib = idx + (size_t)w.smp * mk;
        float *ob = out + ((size_t)w.smp * out_c + out_c0 + w.c0) * mk;  // channel c0 + cc of the slice: ob + cc * mk
        if ((mk & 3) == 0 && ((reinterpret_cast<uintptr_t>(ib) | reinterpret_cast<uintptr_t>(ob)) & 15) == 0) {
            // four consecutive slots per thread (lo, hi and mk are multiples of 4): the output is a write-only stream many
            // times the L2, stored as 16 bytes per lane; the index list as two 16-byte loads
            for (unsigned e4 = w.lo + (unsigned)tid * 4; e4 < w.hi; e4 += kT * 4) {
                const v2l ia = *reinterpret_cast<const v2l *>(ib + e4), ic = *reinterpret_cast<const v2l *>(ib + e4 + 2);
                const long long raw[4] = {ia.x, ia.y, ic.x, ic.y};
                int t[4];
                bool ok[4];
                unsigned i[4] = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    ok[q] = in_range(raw[q], n);
                    t[q] = ok[q] ? (int)raw[q] : 0;
                }
                if (centre) {  // the centres of the four slots (any k >= 1)
                    unsigned row = e4 / (unsigned)k, r = e4 - row * (unsigned)k;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        i[q] = row;
                        if (++r == (unsigned)k) r = 0, ++row;
                    }
                }
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        float v[4];
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            v[q] = at(cc, t[q]);
                            if (centre) v[q] -= cen(cc, i[q]);
                            v[q] = ok[q] ? v[q] : 0.f;
                        }
                        const v4f o = {v[0], v[1], v[2], v[3]};
                        __builtin_nontemporal_store(o, reinterpret_cast<v4f *>(ob + (size_t)cc * mk + e4));
                    }
                }
            }
        } else {
            for (unsigned e = w.lo + (unsigned)tid; e < w.hi; e += kT) {
                const long long raw = ib[e];
                const bool ok = in_range(raw, n);
                const int t = ok ? (int)raw : 0;
                const unsigned i = centre ? e / (unsigned)k : 0u;
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        float v = at(cc, t);
                        if (centre) v -= cen(cc, i);
                        ob[(size_t)cc * mk + e] = ok ? v : 0.f;
                    }
                }
            }
        }
    }
}

// Backward of the gather: grad_x[smp, c0 + cc, t] += g[smp, out_c0 + c0 + cc, e] over the slots e with idx[e] == t.
// LDS path: the bins of the unit live in LDS (zeroed, ds_add_f32, written out whole: every element of grad_x is
// written); direct path: global atomics into grad_x, zero-filled by the host.  Either way the 64 consecutive slots of a
// wave are first reduced over their runs of equal consecutive targets, and one lane per run adds.
template <int CB, bool DIRECT>
__global__ __launch_bounds__(kT) void group_bwd_kernel(int c, int n, int m, int k, int point_major, long long units, int nsplit,
                                                       unsigned chunk, const int64_t *__restrict__ idx,
                                                       const float *__restrict__ g, int out_c, int out_c0,
                                                       float *__restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) float bins[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15;
    const unsigned mk = (unsigned)m * (unsigned)k;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, mk, nsplit, chunk);
        if (!DIRECT) {
            __syncthreads();  // (the previous unit's bins are written out)
            for (int i = tid; i < w.cb * n; i += kT) bins[i] = 0.f;
            __syncthreads();
        }
        const int64_t *ib = idx + (size_t)w.smp * mk;
        const float *gb = g + ((size_t)w.smp * out_c + out_c0 + w.c0) * mk;
        float *gx = grad_x + (size_t)w.smp * c * n;
        // whole waves walk the list (lo is a multiple of 64, the bound is wave-uniform): DPP and ballot need every lane
        for (unsigned base = w.lo + (unsigned)(tid & ~63); base < w.hi; base += kT) {
            const unsigned e = base + (unsigned)lane;
            const bool valid = e < w.hi;
            const long long raw = valid ? ib[e] : -1;
            const int t = in_range(raw, n) ? (int)raw : -1;  // (slots without a point form runs of -1: summed, never added)
            float v[CB];
#pragma unroll
            for (int cc = 0; cc < CB; cc++) v[cc] = valid && cc < w.cb ? gb[(size_t)cc * mk + e] : 0.f;
            // the runs of equal consecutive targets among these 64 slots: bit l of `heads` = lane l opens a run; a lane
            // adds its partner at a step of the prefix sum iff the partner is not before the head of the lane's run
            const int tp = __shfl_up(t, 1, 64);
            const unsigned long long heads = __ballot(lane == 0 || tp != t);
            const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
            const pcc::SegMasks runs = {-(int)(lr >= 1 && lane - 1 >= head), -(int)(lr >= 2 && lane - 2 >= head),
                                        -(int)(lr >= 4 && lane - 4 >= head), -(int)(lr >= 8 && lane - 8 >= head),
                                        -(int)((lane & 16) != 0 && lane - lr - 1 >= head), -(int)(lane >= 32 && 31 >= head)};
            const bool tail = t >= 0 && (lane == 63 || ((heads >> ((lane + 1) & 63)) & 1ull) != 0);
#pragma unroll
            for (int cc = 0; cc < CB; cc++) v[cc] = pcc::seg_prefix_sum(v[cc], runs);
            if (tail) {
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        if constexpr (DIRECT) {
                            atomicAdd(point_major ? gx + (size_t)t * c + w.c0 + cc : gx + (size_t)(w.c0 + cc) * n + t, v[cc]);
                        } else {
                            atomicAdd(&bins[cc * n + t], v[cc]);
                        }
                    }
                }
            }
        }
        if (!DIRECT) {
            __syncthreads();
            if (point_major) {  // the transposing store, as the forward loads
                for (int i = tid; i < w.cb * n; i += kT) {
                    const int cc = i / n, p = i - cc * n;
                    gx[(size_t)p * c + w.c0 + cc] = bins[i];
                }
            } else {
                float *dst = gx + (size_t)w.c0 * n;
                for (int i = tid; i < w.cb * n; i += kT) dst[i] = bins[i];
            }
        }
    }
}

// grad_centre[smp, ch, i] = -(sum over the in-range slots j of row i of g[smp, out_c0 + ch, i, j]): one wave per row of the
// list, the lanes striding over its k slots (coalesced), the channels in turn; a fixed summation order, no atomics.
__global__ __launch_bounds__(256) void group_centre_bwd_kernel(int c, int n, int m, int k, int point_major, long long rows,
                                                               const int64_t *__restrict__ idx, const float *__restrict__ g,
                                                               int out_c, int out_c0, float *__restrict__ grad_centre) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += stride) {
        const long long smp = r / m;
        const int i = (int)(r - smp * m);
        const int64_t *ib = idx + (size_t)r * k;
        for (int ch = 0; ch < c; ch++) {
            const float *gr = g + (((size_t)smp * out_c + out_c0 + ch) * m + i) * k;
            float sum = 0.f;
            for (int j = lane; j < k; j += 64) sum += in_range(ib[j], n) ? gr[j] : 0.f;
            sum = pcc::wave_sum_down(sum);
            if (lane == 0) grad_centre[point_major ? ((size_t)smp * m + i) * c + ch : ((size_t)smp * c + ch) * m + i] = -sum;
        }
    }
}

// The plan of a call over the m * k slots of a sample (the group_path switch forces either path)
pcc::ListPlan make_plan(int b, int c, int n, int m, int k, bool split_lds) {
    return pcc::make_list_plan(b, c, n, (unsigned)m * (unsigned)k, split_lds, kMinChunk, pcc::tuning(PCC_TUNE_GROUP_PATH));
}

int check_sizes(const char *name, int b, int c, int n, int m, int k, int point_major, int out_c, int out_c0) {
    pcc::clear_error();
    if (int rc = pcc::check_list_sizes(name, b, c, n, m, k)) return rc;
    if (int rc = pcc::check_out_slice(name, c, out_c, out_c0)) return rc;
    if (point_major != 0 && point_major != 1) return pcc::invalidf("%s: point_major must be 0 or 1", name);
    return PCC_OK;
}

}  // namespace

extern "C" {

int pcc_group_points(int b, int c, int n, int m, int k, int point_major, const float *x, const int64_t *idx,
                     const float *centre, float *out, int out_c, int out_c0, pcc_stream_t stream) {
    if (int rc = check_sizes("group_points", b, c, n, m, k, point_major, out_c, out_c0)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!x || !idx || !out) return pcc::invalid("group_points: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const pcc::ListPlan p = make_plan(b, c, n, m, k, true);
    if (p.lds) {
        static const char *const kNames[] = {"group_fwd_kernel<lds> cb=1", "group_fwd_kernel<lds> cb=2",
                                             "group_fwd_kernel<lds> cb=4", "group_fwd_kernel<lds> cb=8"};
        pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
        pcc::dispatch_cb(p.cb, [&](auto CB) {
            (void)pcc::allow_lds<group_fwd_kernel<CB, false>>(pcc::kLdsWg);
            hipLaunchKernelGGL((group_fwd_kernel<CB, false>), dim3(p.grid()), dim3(kT), p.lds_bytes, st, c, n, m, k, point_major,
                               p.units, p.nsplit, p.chunk, x, idx, centre, out, out_c, out_c0);
        });
    } else {
        pcc::ProfScope prof("group_fwd_kernel<direct>", st);
        hipLaunchKernelGGL((group_fwd_kernel<kCbDirect, true>), dim3(p.grid()), dim3(kT), 0, st, c, n, m, k, point_major, p.units,
                           p.nsplit, p.chunk, x, idx, centre, out, out_c, out_c0);
    }
    return pcc::check_launch("group_points");
}

int pcc_group_points_bwd(int b, int c, int n, int m, int k, int point_major, const int64_t *idx, const float *grad_out,
                         int out_c, int out_c0, float *grad_x, float *grad_centre, pcc_stream_t stream) {
    if (int rc = check_sizes("group_points_bwd", b, c, n, m, k, point_major, out_c, out_c0)) return rc;
    if (b == 0 || (!grad_x && !grad_centre)) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t gx_bytes = (size_t)b * c * n * sizeof(float);
    const char *cannot_zero = "group_points_bwd: cannot zero grad_x";
    if (m == 0)  // an empty list: nothing points anywhere
        return grad_x ? pcc::zero_async(grad_x, gx_bytes, st, cannot_zero) : PCC_OK;
    if (!idx || !grad_out) return pcc::invalid("group_points_bwd: null pointer");
    if (grad_x) {
        const pcc::ListPlan p = make_plan(b, c, n, m, k, false);
        if (p.lds) {
            static const char *const kNames[] = {"group_bwd_kernel<lds> cb=1", "group_bwd_kernel<lds> cb=2",
                                                 "group_bwd_kernel<lds> cb=4", "group_bwd_kernel<lds> cb=8"};
            pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
            pcc::dispatch_cb(p.cb, [&](auto CB) {
                (void)pcc::allow_lds<group_bwd_kernel<CB, false>>(pcc::kLdsWg);
                hipLaunchKernelGGL((group_bwd_kernel<CB, false>), dim3(p.grid()), dim3(kT), p.lds_bytes, st, c, n, m, k,
                                   point_major, p.units, p.nsplit, p.chunk, idx, grad_out, out_c, out_c0, grad_x);
            });
        } else {
            if (int rc = pcc::zero_async(grad_x, gx_bytes, st, cannot_zero)) return rc;
            pcc::ProfScope prof("group_bwd_kernel<direct>", st);
            hipLaunchKernelGGL((group_bwd_kernel<kCbDirect, true>), dim3(p.grid()), dim3(kT), 0, st, c, n, m, k, point_major,
                               p.units, p.nsplit, p.chunk, idx, grad_out, out_c, out_c0, grad_x);
        }
    }
    if (grad_centre) {
        const long long rows = (long long)b * m, wgs = (rows + 3) / 4;
        pcc::ProfScope prof("group_centre_bwd_kernel", st);
        hipLaunchKernelGGL(group_centre_bwd_kernel, dim3(pcc::grid_for(wgs)), dim3(256), 0, st, c, n, m, k, point_major, rows, idx, grad_out, out_c, out_c0, grad_centre);
    }
    return pcc::check_launch("group_points_bwd");
}

}  // extern "C"
