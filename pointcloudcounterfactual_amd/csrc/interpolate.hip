// Feature propagation along an index list with weights (pcc_interpolate / pcc_interpolate_bwd, include/pcc_neighbour.h),
// gfx950, wave64: out[b,ch,i] = sum_j w[b,i,j] * x[b,ch,idx[b,i,j]] for the m dense points of a pcc_knn_cross list into a
// sparse cloud of n points -- the way back up of an encoder-decoder over point sets, the counterpart of grouping.hip.
//
// The same shape of work as grouping.hip: a workgroup owns CB channels of one sample (chan_block.hpp) and reuses one load
// of a dense point's k indices and weights for its CB channels.  Two paths for the forward and for grad_x, chosen by n
// alone:
//   * LDS     the CB rows of x (forward) or the CB * n gradient bins (grad_x) live in LDS;
//   * direct  where one channel row does not fit a workgroup's LDS: gathers straight from global memory, and global float
//             atomics into a zero-filled grad_x.
// Consecutive lanes take consecutive dense points, so the output is one coalesced store per channel: 16 bytes per lane
// (four consecutive points, non-temporal) where m % 4 == 0 and the bases are 16-byte aligned, a scalar loop otherwise.
// The rows of a k-NN list hold distinct indices, so the backward adds every slot on its own (no run merging as in
// group_bwd_kernel).  grad_w is a thread per slot walking the channels in ascending order: a fixed order, no atomics.
#include "chan_block.hpp"
#include "pcc_common.hpp"

#include <cstdint>

#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"

namespace {

// (a workgroup's unit -- its channels and its dense points lo .. hi - 1 of the sample's m -- and the plan: chan_block.hpp.
// A slot that is not pcc::in_range adds nothing and carries no gradient.)
using pcc::canonical_nan;
using pcc::in_range;
using pcc::kCbDirect;
using pcc::v4f;

constexpr int kT = pcc::kWgThreads;   // threads per workgroup at the most (ListPlan::threads)
constexpr unsigned kMinChunk = 1024;  // dense points per workgroup below which the points of a sample are not split further

// Forward.  LDS path: rows[cc][p] = x[smp, c0 + cc, p]; direct path: x read in place.  P dense points per thread (4 with
// the 16-byte stores, 1 otherwise); per slot j in order, acc = acc + (w * x): a rounded product, then a rounded sum.
// FULL: the workgroup has kT threads (ListPlan::threads), a compile-time stride: measurably faster in the long loops.
template <int CB, bool DIRECT, bool FULL>
__global__ __launch_bounds__(kT) void interp_fwd_kernel(int c, int n, int m, int k, long long units, int nsplit, unsigned chunk,
                                                        const float *__restrict__ x, const int64_t *__restrict__ idx,
                                                        const float *__restrict__ wgt, float *__restrict__ out, int out_c,
                                                        int out_c0) {
    extern __shared__ __attribute__((aligned(16))) float rows[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x, nt = FULL ? kT : (int)blockDim.x;
    const unsigned um = (unsigned)m;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, um, nsplit, chunk);
        const float *xb = x + ((size_t)w.smp * c + w.c0) * n;  // channel c0 + cc: xb + cc * n
        if (!DIRECT) {
            __syncthreads();  // (the previous unit's gathers are done)
            for (int i = tid; i < w.cb * n; i += nt) rows[i] = xb[i];
            __syncthreads();
        }
        auto at = [&](int cc, int t) -> float {
            if constexpr (DIRECT) {
                return xb[(size_t)cc * n + t];
            } else {
                return rows[cc * n + t];
            }
        };
        const int64_t *ib = idx + (size_t)w.smp * um * k;
        const float *wb = wgt + (size_t)w.smp * um * k;
        float *ob = out + ((size_t)w.smp * out_c + out_c0 + w.c0) * um;  // channel c0 + cc of the slice: ob + cc * m
        if ((um & 3) == 0 && (reinterpret_cast<uintptr_t>(ob) & 15) == 0) {
            // four consecutive dense points per thread (lo, hi and m are multiples of 4)
            for (unsigned i4 = w.lo + (unsigned)tid * 4; i4 < w.hi; i4 += (unsigned)nt * 4) {
                float acc[CB][4];
#pragma unroll
                for (int cc = 0; cc < CB; cc++)
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[cc][q] = 0.f;
                const size_t e0 = (size_t)i4 * k;
                for (int j = 0; j < k; j++) {
                    int t[4];
                    bool ok[4];
                    float wv[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const size_t e = e0 + (size_t)q * k + j;
                        const long long raw = ib[e];
                        ok[q] = in_range(raw, n);
                        t[q] = ok[q] ? (int)raw : 0;
                        wv[q] = wb[e];
                    }
#pragma unroll
                    for (int cc = 0; cc < CB; cc++) {
                        if (cc < w.cb) {
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                const float p = wv[q] * at(cc, t[q]);
                                acc[cc][q] = ok[q] ? acc[cc][q] + p : acc[cc][q];
                            }
                        }
                    }
                }
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        const v4f o = {canonical_nan(acc[cc][0]), canonical_nan(acc[cc][1]), canonical_nan(acc[cc][2]),
                                       canonical_nan(acc[cc][3])};
                        __builtin_nontemporal_store(o, reinterpret_cast<v4f *>(ob + (size_t)cc * um + i4));
                    }
                }
            }
        } else {
            for (unsigned i = w.lo + (unsigned)tid; i < w.hi; i += (unsigned)nt) {
                float acc[CB];
#pragma unroll
                for (int cc = 0; cc < CB; cc++) acc[cc] = 0.f;
                const size_t e0 = (size_t)i * k;
                for (int j = 0; j < k; j++) {
                    const long long raw = ib[e0 + j];
                    const bool ok = in_range(raw, n);
                    const int t = ok ? (int)raw : 0;
                    const float wv = wb[e0 + j];
#pragma unroll
                    for (int cc = 0; cc < CB; cc++) {
                        if (cc < w.cb) {
                            const float p = wv * at(cc, t);
                            acc[cc] = ok ? acc[cc] + p : acc[cc];
                        }
                    }
                }
#pragma unroll
                for (int cc = 0; cc < CB; cc++)
                    if (cc < w.cb) ob[(size_t)cc * um + i] = canonical_nan(acc[cc]);
            }
        }
    }
}

// grad_x[smp, c0 + cc, t] += w[e] * g[smp, out_c0 + c0 + cc, i] over the in-range slots e = (i, j) with idx[e] == t.
// LDS path: the bins of the unit live in LDS (zeroed, ds_add_f32, written out whole: every element of grad_x is written);
// direct path: global atomics into grad_x, zero-filled by the host.  A lane takes a dense point: its CB gradient words
// are loaded once (coalesced) and meet each of its k slots.
template <int CB, bool DIRECT, bool FULL>
__global__ __launch_bounds__(kT) void interp_bwd_x_kernel(int c, int n, int m, int k, long long units, int nsplit, unsigned chunk,
                                                          const int64_t *__restrict__ idx, const float *__restrict__ wgt,
                                                          const float *__restrict__ g, int out_c, int out_c0,
                                                          float *__restrict__ grad_x) {
    extern __shared__ __attribute__((aligned(16))) float bins[];  // [CB][n] (LDS path)
    const int tid = threadIdx.x, nt = FULL ? kT : (int)blockDim.x;
    const unsigned um = (unsigned)m;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const pcc::ListUnit w = pcc::list_unit<CB>(u, c, um, nsplit, chunk);
        if (!DIRECT) pcc::bins_clear(bins, w.cb * n, tid, nt);
        const int64_t *ib = idx + (size_t)w.smp * um * k;
        const float *wb = wgt + (size_t)w.smp * um * k;
        const float *gb = g + ((size_t)w.smp * out_c + out_c0 + w.c0) * um;
        float *gx = grad_x + ((size_t)w.smp * c + w.c0) * n;
        for (unsigned i = w.lo + (unsigned)tid; i < w.hi; i += (unsigned)nt) {
            float gv[CB];
#pragma unroll
            for (int cc = 0; cc < CB; cc++) gv[cc] = cc < w.cb ? gb[(size_t)cc * um + i] : 0.f;
            const size_t e0 = (size_t)i * k;
            for (int j = 0; j < k; j++) {
                const long long raw = ib[e0 + j];
                if (!in_range(raw, n)) continue;
                const int t = (int)raw;
                const float wv = wb[e0 + j];
#pragma unroll
                for (int cc = 0; cc < CB; cc++) {
                    if (cc < w.cb) {
                        if constexpr (DIRECT) {
                            atomicAdd(gx + (size_t)cc * n + t, wv * gv[cc]);
                        } else {
                            atomicAdd(&bins[cc * n + t], wv * gv[cc]);
                        }
                    }
                }
            }
        }
        if (!DIRECT) pcc::bins_store(gx, bins, w.cb * n, tid, nt);
    }
}

// grad_w[smp, i, j] = sum over ch ascending of g[smp, out_c0 + ch, i] * x[smp, ch, idx[smp, i, j]], acc = acc + (g * x) from
// +0: a thread per slot, consecutive lanes consecutive slots (the k lanes of a point read one gradient word; the gathers
// hit the sample's x in L2).  +0.0 for an out-of-range slot.
__global__ __launch_bounds__(256) void interp_bwd_w_kernel(int c, int n, int m, int k, long long slots, const float *__restrict__ x,
                                                           const int64_t *__restrict__ idx, const float *__restrict__ g, int out_c,
                                                           int out_c0, float *__restrict__ grad_w) {
    const long long per = (long long)m * k, stride = (long long)gridDim.x * 256;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < slots; s += stride) {
        const long long smp = s / per;
        const unsigned i = (unsigned)((s - smp * per) / k);
        const long long raw = idx[s];
        float acc = 0.f;
        if (in_range(raw, n)) {
            const float *xp = x + (size_t)smp * c * n + (size_t)raw;
            const float *gp = g + ((size_t)smp * out_c + out_c0) * m + i;
            for (int ch = 0; ch < c; ch++) {
                const float p = gp[(size_t)ch * m] * xp[(size_t)ch * n];
                acc = acc + p;
            }
        }
        grad_w[s] = acc;
    }
}

// The plan of a call over the m dense points of a sample (the interp_path switch forces either path)
pcc::ListPlan make_plan(int b, int c, int n, int m, bool split_lds) {
    return pcc::make_list_plan(b, c, n, (unsigned)m, split_lds, kMinChunk, pcc::tuning(PCC_TUNE_INTERP_PATH));
}

// f(std::bool_constant<the workgroup has kT threads>)
template <class F>
void full_or_not(const dim3 &block, F &&f) {
    if (block.x == (unsigned)kT) return f(std::true_type{});
    f(std::false_type{});
}

int check_sizes(const char *name, int b, int c, int n, int m, int k, int out_c, int out_c0) {
    pcc::clear_error();
    if (int rc = pcc::check_list_sizes(name, b, c, n, m, k)) return rc;
    return pcc::check_out_slice(name, c, out_c, out_c0);
}

}  // namespace

extern "C" {

int pcc_interpolate(int b, int c, int n, int m, int k, const float *x, const int64_t *idx, const float *w, float *out,
                    int out_c, int out_c0, pcc_stream_t stream) {
    if (int rc = check_sizes("interpolate", b, c, n, m, k, out_c, out_c0)) return rc;
    if (b == 0 || m == 0) return PCC_OK;
    if (!x || !idx || !w || !out) return pcc::invalid("interpolate: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const pcc::ListPlan p = make_plan(b, c, n, m, true);
    // (four points per thread where the kernel takes its 16-byte stores: the same test as there, every channel row of the
    // slice is aligned when the base is and m % 4 == 0)
    const dim3 block(p.threads((unsigned)m, (m & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 4 : 1));
    if (p.lds) {
        static const char *const kNames[] = {"interp_fwd_kernel<lds> cb=1", "interp_fwd_kernel<lds> cb=2",
                                             "interp_fwd_kernel<lds> cb=4", "interp_fwd_kernel<lds> cb=8"};
        pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
        pcc::dispatch_cb(p.cb, [&](auto CB) {
            full_or_not(block, [&](auto FULL) {
                (void)pcc::allow_lds<interp_fwd_kernel<CB, false, FULL>>(pcc::kLdsWg);
                hipLaunchKernelGGL((interp_fwd_kernel<CB, false, FULL>), dim3(p.grid()), block, p.lds_bytes, st, c, n, m, k, p.units,
                                   p.nsplit, p.chunk, x, idx, w, out, out_c, out_c0);
            });
        });
    } else {
        pcc::ProfScope prof("interp_fwd_kernel<direct>", st);
        full_or_not(block, [&](auto FULL) {
            hipLaunchKernelGGL((interp_fwd_kernel<kCbDirect, true, FULL>), dim3(p.grid()), block, 0, st, c, n, m, k, p.units,
                               p.nsplit, p.chunk, x, idx, w, out, out_c, out_c0);
        });
    }
    return pcc::check_launch("interpolate");
}

int pcc_interpolate_bwd(int b, int c, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                        const float *grad_out, int out_c, int out_c0, float *grad_x, float *grad_w, pcc_stream_t stream) {
    if (int rc = check_sizes("interpolate_bwd", b, c, n, m, k, out_c, out_c0)) return rc;
    if (b == 0 || (!grad_x && !grad_w)) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t gx_bytes = (size_t)b * c * n * sizeof(float);
    const char *cannot_zero = "interpolate_bwd: cannot zero grad_x";
    if (m == 0)  // an empty list: nothing points anywhere, and grad_w has no element
        return grad_x ? pcc::zero_async(grad_x, gx_bytes, st, cannot_zero) : PCC_OK;
    if (!idx || !w || !grad_out || (grad_w && !x)) return pcc::invalid("interpolate_bwd: null pointer");
    if (grad_x) {
        const pcc::ListPlan p = make_plan(b, c, n, m, false);
        const dim3 block(p.threads((unsigned)m, 1));
        if (p.lds) {
            static const char *const kNames[] = {"interp_bwd_x_kernel<lds> cb=1", "interp_bwd_x_kernel<lds> cb=2",
                                                 "interp_bwd_x_kernel<lds> cb=4", "interp_bwd_x_kernel<lds> cb=8"};
            pcc::ProfScope prof(kNames[pcc::cb_index(p.cb)], st);
            pcc::dispatch_cb(p.cb, [&](auto CB) {
                full_or_not(block, [&](auto FULL) {
                    (void)pcc::allow_lds<interp_bwd_x_kernel<CB, false, FULL>>(pcc::kLdsWg);
                    hipLaunchKernelGGL((interp_bwd_x_kernel<CB, false, FULL>), dim3(p.grid()), block, p.lds_bytes, st, c, n, m, k,
                                       p.units, p.nsplit, p.chunk, idx, w, grad_out, out_c, out_c0, grad_x);
                });
            });
        } else {
            if (int rc = pcc::zero_async(grad_x, gx_bytes, st, cannot_zero)) return rc;
            pcc::ProfScope prof("interp_bwd_x_kernel<direct>", st);
            full_or_not(block, [&](auto FULL) {
                hipLaunchKernelGGL((interp_bwd_x_kernel<kCbDirect, true, FULL>), dim3(p.grid()), block, 0, st, c, n, m, k, p.units,
                                   p.nsplit, p.chunk, idx, w, grad_out, out_c, out_c0, grad_x);
            });
        }
    }
    if (grad_w) {
        const long long slots = (long long)b * m * k, wgs = (slots + 255) / 256;
        pcc::ProfScope prof("interp_bwd_w_kernel", st);
        hipLaunchKernelGGL(interp_bwd_w_kernel, dim3(pcc::grid_for(wgs)), dim3(256), 0, st, c, n, m, k, slots, x, idx, grad_out, out_c,
                           out_c0, grad_w);
    }
    return pcc::check_launch("interpolate_bwd");
}

}  // extern "C"
