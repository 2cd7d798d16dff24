// Cost and gradients over a STORED match tensor for gfx950 (MI355X), wave64: replaces matchcostkernel and
// matchcostgrad{1,2}kernel (external/pytorch_structural_losses/src/approxmatch.cu:200-326).  The reference re-reads match
// three times; here the cost is one read, both gradients ONE read (HBM bound); no level machinery (approxmatch.hip).
#include "approxmatch.hpp"
#include "wave_ops.hpp"

namespace {

using pcc::sq3;

// out[b] = sum_p part[b][p] in index order (deterministic second stage of every cost reduction).
__global__ __launch_bounds__(256) void reduce_rows_kernel(int parts, const float *__restrict__ part,
                                                           float *__restrict__ out) {
    __shared__ float red[256];
    const int smp = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < parts; i += 256) s += part[(size_t)smp * parts + i];
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[smp] = red[0];
}

// ---------------------------------------------------------------------------------------------------
// matchcost: "row" kernel.  A workgroup takes RT rows (query points l of set2) of one sample; set1 is
// staged SoA in LDS chunk by chunk; each wave streams whole rows of match with coalesced float4 loads
// (1 KiB per wave-instruction).  Cost partial = sum match * sqrt(d2)   (approxmatch.cu:200-209)
// ---------------------------------------------------------------------------------------------------
constexpr int kRowRT = 32;  // rows per workgroup -> 8 per wave

template <bool VEC>
__global__ __launch_bounds__(256) void am_row_kernel(int n, int m, const float *__restrict__ xyz1,
                                                      const float *__restrict__ xyz2,
                                                      const float *__restrict__ match, float *__restrict__ out) {
    constexpr int RPW = kRowRT / 4, CH = 2048;  // (set1 points staged per chunk)
    __shared__ __attribute__((aligned(16))) float lds_p[3 * CH];
    __shared__ float lds_red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int smp = blockIdx.y;
    const int r0 = blockIdx.x * kRowRT;
    const float *p1 = xyz1 + (size_t)smp * n * 3;
    const float *p2 = xyz2 + (size_t)smp * m * 3;
    const float4 *X4 = reinterpret_cast<const float4 *>(lds_p);
    const float4 *Y4 = X4 + CH / 4;
    const float4 *Z4 = Y4 + CH / 4;

    float csum = 0.f;

    for (int q0 = 0; q0 < n; q0 += CH) {
        const int cnt = min(CH, n - q0);
        if (q0) __syncthreads();
        for (int i = tid; i < cnt * 3; i += 256) {
            const float v = p1[(size_t)q0 * 3 + i];
            const int p = i / 3;
            lds_p[(i - p * 3) * CH + p] = v;
        }
        for (int i = cnt + tid; i < ((cnt + 3) & ~3); i += 256) lds_p[i] = lds_p[CH + i] = lds_p[2 * CH + i] = 0.f;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < RPW; i++) {
            const int row = r0 + w + 4 * i;
            const bool live = row < m;  // wave-uniform
            const int rowc = live ? row : m - 1;
            const float x2 = p2[rowc * 3 + 0], y2 = p2[rowc * 3 + 1], z2 = p2[rowc * 3 + 2];
            const float *mrow = match + ((size_t)smp * m + rowc) * n + q0;
            for (int k = lane * 4; live && k < cnt; k += 256) {
                float mv[4];
                if (VEC && k + 3 < cnt) {
                    const v4f t4 = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(mrow + k));
                    const float4 t = make_float4(t4.x, t4.y, t4.z, t4.w);
                    mv[0] = t.x; mv[1] = t.y; mv[2] = t.z; mv[3] = t.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) mv[q] = (k + q < cnt) ? mrow[k + q] : 0.f;
                }
                const float4 xs = X4[k >> 2], ys = Y4[k >> 2], zs = Z4[k >> 2];
                const float px[4] = {xs.x, xs.y, xs.z, xs.w};
                const float py[4] = {ys.x, ys.y, ys.z, ys.w};
                const float pz[4] = {zs.x, zs.y, zs.z, zs.w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float dx = x2 - px[q], dy = y2 - py[q], dz = z2 - pz[q];
                    csum = __builtin_fmaf(mv[q], __builtin_amdgcn_sqrtf(sq3(dx, dy, dz)), csum);
                }
            }
        }
    }
    csum = pcc::wave_sum_down(csum);
    if (lane == 0) lds_red[w] = csum;
    __syncthreads();
    if (tid == 0) out[(size_t)smp * gridDim.x + blockIdx.x] = ((lds_red[0] + lds_red[1]) + lds_red[2]) + lds_red[3];
}

// ---------------------------------------------------------------------------------------------------
// matchcostgrad, fused: ONE read of match produces both gradients (the reference reads it twice,
// approxmatch.cu:319-320).  A workgroup takes RT rows (points k of set2) x a 2048-column slab (points l of set1);
// a wave streams whole row segments with float4 loads; per element t = d * match * rsqrt(max(|d|^2,1e-20)):
//   grad1[l] += t   (column sums: 4 columns x 3 components per lane per 256-column step, kept in registers,
//                    merged over the 4 waves in LDS, written as one partial per row tile)
//   grad2[k] -= t   (row sums: per-lane partials, wave butterfly at the end of the row segment)
// Partials are combined in a fixed order by reduce_splits_kernel / the slab loop: deterministic.
// ---------------------------------------------------------------------------------------------------
constexpr int kGradRT = 64;     // rows per workgroup (16 per wave)
constexpr int kGradSlab = 1024;  // columns per slab = 4 steps of 256 (48 column-sum registers per lane; 2048 -> 175 us, 1024 -> 129 us, 512 -> 134 us at B=32,N=2048)

template <bool VEC>
__global__ __launch_bounds__(256) void am_grad_fused_kernel(int n, int m, int row_tiles,
                                                             const float *__restrict__ xyz1,
                                                             const float *__restrict__ xyz2,
                                                             const float *__restrict__ match,
                                                             float *__restrict__ part1,  // [b][row_tiles][n][3]
                                                             float *__restrict__ part2,  // [b][slabs][m][3]
                                                             const float *__restrict__ scale2)  // applied when part2 IS grad2
{
    constexpr int STEPS = kGradSlab / 256;
    // set1 slab SoA (24 KiB); after the row loop the same bytes carry one wave's column sums at a time to wave 0
    __shared__ __attribute__((aligned(16))) float lds_p[3 * kGradSlab > STEPS * 12 * 64 ? 3 * kGradSlab : STEPS * 12 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int smp = blockIdx.z, slab = blockIdx.y, rt = blockIdx.x;
    const int c0 = slab * kGradSlab;
    const int cnt = min(kGradSlab, n - c0);
    const float *p1 = xyz1 + ((size_t)smp * n + c0) * 3;
    const float *p2 = xyz2 + (size_t)smp * m * 3;
    for (int i = tid; i < cnt * 3; i += 256) {
        const float v = p1[i];
        const int p = i / 3;
        lds_p[(i - p * 3) * kGradSlab + p] = v;
    }
    for (int i = cnt + tid; i < kGradSlab; i += 256) lds_p[i] = lds_p[kGradSlab + i] = lds_p[2 * kGradSlab + i] = 0.f;
    __syncthreads();
    const float4 *X4 = reinterpret_cast<const float4 *>(lds_p);
    const float4 *Y4 = X4 + kGradSlab / 4;
    const float4 *Z4 = Y4 + kGradSlab / 4;

    float g1[STEPS][4][3];
#pragma unroll
    for (int st = 0; st < STEPS; st++)
#pragma unroll
        for (int q = 0; q < 4; q++) g1[st][q][0] = g1[st][q][1] = g1[st][q][2] = 0.f;

    const int r_begin = rt * kGradRT, r_end = min(r_begin + kGradRT, m);
    const bool full = VEC && cnt == kGradSlab;  // whole slab, aligned: branch-free body, 8 row loads in flight
    for (int row = r_begin + w; row < r_end; row += 4) {
        const float x2 = p2[row * 3 + 0], y2 = p2[row * 3 + 1], z2 = p2[row * 3 + 2];
        const float *mrow = match + ((size_t)smp * m + row) * n + c0;
        float rx = 0.f, ry = 0.f, rz = 0.f;
        float mv[STEPS][4];
        if (full) {
#pragma unroll
            for (int st = 0; st < STEPS; st++) {
                const v4f t4 = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(mrow + st * 256 + lane * 4));
                const float4 t = make_float4(t4.x, t4.y, t4.z, t4.w);  // read once: non-temporal (128 -> 119 us)
                mv[st][0] = t.x; mv[st][1] = t.y; mv[st][2] = t.z; mv[st][3] = t.w;
            }
        } else {
#pragma unroll
            for (int st = 0; st < STEPS; st++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int k = st * 256 + lane * 4 + q;
                    mv[st][q] = k < cnt ? mrow[k] : 0.f;  // columns past the slab contribute exactly 0
                }
        }
#pragma unroll
        for (int st = 0; st < STEPS; st++) {
            const int k = st * 256 + lane * 4;
            const float4 xs = X4[k >> 2], ys = Y4[k >> 2], zs = Z4[k >> 2];
            const float px[4] = {xs.x, xs.y, xs.z, xs.w};
            const float py[4] = {ys.x, ys.y, ys.z, ys.w};
            const float pz[4] = {zs.x, zs.y, zs.z, zs.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                // grad1 uses (p1 - p2) (approxmatch.cu:281-284); grad2 the negated vector (:240-246)
                const float dx = px[q] - x2, dy = py[q] - y2, dz = pz[q] - z2;
                const float f = mv[st][q] * __builtin_amdgcn_rsqf(__builtin_fmaxf(sq3(dx, dy, dz), 1e-20f));
                const float tx = dx * f, ty = dy * f, tz = dz * f;
                g1[st][q][0] += tx;
                g1[st][q][1] += ty;
                g1[st][q][2] += tz;
                rx -= tx;
                ry -= ty;
                rz -= tz;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            rx += __shfl_down(rx, off, 64);
            ry += __shfl_down(ry, off, 64);
            rz += __shfl_down(rz, off, 64);
        }
        if (lane == 0) {
            float *dst = part2 + (((size_t)smp * gridDim.y + slab) * m + row) * 3;
            const float sc = scale2 ? scale2[smp] : 1.0f;
            dst[0] = scale2 ? rx * sc : rx;
            dst[1] = scale2 ? ry * sc : ry;
            dst[2] = scale2 ? rz * sc : rz;
        }
    }
    // column partials: waves 1, 2, 3 hand their sums to wave 0 one after the other (fixed order)
    float *red = lds_p;
    for (int src = 1; src < 4; src++) {
        __syncthreads();
        if (w == src) {
#pragma unroll
            for (int st = 0; st < STEPS; st++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int c = 0; c < 3; c++) red[((st * 4 + q) * 3 + c) * 64 + lane] = g1[st][q][c];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int st = 0; st < STEPS; st++)
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int c = 0; c < 3; c++) g1[st][q][c] += red[((st * 4 + q) * 3 + c) * 64 + lane];
        }
    }
    if (w == 0) {
        float *dst = part1 + (((size_t)smp * row_tiles + rt) * n + c0) * 3;
#pragma unroll
        for (int st = 0; st < STEPS; st++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = st * 256 + lane * 4 + q;
                if (k < cnt) {
#pragma unroll
                    for (int c = 0; c < 3; c++) dst[(size_t)k * 3 + c] = g1[st][q][c];
                }
            }
    }
}

// grad1[b][i] = sum_s part[b][s][i]  (i over n*3), fixed order.
__global__ __launch_bounds__(256) void reduce_splits_kernel(int rs, size_t per_sample, const float *__restrict__ part,
                                                             const float *__restrict__ scale, float *__restrict__ out) {
    const int smp = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_sample) return;
    const float *p = part + (size_t)smp * rs * per_sample + i;
    float s = p[0];
    for (int t = 1; t < rs; t++) s += p[t * per_sample];
    out[(size_t)smp * per_sample + i] = scale ? s * scale[smp] : s;  // optional upstream gradient (match_cost.py:41-42)
}

}  // namespace

void pcc::launch_reduce_rows(int b, int parts, const float *part, float *out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(b), dim3(256), 0, st, parts, part, out);
}

extern "C" {

int pcc_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *out,
                  pcc_stream_t stream) {
    pcc::clear_error();
    if (int rc = check_sizes("matchcost", b, n, m)) return rc;
    if (b == 0) return PCC_OK;
    if (!out) return pcc::invalid("matchcost: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || m == 0) return zero_fill_empty(b, n, m, out, nullptr, nullptr, st, "matchcost: memset failed");
    if (!xyz1 || !xyz2 || !match) return pcc::invalid("matchcost: null pointer");
    const int tiles = pcc::ceil_div(m, kRowRT);
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc((size_t)b * tiles * sizeof(float), "workspace allocation failed")) return rc;
    float *part = static_cast<float *>(ws.p);
    const bool vec = (n % 4 == 0) && aligned16(match);
    {
        pcc::ProfScope prof("am_row_kernel<cost>", st);
        if (vec) hipLaunchKernelGGL((am_row_kernel<true>), dim3(tiles, b), dim3(256), 0, st, n, m, xyz1, xyz2, match, part);
        else hipLaunchKernelGGL((am_row_kernel<false>), dim3(tiles, b), dim3(256), 0, st, n, m, xyz1, xyz2, match, part);
    }
    if (int rc = pcc::check_launch("matchcost")) return rc;
    pcc::launch_reduce_rows(b, tiles, part, out, st);
    return pcc::check_launch("matchcost(reduce)");
}

void matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *out,
               pcc_stream_t stream) {
    (void)pcc_matchcost(b, n, m, xyz1, xyz2, match, out, stream);
}

int pcc_matchcostgrad_scaled(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                             const float *grad_cost, float *grad1, float *grad2, pcc_stream_t stream) {
    pcc::clear_error();
    if (int rc = check_sizes("matchcostgrad", b, n, m)) return rc;
    if (b == 0) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || m == 0) return zero_fill_empty(b, n, m, nullptr, grad1, grad2, st, "matchcostgrad: memset failed");
    if (!xyz1 || !xyz2 || !match || !grad1 || !grad2) return pcc::invalid("matchcostgrad: null pointer");
    const bool vec = (n % 4 == 0) && aligned16(match);
    const int row_tiles = pcc::ceil_div(m, kGradRT), slabs = pcc::ceil_div(n, kGradSlab);
    pcc::WsBlock ws(st);
    const size_t p1_elems = (size_t)b * row_tiles * n * 3, p2_elems = slabs > 1 ? (size_t)b * slabs * m * 3 : 0;
    if (int rc = ws.alloc((p1_elems + p2_elems) * sizeof(float), "workspace allocation failed")) return rc;
    float *part1 = static_cast<float *>(ws.p);
    float *part2 = slabs > 1 ? part1 + p1_elems : grad2;  // a single slab writes grad2 directly
    {
        pcc::ProfScope prof("am_grad_fused_kernel", st);
        const dim3 grid(row_tiles, slabs, b);
        const float *sc2 = slabs > 1 ? nullptr : grad_cost;
        if (vec) hipLaunchKernelGGL((am_grad_fused_kernel<true>), grid, dim3(256), 0, st, n, m, row_tiles, xyz1, xyz2, match, part1, part2, sc2);
        else hipLaunchKernelGGL((am_grad_fused_kernel<false>), grid, dim3(256), 0, st, n, m, row_tiles, xyz1, xyz2, match, part1, part2, sc2);
    }
    if (int rc = pcc::check_launch("matchcostgrad(fused)")) return rc;
    const size_t per1 = (size_t)n * 3, per2 = (size_t)m * 3;
    hipLaunchKernelGGL(reduce_splits_kernel, dim3((unsigned)((per1 + 255) / 256), b), dim3(256), 0, st, row_tiles, per1, part1, grad_cost, grad1);
    if (slabs > 1)
        hipLaunchKernelGGL(reduce_splits_kernel, dim3((unsigned)((per2 + 255) / 256), b), dim3(256), 0, st, slabs, per2, part2, grad_cost, grad2);
    return pcc::check_launch("matchcostgrad(reduce)");
}

int pcc_matchcostgrad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *grad1,
                      float *grad2, pcc_stream_t stream) {
    return pcc_matchcostgrad_scaled(b, n, m, xyz1, xyz2, match, nullptr, grad1, grad2, stream);
}

void matchcostgrad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *grad1,
                   float *grad2, pcc_stream_t stream) {
    (void)pcc_matchcostgrad(b, n, m, xyz1, xyz2, match, grad1, grad2, stream);
}

}  // extern "C"
