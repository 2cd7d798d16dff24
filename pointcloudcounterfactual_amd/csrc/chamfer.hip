// Chamfer nearest-neighbour forward / backward for gfx950 (MI355X), wave64.
//
// Replaces the reference's NmDistanceKernel / NmDistanceGradKernel and their launchers
// (external/pytorch_structural_losses/src/nndistance.cu:2-154).  This is not a translation of that
// kernel: the reference gives every thread one query and a 512-point shared tile, launches the
// two directions separately on 32x16 blocks and scatters gradients with 12 global float atomics
// per point.  Here:
//   * forward: ONE launch covers both directions.  A workgroup owns 64*R queries of one sample
//     (R per lane, in registers) and the whole candidate cloud of that sample sits in LDS as SoA
//     x|y|z; its S waves scan disjoint candidate ranges with broadcast ds_read_b128, 8 candidates
//     per step.  The running minimum is kept with v_min3_f32 per 8-candidate group (0.5 VALU op
//     per pair) and only the winning GROUP is tracked; the exact argmin inside that group is
//     recovered by one 8-candidate rescan at the end.  That is 6.9 VALU ops per pair instead of
//     the 9 of compare+2 selects, on a path whose roofline is the f32 VALU rate.
//   * tie rule and numerics are the oracle's: lowest index wins, d2 = fmaf(dz,dz,fmaf(dx,dx,dy*dy))
//     on differences, so indices and distances are bit-exact against oracle/structural_oracle.c.
//   * backward: workgroups own destination ranges of both gradients in LDS, write the direct term with
//     plain stores and fold in the scattered terms with ds_add_f32, then store once, coalesced --
//     no memset, no global atomics.
#include "pcc_common.hpp"

namespace {

using pcc::kWave;
using pcc::sq3;

constexpr int kGroup = 8;  // candidates per inner step (two float4 per coordinate)

template <int R, int S, int CH>
__global__ __launch_bounds__(64 * S) void nn_fwd_kernel(int b, int n, const float *__restrict__ xyz, int m,
                                                         const float *__restrict__ xyz2,
                                                         float *__restrict__ res1, int *__restrict__ idx1,
                                                         float *__restrict__ res2, int *__restrict__ idx2,
                                                         int tiles_n, int tiles_m) {
    constexpr int T = 64 * S;
    constexpr int TQ = 64 * R;
    static_assert(CH % (kGroup * 4) == 0, "chunk must hold whole float4 groups");
    __shared__ __attribute__((aligned(16))) float lds_c[3 * CH];  // x[CH] | y[CH] | z[CH]
    __shared__ float red_best[S][TQ];
    __shared__ int red_idx[S][TQ];
    __shared__ float run_best[TQ];
    __shared__ int run_idx[TQ];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // Which direction / sample / query tile is this workgroup?  (wave-uniform)
    // XCD affinity (cdna_hip_programming.md T1): blocks with equal blockIdx % 8 share an XCD and its L2.  Every workgroup
    // of a (direction, sample) scans the same candidate cloud, so the blocks of one residue class get a contiguous run of
    // logical ids (bijective): a cloud crosses the fabric once per launch instead of once per XCD (a pure speed choice).
    int bid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int dir0 = b * tiles_n;
    const float *Q, *C;
    float *out_d;
    int *out_i;
    int nq, nc, tiles;
    if (bid < dir0) {
        Q = xyz; C = xyz2; nq = n; nc = m; tiles = tiles_n; out_d = res1; out_i = idx1;
    } else {
        bid -= dir0;
        Q = xyz2; C = xyz; nq = m; nc = n; tiles = tiles_m; out_d = res2; out_i = idx2;
    }
    const int smp = bid / tiles;
    const int tile = bid - smp * tiles;
    Q += (size_t)smp * nq * 3;
    C += (size_t)smp * nc * 3;
    out_d += (size_t)smp * nq;
    out_i += (size_t)smp * nq;

    float qx[R], qy[R], qz[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        int q = tile * TQ + r * 64 + lane;
        q = q < nq ? q : nq - 1;
        qx[r] = Q[q * 3 + 0];
        qy[r] = Q[q * 3 + 1];
        qz[r] = Q[q * 3 + 2];
    }
    for (int e = tid; e < TQ; e += T) {
        run_best[e] = __builtin_inff();
        run_idx[e] = 0;
    }

    const float4 *X4 = reinterpret_cast<const float4 *>(lds_c);
    const float4 *Y4 = X4 + CH / 4;
    const float4 *Z4 = Y4 + CH / 4;

    for (int c0 = 0; c0 < nc; c0 += CH) {
        const int cnt = min(CH, nc - c0);
        const int ngroups = (cnt + kGroup - 1) / kGroup;
        __syncthreads();  // previous chunk fully consumed (and run_* initialised)
        // Stage AoS global -> SoA LDS; pad the last group with +inf so it can never win.
        const float *src = C + (size_t)c0 * 3;
        for (int i = tid; i < cnt * 3; i += T) {
            float v = src[i];
            int p = i / 3;
            int c = i - p * 3;
            lds_c[c * CH + p] = v;
        }
        for (int i = cnt + tid; i < ngroups * kGroup; i += T) {
            lds_c[i] = __builtin_inff();
            lds_c[CH + i] = __builtin_inff();
            lds_c[2 * CH + i] = __builtin_inff();
        }
        __syncthreads();

        const int gs = (ngroups + S - 1) / S;
        const int g_begin = w * gs;
        const int g_end = min(g_begin + gs, ngroups);

        float cb[R];
        int cg[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            cb[r] = __builtin_inff();
            cg[r] = min(g_begin, ngroups - 1);
        }
        for (int g = g_begin; g < g_end; g++) {
            const float4 xa = X4[2 * g], xb = X4[2 * g + 1];
            const float4 ya = Y4[2 * g], yb = Y4[2 * g + 1];
            const float4 za = Z4[2 * g], zb = Z4[2 * g + 1];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float d0 = sq3(xa.x - qx[r], ya.x - qy[r], za.x - qz[r]);
                const float d1 = sq3(xa.y - qx[r], ya.y - qy[r], za.y - qz[r]);
                const float d2 = sq3(xa.z - qx[r], ya.z - qy[r], za.z - qz[r]);
                const float d3 = sq3(xa.w - qx[r], ya.w - qy[r], za.w - qz[r]);
                const float d4 = sq3(xb.x - qx[r], yb.x - qy[r], zb.x - qz[r]);
                const float d5 = sq3(xb.y - qx[r], yb.y - qy[r], zb.y - qz[r]);
                const float d6 = sq3(xb.z - qx[r], yb.z - qy[r], zb.z - qz[r]);
                const float d7 = sq3(xb.w - qx[r], yb.w - qy[r], zb.w - qz[r]);
                float mn = __builtin_fminf(__builtin_fminf(d0, d1), d2);
                mn = __builtin_fminf(__builtin_fminf(mn, d3), d4);
                mn = __builtin_fminf(__builtin_fminf(mn, d5), d6);
                mn = __builtin_fminf(mn, d7);
                const bool lt = mn < cb[r];  // strict: the first group reaching the minimum keeps it
                cb[r] = lt ? mn : cb[r];
                cg[r] = lt ? g : cg[r];
            }
        }
        // Exact argmin inside the winning group: lowest candidate whose distance equals the minimum.
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int base = cg[r] * kGroup;
            int found = 0;
#pragma unroll
            for (int c = kGroup - 1; c >= 0; c--) {
                const float d = sq3(lds_c[base + c] - qx[r], lds_c[CH + base + c] - qy[r],
                                    lds_c[2 * CH + base + c] - qz[r]);
                found = (d == cb[r]) ? c : found;
            }
            red_best[w][r * 64 + lane] = cb[r];
            red_idx[w][r * 64 + lane] = c0 + base + found;
        }
        __syncthreads();
        // Merge the S candidate ranges in index order; strict '<' keeps the lowest index on ties.
        for (int e = tid; e < TQ; e += T) {
            float rb = run_best[e];
            int ri = run_idx[e];
#pragma unroll
            for (int s = 0; s < S; s++) {
                const float v = red_best[s][e];
                const bool lt = v < rb;
                ri = lt ? red_idx[s][e] : ri;
                rb = lt ? v : rb;
            }
            run_best[e] = rb;
            run_idx[e] = ri;
        }
    }
    __syncthreads();
    for (int e = tid; e < TQ; e += T) {
        const int q = tile * TQ + e;
        if (q < nq) {
            float rb = run_best[e];
            int ri = run_idx[e];
            // non-finite inputs as the reference treats them (nndistance.cu:26-28, `k == 0 || d < best`): candidate 0 is
            // always taken first, and nothing compares below NaN -- a NaN query point, or a NaN candidate 0, gives
            // dist = NaN with index 0; a NaN candidate elsewhere never wins.  The scan above ignores NaN (fminf, strict <).
            const float ux = Q[q * 3 + 0], uy = Q[q * 3 + 1], uz = Q[q * 3 + 2];
            const float d0 = sq3(C[0] - ux, C[1] - uy, C[2] - uz);
            if (d0 != d0 || !(rb < __builtin_inff())) {
                rb = d0;
                ri = 0;
            }
            // The reference's `k == 0` is local to its 512-candidate chunks (nndistance.cu:4-10,26): a NaN distance to
            // candidate 512*c (c >= 1) becomes that chunk's `best`, nothing in the chunk compares below it and the
            // cross-chunk merge (`result > best`, :116) drops the chunk -- candidates 512c .. 512c+511 are hidden from
            // this query.  Detected here with one distance per chunk head; such a query (a diverged input) is re-scanned
            // by the reference's own rule, one candidate at a time.
            bool quirk = false;
            for (int h = 512; h < nc; h += 512) {
                const float dh = sq3(C[h * 3 + 0] - ux, C[h * 3 + 1] - uy, C[h * 3 + 2] - uz);
                quirk |= (dh != dh);
            }
            if (quirk && d0 == d0) {
                for (int k2 = 0; k2 < nc; k2 += 512) {
                    const int end_k = min(nc, k2 + 512);
                    float best = 0.f;
                    int best_i = 0;
                    for (int k = k2; k < end_k; k++) {
                        const float d = sq3(C[k * 3 + 0] - ux, C[k * 3 + 1] - uy, C[k * 3 + 2] - uz);
                        if (k == k2 || d < best) {
                            best = d;
                            best_i = k;
                        }
                    }
                    if (k2 == 0 || rb > best) {
                        rb = best;
                        ri = best_i;
                    }
                }
            }
            out_d[q] = rb;
            out_i[q] = ri;
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------
// grad1[j] = 2 g1[j] (p1_j - p2[idx1[j]]) - sum_{k: idx2[k]=j} 2 g2[k] (p2_k - p1_j)   (and symmetric),
// i.e. exactly the four atomicAdd groups of nndistance.cu:140-145 applied in both directions.
// Each sample is cut into P destination ranges; a workgroup OWNS one range of grad1 and one of grad2,
// keeps them in LDS, writes the direct term with plain stores, then scans all nearest-neighbour
// indices of its sample and accumulates only the scattered terms that land in its range
// (ds_add_f32).  Outputs are complete and written once, coalesced: no memset, no global atomics, no
// workspace, and the LDS-atomic load is spread over b*P workgroups.
__global__ __launch_bounds__(256) void nn_bwd_range_kernel(int n, const float *__restrict__ xyz1, int m,
                                                            const float *__restrict__ xyz2,
                                                            const float *__restrict__ gd1,
                                                            const int *__restrict__ idx1,
                                                            const float *__restrict__ gd2,
                                                            const int *__restrict__ idx2,
                                                            float *__restrict__ grad1, float *__restrict__ grad2,
                                                            int P, const float *__restrict__ gloss, int mean, int gloss_stride,
                                                            const float *__restrict__ add1,
                                                            const float *__restrict__ add2,
                                                            const float *__restrict__ add_scale, int add_stride) {
    extern __shared__ __attribute__((aligned(16))) float acc[];
    // (a sample's P workgroups gather from the same two clouds: one XCD, see nn_fwd_kernel)
    const int lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int smp = lid / P, p = lid - smp * P;
    const int tid = threadIdx.x, T = 256;
    const int j0 = (int)((long long)n * p / P), j1 = (int)((long long)n * (p + 1) / P);
    const int k0 = (int)((long long)m * p / P), k1 = (int)((long long)m * (p + 1) / P);
    float *acc1 = acc;                   // [(j1-j0)*3]
    float *acc2 = acc + (j1 - j0) * 3;   // [(k1-k0)*3]
    const float *p1 = xyz1 + (size_t)smp * n * 3;
    const float *p2 = xyz2 + (size_t)smp * m * 3;
    const int *i1 = idx1 + (size_t)smp * n;
    const int *i2 = idx2 + (size_t)smp * m;
    // upstream gradient: per point (nn_distance backward) or, for the fused Chamfer loss, one scalar per sample
    // spread over the points (loss = sum or mean of the distances)
    const float *g1 = gloss ? nullptr : gd1 + (size_t)smp * n;
    const float *g2 = gloss ? nullptr : gd2 + (size_t)smp * m;
    const float gs = gloss ? gloss[(size_t)smp * gloss_stride] : 0.f;  // stride 0: one value for the batch (an expanded scalar)
    const float gs1 = mean ? gs / (float)n : gs, gs2 = mean ? gs / (float)m : gs;
    // direct terms (one owner per destination -> plain LDS stores)
    for (int j = j0 + tid; j < j1; j += T) {
        const int j2 = i1[j];
        const float g = (gloss ? gs1 : g1[j]) * 2;
#pragma unroll
        for (int c = 0; c < 3; c++) acc1[(j - j0) * 3 + c] = g * (p1[j * 3 + c] - p2[j2 * 3 + c]);
    }
    for (int k = k0 + tid; k < k1; k += T) {
        const int k2 = i2[k];
        const float g = (gloss ? gs2 : g2[k]) * 2;
#pragma unroll
        for (int c = 0; c < 3; c++) acc2[(k - k0) * 3 + c] = g * (p2[k * 3 + c] - p1[k2 * 3 + c]);
    }
    __syncthreads();
    // scattered terms landing in this workgroup's ranges
    for (int k = tid; k < m; k += T) {
        const int j = i2[k];
        if (j >= j0 && j < j1) {
            const float g = (gloss ? gs2 : g2[k]) * 2;
#pragma unroll
            for (int c = 0; c < 3; c++) atomicAdd(&acc1[(j - j0) * 3 + c], -(g * (p2[k * 3 + c] - p1[j * 3 + c])));
        }
    }
    for (int j = tid; j < n; j += T) {
        const int k = i1[j];
        if (k >= k0 && k < k1) {
            const float g = (gloss ? gs1 : g1[j]) * 2;
#pragma unroll
            for (int c = 0; c < 3; c++) atomicAdd(&acc2[(k - k0) * 3 + c], -(g * (p1[j * 3 + c] - p2[k * 3 + c])));
        }
    }
    __syncthreads();
    float *o1 = grad1 + ((size_t)smp * n + j0) * 3;
    float *o2 = grad2 + ((size_t)smp * m + k0) * 3;
    if (add1) {
        // a second loss on the same clouds (the reference's ChamferEMD reconstruction loss, metrics_and_losses.py:70-79):
        // its gradients, scaled by its upstream gradient, join here -- rounded product, then rounded sum, i.e. the bits
        // autograd's `grad * scale` followed by gradient accumulation would give
        const float as = add_scale ? add_scale[(size_t)smp * add_stride] : 1.0f;
        const float *a1 = add1 + ((size_t)smp * n + j0) * 3;
        const float *a2 = add2 + ((size_t)smp * m + k0) * 3;
        for (int i = tid; i < (j1 - j0) * 3; i += T) o1[i] = acc1[i] + a1[i] * as;
        for (int i = tid; i < (k1 - k0) * 3; i += T) o2[i] = acc2[i] + a2[i] * as;
        return;
    }
    for (int i = tid; i < (j1 - j0) * 3; i += T) o1[i] = acc1[i];
    for (int i = tid; i < (k1 - k0) * 3; i += T) o2[i] = acc2[i];
}

// loss[b] = sum_j dist1[b,j] (/ n) + sum_k dist2[b,k] (/ m): the reduction of the Chamfer loss
// (pykeops_chamfer: mean, metrics_and_losses.py:38-41; torch_chamfer: sum, :46-47), one workgroup per sample,
// fixed-order tree (deterministic).
__global__ __launch_bounds__(256) void chamfer_reduce_kernel(int n, int m, const float *__restrict__ dist1,
                                                              const float *__restrict__ dist2, int mean,
                                                              float *__restrict__ loss) {
    __shared__ float red[2][256];
    const int smp = blockIdx.x, tid = threadIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < n; i += 256) s1 += dist1[(size_t)smp * n + i];
    for (int i = tid; i < m; i += 256) s2 += dist2[(size_t)smp * m + i];
    red[0][tid] = s1;
    red[1][tid] = s2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) loss[smp] = mean ? red[1][0] / (float)m + red[0][0] / (float)n : red[0][0] + red[1][0];
}

int launch_bwd(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1, const int *idx1,
               const float *grad_dist2, const int *idx2, const float *gloss, int mean, int gloss_stride,
               float *grad_xyz1, float *grad_xyz2, hipStream_t st, const float *add1 = nullptr,
               const float *add2 = nullptr, const float *add_scale = nullptr, int add_stride = 1) {
    // P destination ranges per sample: ~512 workgroups on the chip, each range pair <= 48 KiB of LDS.
    long long P = std::max<long long>(1, pcc::ceil_div(512, b));
    P = std::min<long long>(P, std::max(1, std::min(n, m) / 64));
    const long long lds_min = ((long long)n + m) * 12 / (48 * 1024) + 1;
    P = std::max(P, lds_min);
    if (P * b > 0x7fffffffLL) return pcc::invalid("nndistancegrad: clouds too large");
    const size_t lds = ((size_t)pcc::ceil_div(n, (int)P) + pcc::ceil_div(m, (int)P) + 2) * 3 * sizeof(float);
    {
        pcc::ProfScope prof("nn_bwd_range_kernel", st);
        hipLaunchKernelGGL(nn_bwd_range_kernel, dim3((unsigned)(P * b)), dim3(256), lds, st, n, xyz1, m, xyz2,
                           grad_dist1, idx1, grad_dist2, idx2, grad_xyz1, grad_xyz2, (int)P, gloss, mean, gloss_stride,
                           add1, add2, add_scale, add_stride);
    }
    return pcc::check_launch("nndistancegrad");
}

template <int R, int S>
int launch_fwd(int b, int n, const float *xyz, int m, const float *xyz2, float *res1, int *idx1, float *res2,
               int *idx2, hipStream_t st) {
    constexpr int CH = 2048;
    const int tiles_n = pcc::ceil_div(n, 64 * R), tiles_m = pcc::ceil_div(m, 64 * R);
    const long long grid = (long long)b * (tiles_n + tiles_m);
    if (grid > 0x7fffffffLL) return pcc::invalid("nndistance: grid too large");
    {
        pcc::ProfScope prof("nn_fwd_kernel", st);
        hipLaunchKernelGGL((nn_fwd_kernel<R, S, CH>), dim3((unsigned)grid), dim3(64 * S), 0, st, b, n, xyz, m, xyz2,
                           res1, idx1, res2, idx2, tiles_n, tiles_m);
    }
    return pcc::check_launch("nndistance");
}

}  // namespace

extern "C" {

int pcc_nndistance(int b, int n, const float *xyz, int m, const float *xyz2, float *result, int *result_i,
                   float *result2, int *result2_i, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0) return pcc::invalid("nndistance: negative size");
    if (b == 0 || (n == 0 && m == 0)) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("nndistance: one cloud is empty (reference leaves outputs undefined)");
    if (!xyz || !xyz2 || !result || !result_i || !result2 || !result2_i) return pcc::invalid("nndistance: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // Queries per lane (R) x candidate split (S): fill 256 CUs with >= 2 waves per SIMD first, then
    // spend registers on R (each LDS broadcast read is amortised over R queries).
    // (measured at B=32, N=2048: 4 queries per lane x 4 waves is the fastest of {1,2,4,8} x {4,8})
    const long long queries = (long long)b * ((long long)n + m);
    if (queries >= 256LL * 64 * 8) return launch_fwd<4, 4>(b, n, xyz, m, xyz2, result, result_i, result2, result2_i, st);
    if (queries >= 256LL * 64 * 2) return launch_fwd<2, 4>(b, n, xyz, m, xyz2, result, result_i, result2, result2_i, st);
    return launch_fwd<1, 4>(b, n, xyz, m, xyz2, result, result_i, result2, result2_i, st);
}

void nndistance(int b, int n, const float *xyz, int m, const float *xyz2, float *result, int *result_i,
                float *result2, int *result2_i, pcc_stream_t stream) {
    (void)pcc_nndistance(b, n, xyz, m, xyz2, result, result_i, result2, result2_i, stream);
}

int pcc_nndistancegrad(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                       const int *idx1, const float *grad_dist2, const int *idx2, float *grad_xyz1,
                       float *grad_xyz2, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0) return pcc::invalid("nndistancegrad: negative size");
    if (b == 0 || (n == 0 && m == 0)) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("nndistancegrad: one cloud is empty");
    if (!xyz1 || !xyz2 || !grad_dist1 || !idx1 || !grad_dist2 || !idx2 || !grad_xyz1 || !grad_xyz2)
        return pcc::invalid("nndistancegrad: null pointer");
    return launch_bwd(b, n, xyz1, m, xyz2, grad_dist1, idx1, grad_dist2, idx2, nullptr, 0, 1, grad_xyz1, grad_xyz2,
                      static_cast<hipStream_t>(stream));
}

int pcc_chamfer_loss(int b, int n, const float *xyz1, int m, const float *xyz2, int mean, float *loss, float *dist1,
                     int *idx1, float *dist2, int *idx2, pcc_stream_t stream) {
    if (int rc = pcc_nndistance(b, n, xyz1, m, xyz2, dist1, idx1, dist2, idx2, stream)) return rc;
    if (b == 0) return PCC_OK;
    if (!loss) return pcc::invalid("chamfer_loss: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(chamfer_reduce_kernel, dim3((unsigned)b), dim3(256), 0, st, n, m, dist1, dist2, mean, loss);
    return pcc::check_launch("chamfer_loss(reduce)");
}

int pcc_chamfer_loss_grad(int b, int n, const float *xyz1, int m, const float *xyz2, const int *idx1, const int *idx2,
                          const float *grad_loss, int grad_loss_stride, int mean, float *grad_xyz1, float *grad_xyz2,
                          pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0) return pcc::invalid("chamfer_loss_grad: negative size");
    if (b == 0 || (n == 0 && m == 0)) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("chamfer_loss_grad: one cloud is empty");
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !grad_loss || !grad_xyz1 || !grad_xyz2)
        return pcc::invalid("chamfer_loss_grad: null pointer");
    if (grad_loss_stride != 0 && grad_loss_stride != 1) return pcc::invalid("chamfer_loss_grad: grad_loss stride must be 0 or 1");
    return launch_bwd(b, n, xyz1, m, xyz2, nullptr, idx1, nullptr, idx2, grad_loss, mean, grad_loss_stride, grad_xyz1, grad_xyz2,
                      static_cast<hipStream_t>(stream));
}

// Forward of the reference's ChamferEMD reconstruction loss (metrics_and_losses.py:70-79) in one call.  The two losses
// work on the same pair of clouds, and the approximate EMD starts by Hilbert-sorting both: the nearest-neighbour search
// runs on those sorted clouds with box culling (nn_sorted_kernel, nn_sorted.hip) instead of the exhaustive scan --
// same indices, same distances, bit for bit (tests/test_gpu_structural.py).
// (Measured and rejected: the exhaustive search on a side stream "in the shadow" of the EMD's launch chain -- at any
// starting pass, with or without raised wave priority for the chain -- never beat the serial order: the chain's kernels
// are bound by the vector and LDS pipes, not idle.)
int pcc_chamfer_emd(int b, int n, const float *xyz1, int m, const float *xyz2, int mean, float *chamfer_loss,
                    float *dist1, int *idx1, float *dist2, int *idx2, float *emd_cost, float *emd_grad1,
                    float *emd_grad2, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0) return pcc::invalid("chamfer_emd: negative size");
    if (b == 0) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("chamfer_emd: one cloud is empty");
    if ((long long)n * 3 > 0x7fffffffLL || (long long)m * 3 > 0x7fffffffLL) return pcc::invalid("chamfer_emd: bad size");
    if (b > 65535) return pcc::invalid("chamfer_emd: batch too large");  // the match_cost grids carry the batch in y
    if (!xyz1 || !xyz2 || !chamfer_loss || !dist1 || !idx1 || !dist2 || !idx2 || !emd_cost)
        return pcc::invalid("chamfer_emd: null pointer");
    if ((emd_grad1 == nullptr) != (emd_grad2 == nullptr)) return pcc::invalid("chamfer_emd: emd_grad1 and emd_grad2 go together");
    const pcc::ChamferOut ch{mean, chamfer_loss, dist1, dist2, idx1, idx2};
    return pcc::match_cost_with_chamfer(b, n, m, xyz1, xyz2, emd_cost, emd_grad1, emd_grad2,
                                        static_cast<hipStream_t>(stream), ch);
}

int pcc_chamfer_emd_grad(int b, int n, const float *xyz1, int m, const float *xyz2, const int *idx1, const int *idx2,
                         const float *grad_chamfer, int grad_chamfer_stride, int mean, const float *emd_grad1,
                         const float *emd_grad2, const float *grad_emd, int grad_emd_stride, float *grad_xyz1,
                         float *grad_xyz2, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0) return pcc::invalid("chamfer_emd_grad: negative size");
    if (b == 0 || (n == 0 && m == 0)) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("chamfer_emd_grad: one cloud is empty");
    if (!xyz1 || !xyz2 || !idx1 || !idx2 || !grad_chamfer || !emd_grad1 || !emd_grad2 || !grad_xyz1 || !grad_xyz2)
        return pcc::invalid("chamfer_emd_grad: null pointer");
    if ((grad_chamfer_stride != 0 && grad_chamfer_stride != 1) || (grad_emd_stride != 0 && grad_emd_stride != 1))
        return pcc::invalid("chamfer_emd_grad: gradient strides must be 0 or 1");
    return launch_bwd(b, n, xyz1, m, xyz2, nullptr, idx1, nullptr, idx2, grad_chamfer, mean, grad_chamfer_stride, grad_xyz1,
                      grad_xyz2, static_cast<hipStream_t>(stream), emd_grad1, emd_grad2, grad_emd, grad_emd_stride);
}

void nndistancegrad(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                    const int *idx1, const float *grad_dist2, const int *idx2, float *grad_xyz1, float *grad_xyz2,
                    pcc_stream_t stream) {
    (void)pcc_nndistancegrad(b, n, xyz1, m, xyz2, grad_dist1, idx1, grad_dist2, idx2, grad_xyz1, grad_xyz2, stream);
}

}  // extern "C"
