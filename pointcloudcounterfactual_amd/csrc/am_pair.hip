// Implicit match for gfx950 (MI355X), wave64: am_pair_kernel (f32-VALU / transcendental bound), pair_finish_kernel.
// ---------------------------------------------------------------------------------------------------
// Implicit match ("pair" kernel): what the Python-level match_cost needs is cost[b] and, when the clouds require
// gradients, grad1 / grad2 -- never the 512 MiB match tensor itself (reference match_cost.py:25-27,39-42 keeps it on
// ctx only to feed MatchCostGrad, and the gradient treats match as a constant).  This kernel evaluates every match
// element in registers exactly as am_materialise_kernel does (same level order, same rounding) and feeds it straight
// into the cost sum (approxmatch.cu:207-208) and both gradient sums (:239-246, :277-285): no store, no re-read.
// It runs in the Hilbert-sorted index space of the phase kernels, which buys two exact skips the materialising path
// cannot have (match is laid out in the caller's order there):
//   * a level whose exp2(c_i d2) underflows to 0 for every pair (row point, 64Q-column box) is skipped
//     (wave-uniform; the same test as V_CULL, applied to all levels);
//   * a row whose live levels are all skipped for this column box contributes exactly 0: no distance, no sqrt.
// Mapping: workgroup = kPairRT rows (set2 points, sorted) x 64Q columns (set1 points, sorted); a lane owns Q
// consecutive columns (coordinates, the nine ratioL values and the column sums stay in registers), the 4 waves deal
// the rows round-robin, row data is broadcast from LDS.  Row sums: per-lane partials are parked in LDS and folded
// eight rows at a time (48 lanes x 32 sequential adds + one shuffle), so the VALU never runs a 64-lane butterfly per
// row.  All partials are combined in a fixed order by the second-stage kernels: deterministic.
// ---------------------------------------------------------------------------------------------------
#include "approxmatch.hpp"
#include "wave_ops.hpp"

#include <algorithm>

namespace {

using pcc::sq3;

constexpr int kPairRB = 8;    // rows per row-sum fold
constexpr int kPairPad = 65;  // stash row pitch (floats): lanes of one fold hit distinct banks

struct PairArgs {
    int n, m, n4, m4;
    const float *soa1, *soa2;   // [b][3][n4] / [b][3][m4] sorted coordinates
    const float *lv;            // [b][9][n4 + m4] sorted level rows: ratioL | ratioR
    LevelConsts lc;
    float cut2[kLevels];        // a level is exactly 0 beyond this squared distance
    float *cost_part;           // [b][gridDim.y * gridDim.x]
    float *part1;               // [b][row_tiles][n4][3]   column sums (grad1, sorted space)
    float *part2;               // [b][col_blocks][m4][3]  row sums    (grad2, sorted space)
    int col_blocks, row_tiles, bc;  // 1-D grid of col_blocks * row_tiles * bc workgroups (see the kernel)
};

template <int Q, bool GRAD>
__global__ __launch_bounds__(256) void am_pair_kernel(PairArgs a) {
    __shared__ float4 lds_l[kPairRT][3];  // (x,y,z,rr0) (rr1..rr4) (rr5..rr8)
    __shared__ int lds_mask[kPairRT];     // bit i: level i contributes to this row segment
    __shared__ float stash[GRAD ? 4 * kPairRB * 3 * kPairPad : 4];
    __shared__ float lds_red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Dispatch order = work order.  A workgroup's duration goes from ~0 (every row of the tile masked out for this column
    // box) to the full 128 x 256 pairs on all live levels, and the heavy ones are the (row tile, column block) pairs that
    // are CLOSE in space -- close along the two Hilbert orders.  In (x, y, z) grid order the last workgroups dispatched
    // were as likely heavy as light and the chip idled 22 % of the kernel behind them (SQ_BUSY_CU_CYCLES).  The 1-D grid
    // is read shift-major instead: for every shift 0, +1, -1, +2, ... of the row tile against the column block's own
    // position along the curve, every column block, every sample -- near pairs first, far (short) ones last.
    const int cbn = a.col_blocks, rtn = a.row_tiles;
    const int item = (int)blockIdx.x / a.bc, smp = (int)blockIdx.x - item * a.bc;
    const int shift_k = item / cbn, cblk = item - shift_k * cbn;
    const int base_r = (int)(((long long)(2 * cblk + 1) * rtn) / (2 * cbn));
    const int shift = ((shift_k + 1) >> 1) * ((shift_k & 1) ? 1 : -1);  // 0, +1, -1, +2, ... : a complete residue system mod rtn
    const int rtile = ((base_r + shift) % rtn + rtn) % rtn;
    const int l0 = rtile * kPairRT;
    const int kb = cblk * 64 * Q;
    const int k0 = kb + lane * Q;
    const size_t nm4 = (size_t)a.n4 + a.m4;
    const float *lvb = a.lv + (size_t)smp * kLevels * nm4;
    const float *s1 = a.soa1 + (size_t)smp * 3 * a.n4;
    const float *s2 = a.soa2 + (size_t)smp * 3 * a.m4;
    const int lcnt = min(kPairRT, a.m - l0);

    // this thread's row (the first lcnt threads finish one row each once the column box is known)
    float rowx = 0.f, rowy = 0.f, rowz = 0.f, rowr[kLevels];
#pragma unroll
    for (int i = 0; i < kLevels; i++) rowr[i] = 0.f;
    if (tid < lcnt) {
        const int l = l0 + tid;
        rowx = s2[l];
        rowy = s2[a.m4 + l];
        rowz = s2[2 * a.m4 + l];
#pragma unroll
        for (int i = 0; i < kLevels; i++) rowr[i] = lvb[(size_t)i * nm4 + a.n4 + l];
    }
    float x1[Q], y1[Q], z1[Q], rl[kLevels][Q];
    float blo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float bhi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const bool real = k0 + q < a.n;
        const int k = real ? k0 + q : a.n - 1;
        x1[q] = s1[k];
        y1[q] = s1[a.n4 + k];
        z1[q] = s1[2 * a.n4 + k];
#pragma unroll
        for (int i = 0; i < kLevels; i++) rl[i][q] = real ? lvb[(size_t)i * nm4 + k] : 0.f;  // a padded column weighs 0
        blo[0] = fminf(blo[0], x1[q]); bhi[0] = fmaxf(bhi[0], x1[q]);
        blo[1] = fminf(blo[1], y1[q]); bhi[1] = fmaxf(bhi[1], y1[q]);
        blo[2] = fminf(blo[2], z1[q]); bhi[2] = fmaxf(bhi[2], z1[q]);
    }
    // bounding box of the 64Q columns of this workgroup (every wave holds the same columns)
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            blo[c] = fminf(blo[c], __shfl_xor(blo[c], off, 64));
            bhi[c] = fmaxf(bhi[c], __shfl_xor(bhi[c], off, 64));
        }
    }
    if (tid < lcnt) {
        // level i adds exactly 0 to the whole row segment if ratioR_i == 0 (exhausted query point,
        // approxmatch.cu:108-109) or if every exponential underflows: every pair (row, column of the box) has
        // d2 >= bd2
        const float bx = fmaxf(fmaxf(blo[0] - rowx, rowx - bhi[0]), 0.f);
        const float by = fmaxf(fmaxf(blo[1] - rowy, rowy - bhi[1]), 0.f);
        const float bz = fmaxf(fmaxf(blo[2] - rowz, rowz - bhi[2]), 0.f);
        const float bd2 = bx * bx + by * by + bz * bz;
        int mask = 0;
#pragma unroll
        for (int i = 0; i < kLevels; i++) mask |= (rowr[i] != 0.f && !(bd2 > a.cut2[i])) ? (1 << i) : 0;
        lds_l[tid][0] = make_float4(rowx, rowy, rowz, rowr[0]);
        lds_l[tid][1] = make_float4(rowr[1], rowr[2], rowr[3], rowr[4]);
        lds_l[tid][2] = make_float4(rowr[5], rowr[6], rowr[7], rowr[8]);
        lds_mask[tid] = mask;
    }
    float g1[Q][3];
#pragma unroll
    for (int q = 0; q < Q; q++) g1[q][0] = g1[q][1] = g1[q][2] = 0.f;
    float csum = 0.f;
    float *my_stash = stash + (GRAD ? w * kPairRB * 3 * kPairPad : 0);
    __syncthreads();

    // wave w takes rows w, w+4, ...; kPairRB of them per fold
    for (int base = 0; base < lcnt; base += 4 * kPairRB) {
#pragma unroll 1
        for (int s = 0; s < kPairRB; s++) {
            const int li = base + 4 * s + w;
            float rx = 0.f, ry = 0.f, rz = 0.f;
            const int mask = li < lcnt ? __builtin_amdgcn_readfirstlane(lds_mask[li]) : 0;
            if (mask) {
                const float4 A = lds_l[li][0], B = lds_l[li][1], Cc = lds_l[li][2];
                const float rr[kLevels] = {A.w, B.x, B.y, B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w};
                float ex[Q], ey[Q], ez[Q], d[Q], acc[Q];
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    ex[q] = A.x - x1[q];  // p2 - p1 (approxmatch.cu:148-150)
                    ey[q] = A.y - y1[q];
                    ez[q] = A.z - z1[q];
                    d[q] = sq3(ex[q], ey[q], ez[q]);
                    acc[q] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < kLevels; i++) {
                    if (mask & (1 << i)) {
                        // w = exp(level d2) ratioL ratioR; match += w (approxmatch.cu:153-155): the product is added
                        // with one fma (the contraction a compiler applies to `match += a * b`); am_materialise_kernel
                        // rounds the product first -- the two differ by half an ulp of the product
#pragma unroll
                        for (int q = 0; q < Q; q++)
                            acc[q] = __builtin_fmaf(fast_exp2(a.lc.c[i] * d[q]) * rl[i][q], rr[i], acc[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    if (GRAD) {
                        // max(d2, 1e-20): d2 is never NaN, so the bare instruction (no canonicalising pre-pass)
                        float dm;
                        asm("v_max_f32 %0, %1, %2" : "=v"(dm) : "v"(d[q]), "v"(1e-20f));
                        const float f = acc[q] * __builtin_amdgcn_rsqf(dm);
                        // sqrt(d2) = d2 * rsqrt(d2): one transcendental serves both sums (d2 < 1e-20 moves the cost by < 1e-10)
                        csum = __builtin_fmaf(f, d[q], csum);
                        // t = (p2 - p1) match / |p1 - p2|: grad2 (rows) accumulates +t (approxmatch.cu:240-246), grad1
                        // (columns) the negated vector (:281-284)
                        g1[q][0] = __builtin_fmaf(-ex[q], f, g1[q][0]);
                        g1[q][1] = __builtin_fmaf(-ey[q], f, g1[q][1]);
                        g1[q][2] = __builtin_fmaf(-ez[q], f, g1[q][2]);
                        rx = __builtin_fmaf(ex[q], f, rx);
                        ry = __builtin_fmaf(ey[q], f, ry);
                        rz = __builtin_fmaf(ez[q], f, rz);
                    } else {
                        csum = __builtin_fmaf(acc[q], __builtin_amdgcn_sqrtf(d[q]), csum);
                    }
                }
            }
            if (GRAD) {
                my_stash[(s * 3 + 0) * kPairPad + lane] = rx;
                my_stash[(s * 3 + 1) * kPairPad + lane] = ry;
                my_stash[(s * 3 + 2) * kPairPad + lane] = rz;
            }
        }
        if (GRAD) {
            // fold the eight rows: lane (v, h) adds half h of vector v = (slot, component) in index order, the two
            // halves meet through one shuffle.  The stash is private to the wave: no workgroup barrier.
            const int v = lane % 24, h = lane / 24;
            float t = 0.f;
            __builtin_amdgcn_wave_barrier();  // LDS operations of one wave execute in order; keep the compiler to it
            if (lane < 48) {
                const float *src = my_stash + v * kPairPad + h * 32;
#pragma unroll 8
                for (int i = 0; i < 32; i++) t += src[i];
            }
            __builtin_amdgcn_wave_barrier();
            const float hi = __shfl(t, lane + 24, 64);
            const int sl = v / 3, c = v - sl * 3;
            const int li = base + 4 * sl + w;
            if (lane < 24 && li < lcnt)
                a.part2[(((size_t)smp * cbn + cblk) * a.m4 + (l0 + li)) * 3 + c] = t + hi;
        }
    }
    // cost partial of this workgroup
    csum = pcc::wave_sum_down(csum);
    if (lane == 0) lds_red[w] = csum;
    __syncthreads();
    if (tid == 0)
        a.cost_part[(size_t)smp * cbn * rtn + rtile * cbn + cblk] =
            ((lds_red[0] + lds_red[1]) + lds_red[2]) + lds_red[3];
    if (GRAD) {
        // column sums: waves 1..3 hand theirs to wave 0 one after the other (fixed order); the stash is free now
        static_assert(Q * 3 * 64 <= 4 * kPairRB * 3 * kPairPad, "column merge reuses the stash");
        for (int src = 1; src < 4; src++) {
            __syncthreads();
            if (w == src) {
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int c = 0; c < 3; c++) stash[(q * 3 + c) * 64 + lane] = g1[q][c];
            }
            __syncthreads();
            if (w == 0) {
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int c = 0; c < 3; c++) g1[q][c] += stash[(q * 3 + c) * 64 + lane];
            }
        }
        if (w == 0) {
            float *dst = a.part1 + (((size_t)smp * rtn + rtile) * a.n4) * 3;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                if (k0 + q < a.n) {
#pragma unroll
                    for (int c = 0; c < 3; c++) dst[(size_t)(k0 + q) * 3 + c] = g1[q][c];
                }
            }
        }
    }
}

// Second stage of the implicit path: partials are added in index order (deterministic) and the gradients carried from
// the sorted index space back to the caller's point order through `rank`.
// The three second-stage reductions of the implicit path in ONE launch (blockIdx.z: 0 = grad1, 1 = grad2, 2 = cost).
struct FinishArgs {
    int parts[3], npts[2], pitch[2];
    const float *part[3];
    const int *perm[2];   // sorted position -> caller's point index
    const float *scale;
    float *out[3];
    // the Chamfer half of a ChamferEMD call rides along (blockIdx.z == 3): loss[b] = sum / mean of the two distance rows
    const float *ch_d1, *ch_d2;
    float *ch_loss;
    int ch_n, ch_m, ch_mean;
    const int *flags;  // live-counter rows [b][kLiveRow] (slots kInfSlot, kInfSlot + 1), or null
};
__global__ __launch_bounds__(256) void pair_finish_kernel(FinishArgs f) {
    __shared__ float red[256];
    const int which = blockIdx.z, smp = blockIdx.y, tid = threadIdx.x;
    if (which == 3) {  // the same fixed-order tree as chamfer_reduce_kernel (chamfer.hip): the same bits
        if (blockIdx.x) return;
        __shared__ float red2[256];
        float s1 = 0.f, s2 = 0.f;
        // (eight loads in flight, added in the same order: one at a time this slice was a chain of n / 256 round trips, the
        // longest of the launch)
        auto strided_sum = [&](const float *d, int cnt) -> float {
            float acc = 0.f;
            for (int i0 = tid; i0 < cnt; i0 += 8 * 256) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = d[min(i0 + u * 256, cnt - 1)];
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (i0 + u * 256 < cnt) acc += v[u];
            }
            return acc;
        };
        s1 = strided_sum(f.ch_d1 + (size_t)smp * f.ch_n, f.ch_n);
        s2 = strided_sum(f.ch_d2 + (size_t)smp * f.ch_m, f.ch_m);
        red[tid] = s1;
        red2[tid] = s2;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) {
                red[tid] += red[tid + off];
                red2[tid] += red2[tid + off];
            }
            __syncthreads();
        }
        if (tid == 0) f.ch_loss[smp] = f.ch_mean ? red2[0] / (float)f.ch_m + red[0] / (float)f.ch_n : red[0] + red2[0];
        return;
    }
    // a sample with an infinite coordinate: NaN cost and gradients (see am_sort_kernel)
    // ... or whose resident fine-level passes did not complete (am_fine_persist_kernel: a sample barrier timed out)
    const bool poisoned = f.flags && (f.flags[(size_t)smp * kLiveRow + kInfSlot] | f.flags[(size_t)smp * kLiveRow + kInfSlot + 1] |
                                      f.flags[(size_t)smp * kLiveRow + kErrSlot]);
    if (which == 2) {  // cost[b] = sum of the workgroup partials, fixed order
        if (blockIdx.x) return;
        const int parts = f.parts[2];
        float s = 0.f;
        for (int i = tid; i < parts; i += 256) s += f.part[2][(size_t)smp * parts + i];
        red[tid] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
        if (tid == 0) f.out[2][smp] = poisoned ? __builtin_nanf("") : red[0];
        return;
    }
    if (!f.out[which]) return;
    // a thread owns component c of SORTED position s: the partial rows are read as straight coalesced streams (they
    // are the bulk: parts x npts x 12 bytes); only the 12-byte result is scattered to the caller's point order
    const int npts = f.npts[which], pitch = f.pitch[which], parts = f.parts[which];
    const int i = blockIdx.x * 256 + tid;
    if (i >= npts * 3) return;
    const int s = i / 3, c = i - s * 3;
    const float *p = f.part[which] + (size_t)smp * parts * pitch * 3 + i;
    const int pt = f.perm[which][(size_t)smp * npts + s];
    // the partials in the fixed order t = 0, 1, 2 ..., eight loads in flight (one at a time, the fold is a chain of
    // `parts` memory round trips: most of this kernel's time)
    const size_t stride = (size_t)pitch * 3;
    float acc = p[0];
    int t = 1;
    for (; t + 8 <= parts; t += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)(t + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u];
    }
    {
        float v[7];
#pragma unroll
        for (int u = 0; u < 7; u++) v[u] = p[(size_t)min(t + u, parts - 1) * stride];
#pragma unroll
        for (int u = 0; u < 7; u++)
            if (t + u < parts) acc += v[u];
    }
    f.out[which][((size_t)smp * npts + pt) * 3 + c] = poisoned ? __builtin_nanf("") : f.scale ? acc * f.scale[smp] : acc;
}

// cost[b] (and grad1 / grad2 when both are non-null) of the Python-level match_cost without materialising match.
template <int Q>
int launch_pair(const PairArgs &pa, dim3 grid, bool grad, hipStream_t st) {
    pcc::ProfScope prof(grad ? "am_pair_kernel<grad>" : "am_pair_kernel<cost>", st);
    if (grad) hipLaunchKernelGGL((am_pair_kernel<Q, true>), grid, dim3(256), 0, st, pa);
    else hipLaunchKernelGGL((am_pair_kernel<Q, false>), grid, dim3(256), 0, st, pa);
    return pcc::check_launch("match_cost(pair)");
}

}  // namespace

namespace pcc {

// pair + finish kernels of the samples [s0, s0 + bc) on `lst` (`v`: the workspace view at s0; grad_cost, cost, grad1, grad2
// and the Chamfer rows: those of sample 0)
int launch_pair_finish(const AmDims &L, const WsView &v, int s0, int bc, int col_blocks, int row_tiles, const float *grad_cost,
                       float *cost, float *grad1, float *grad2, const ChamferOut *chamfer, hipStream_t lst) {
    const size_t o = (size_t)s0;
    const int n = L.n, m = L.m;
    const bool grad = grad1 && grad2;
    const LevelConsts lc = make_levels();
    PairArgs pa{};
    pa.n = n; pa.m = m; pa.n4 = L.n4; pa.m4 = L.m4;
    pa.soa1 = v.soa1; pa.soa2 = v.soa2; pa.lv = v.lv;
    pa.lc = lc;
    for (int i = 0; i < kLevels; i++) pa.cut2[i] = zero_cut2(lc, i);
    pa.cost_part = v.pair_cost;
    pa.part1 = grad ? v.part1 : nullptr;
    pa.part2 = grad ? v.part2 : nullptr;
    pa.col_blocks = col_blocks; pa.row_tiles = row_tiles; pa.bc = bc;
    if ((long long)col_blocks * row_tiles * bc > 0x7fffffffLL) return pcc::invalid("match_cost: grid too large");
    const dim3 grid((unsigned)(col_blocks * row_tiles * bc));
    if (int rc = launch_pair<kPairQ>(pa, grid, grad, lst)) return rc;
    FinishArgs f{};
    f.parts[0] = row_tiles; f.parts[1] = col_blocks; f.parts[2] = col_blocks * row_tiles;
    f.npts[0] = n; f.npts[1] = m; f.pitch[0] = L.n4; f.pitch[1] = L.m4;
    f.part[0] = pa.part1; f.part[1] = pa.part2; f.part[2] = pa.cost_part;
    f.perm[0] = v.perm1; f.perm[1] = v.perm2;
    f.scale = grad_cost ? grad_cost + o : nullptr;
    f.out[0] = grad ? grad1 + o * n * 3 : nullptr;
    f.out[1] = grad ? grad2 + o * m * 3 : nullptr;
    f.out[2] = cost + o;
    f.flags = v.live_cnt;  // (written by this call's sort)
    if (chamfer) {
        f.ch_d1 = chamfer->dist1 + o * n; f.ch_d2 = chamfer->dist2 + o * m; f.ch_loss = chamfer->loss + o;
        f.ch_n = n; f.ch_m = m; f.ch_mean = chamfer->mean;
    }
    {
        pcc::ProfScope prof("pair_finish_kernel", lst);
        const int blocks = grad ? pcc::ceil_div(std::max(n, m) * 3, 256) : 1;
        hipLaunchKernelGGL(pair_finish_kernel, dim3(blocks, bc, chamfer ? 4 : 3), dim3(256), 0, lst, f);
    }
    return pcc::check_launch("match_cost(reduce)");
}
}  // namespace pcc
