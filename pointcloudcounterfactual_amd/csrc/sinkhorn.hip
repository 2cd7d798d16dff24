// Debiased Sinkhorn divergence between paired clouds (pcc_sinkhorn, include/pcc_structural.h), gfx950, wave64: T + 2
// rounds of all-pairs smoothed minima over up to four (row cloud, column cloud, column potential) scans
//   f: x against y with g     g: y against x with f     p: x against x with p     q: y against y with q
// all updated at once from the previous generation (two workspace buffers, every launch reads one and writes the other).
//
// One launch per round (sk_scan_kernel) covers every scan of every cloud.  A workgroup is 256 rows of one scan against one
// slice of its columns; a thread owns a row.  The column side -- xyz and the potential pre-scaled to the exponent's
// units, w_j = h_j (log2 e / eps) -- is staged through LDS in tiles of 256 float4, so every lane of a wave reads
// the same address.  Per pair: three differences, the squared norm (one product, two fmaf), one fmaf into the exponent
// a = w_j - C (log2 e / eps), one v_exp_f32.  A row keeps (ref, sum): sum = sum_j exp2(a_j - ref), ref = the largest a so
// far.  The columns go by in groups of 8 whose arguments sit in registers: ref is raised (and sum rescaled, one more
// exponential per group) only when a group's largest argument exceeds it, so the largest term is always subtracted, the
// loop costs one exponential per pair, and a row whose terms are all far below an early one cannot underflow to 0.
// SM = -(eps ln 2) (ref + log2(sum / |V|)): the weight 1 / |V| goes onto the sum, where it keeps the logarithm small at a
// high temperature (sum is about |V| there; log2 |V| added to ref and taken off again would cost an ulp of 10).  The final round (GRAD) also accumulates sum_j exp2(a_j - ref) (u_i - v_j).
//
// Column split: with few rows (a batch of one cloud at n = m = 2048 has 8192: 128 waves for 1024 SIMDs) the columns of a
// scan are cut into slices of `chunk` columns (split_for below: a function of n and m only, never of b) whose partial
// (ref, sum) pairs sk_merge_kernel merges in ascending slice order.  Without a split the scan kernel writes the new
// potential itself.  The final round always leaves partials (and the three weighted differences); sk_combine_kernel, one
// thread per point, merges them and forms pot_x = f* - p*, pot_y = g* - q* and the gradients; sk_cost_kernel, one workgroup
// per cloud, forms cost[b] by the halving tree.
// Nothing here uses an atomic or a device-wide barrier: every word depends on the cloud's own data, n, m and the schedule.
#include "approxmatch.hpp"

#include <algorithm>
#include <cmath>

#include "pcc_test_hooks.h"

namespace {

constexpr int kRows = 256;       // rows (threads) per workgroup
constexpr int kTile = 256;       // columns per LDS tile
constexpr int kGroup = 8;        // columns whose arguments are held in registers at once
constexpr int kMaxSplit = 16;    // column slices per scan at the most
constexpr int kFinishThreads = 1024;
static_assert(kGroup == 8 && kTile % kGroup == 0 && kTile == kRows, "a thread stages one column per tile");

struct Scan {
    int rows, cols;        // points on the row / column side
    int rows_y, cols_y;    // 1: that side is cloud y
    int row_off, col_off;  // offsets of the row / column potential inside a cloud's R words
    int nsplit, chunk;     // column slices (<= the allowance) and columns per slice (a multiple of kGroup)
    int blk0, nblk;        // this scan's workgroups: blk0 .. blk0 + nblk - 1 = (row block, slice)
    float inv_cols;        // the float32 nearest to 1 / cols
};

struct Round {
    Scan sc[4];
    int nscan, n, m;
    int R, S;             // potential words per cloud; slices per row in the partial arrays (the largest nsplit)
    const float *x, *y;
    const float *hin;     // [b, R] previous generation (null: the initialisation, zero potentials)
    float *hout;          // [b, R] next generation (scan kernel without a split, merge kernel)
    float2 *part;         // [b, R, S] (ref, sum)
    float *gpart;         // [b, R, S, 3] weighted differences of the final round
    float k, nhk;         // log2 e / eps, -0.5 log2 e / eps
    float eps_ln2;        // eps ln 2
    int average;          // h <- 0.5 (h + SM) (the T inner rounds) or h <- SM (the initialisation)
};

__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }

// The partials of potential word `word` of `cloud` sit at part[(cloud S + slice) R + word] (slice-major: the rows of a
// workgroup write, and the merging threads read, consecutive words), the weighted differences likewise times 3.
__device__ __forceinline__ size_t part_index(const Round &r, int cloud, int slice, int word) {
    return ((size_t)cloud * r.S + slice) * r.R + word;
}

// partials of one row, in ascending slice order: (M, tot) with sum_j exp2(a_j) = tot exp2(M); g (if asked for) = the
// weighted differences on the same reference
__device__ __forceinline__ void merge_row(const Round &r, int cloud, int word, int nsplit, float &M, float &tot, float (&g)[3], bool grad) {
    const float2 *p = r.part + part_index(r, cloud, 0, word);
    const size_t stride = (size_t)r.R;
    M = p[0].x;
    for (int s = 1; s < nsplit; s++) M = fmaxf(M, p[s * stride].x);
    tot = 0.f;
    g[0] = g[1] = g[2] = 0.f;
    for (int s = 0; s < nsplit; s++) {
        const float w = fast_exp2(p[s * stride].x - M);
        tot = __builtin_fmaf(p[s * stride].y, w, tot);
        if (grad) {
            const float *gp = r.gpart + part_index(r, cloud, s, word) * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) g[c] = __builtin_fmaf(gp[c], w, g[c]);
        }
    }
}

template <bool GRAD>
__global__ __launch_bounds__(kRows) void sk_scan_kernel(Round r) {
    __shared__ float4 tile[kTile];
    const int tid = threadIdx.x, cloud = blockIdx.y, bx = blockIdx.x;
    int si = 0;
    while (si + 1 < r.nscan && bx >= r.sc[si + 1].blk0) ++si;
    const Scan sc = r.sc[si];
    const int local = bx - sc.blk0, rb = local / sc.nsplit, sp = local % sc.nsplit;
    const int row = rb * kRows + tid;
    const bool live = row < sc.rows;
    const float *rowpts = (sc.rows_y ? r.y + (size_t)cloud * r.m * 3 : r.x + (size_t)cloud * r.n * 3);
    const float *colpts = (sc.cols_y ? r.y + (size_t)cloud * r.m * 3 : r.x + (size_t)cloud * r.n * 3);
    const float *colpot = r.hin ? r.hin + (size_t)cloud * r.R + sc.col_off : nullptr;
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
    if (live) u0 = rowpts[(size_t)row * 3], u1 = rowpts[(size_t)row * 3 + 1], u2 = rowpts[(size_t)row * 3 + 2];

    const int c0 = sp * sc.chunk, c1 = min(sc.cols, c0 + sc.chunk);
    float ref = -INFINITY, sum = 0.f, tsum = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;  // (tsum: the current tile's share of sum)
    (void)g0, (void)g1, (void)g2;
    for (int base = c0; base < c1; base += kTile) {
        __syncthreads();  // (the previous tile's readers are done)
        {
            const int j = base + tid;
            float4 v = make_float4(0.f, 0.f, 0.f, -INFINITY);  // a pad column: exp2(-inf - ref) = 0
            if (j < c1) {
                const float h = colpot ? colpot[j] : 0.f;
                v = make_float4(colpts[(size_t)j * 3], colpts[(size_t)j * 3 + 1], colpts[(size_t)j * 3 + 2],
                                h * r.k);
            }
            tile[tid] = v;
        }
        __syncthreads();
        const int cnt = min(kTile, c1 - base);
        for (int j = 0; j < cnt; j += kGroup) {  // (the tile is padded to a multiple of kGroup)
            float a[kGroup], d0[kGroup], d1[kGroup], d2[kGroup];
            float mx = -INFINITY;
#pragma unroll
            for (int q = 0; q < kGroup; q++) {
                const float4 v = tile[j + q];
                d0[q] = u0 - v.x, d1[q] = u1 - v.y, d2[q] = u2 - v.z;
                const float c2 = __builtin_fmaf(d2[q], d2[q], __builtin_fmaf(d1[q], d1[q], d0[q] * d0[q]));
                a[q] = __builtin_fmaf(c2, r.nhk, v.w);
                // Non-finite input, on purpose: fmaxf ignores a NaN argument, which then reaches sum through exp2 below; an
                // infinite coordinate gives a = -inf, a term of 0 in every other row, and in the point's own row ref stays
                // -inf and exp2(-inf - -inf) is NaN.  Either way the cloud's cost comes out non-finite, as the contract says.
                mx = fmaxf(mx, a[q]);
            }
            if (mx > ref) {
                const float s = fast_exp2(ref - mx);  // (ref = -inf: 0, and sum is 0)
                sum = sum * s, tsum = tsum * s;
                if constexpr (GRAD) g0 = g0 * s, g1 = g1 * s, g2 = g2 * s;
                ref = mx;
            }
            float e[kGroup];
#pragma unroll
            for (int q = 0; q < kGroup; q++) {
                e[q] = fast_exp2(a[q] - ref);
                if constexpr (GRAD) {
                    g0 = __builtin_fmaf(e[q], d0[q], g0), g1 = __builtin_fmaf(e[q], d1[q], g1), g2 = __builtin_fmaf(e[q], d2[q], g2);
                }
            }
            // a group's terms pairwise, the groups of a tile in order, the tiles in order: with thousands of columns one
            // running sum would lose sqrt(cols) roundings, which at a high temperature is the potential's whole error
            tsum = tsum + (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7])));
        }
        sum = sum + tsum, tsum = 0.f;
    }
    if (!live) return;
    const size_t word = (size_t)cloud * r.R + sc.row_off + row;
    if (!GRAD && sc.nsplit == 1 && r.hout) {
        const float sm = -r.eps_ln2 * (ref + fast_log2(sum * sc.inv_cols));
        r.hout[word] = r.average ? 0.5f * (r.hin[word] + sm) : sm;
        return;
    }
    const size_t slot = part_index(r, cloud, sp, sc.row_off + row);
    r.part[slot] = make_float2(ref, sum);
    if constexpr (GRAD) {
        float *gp = r.gpart + slot * 3;
        gp[0] = g0, gp[1] = g1, gp[2] = g2;
    }
}

// With a column split: the rows of every scan, one thread each; the new potential from the row's partials.  (A scan whose
// columns fit one slice wrote its potential in the scan kernel and left no partial.)
__global__ __launch_bounds__(256) void sk_merge_kernel(Round r) {
    const int cloud = blockIdx.y;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= r.R) return;
    int si = 0;
    while (si + 1 < r.nscan && w >= r.sc[si + 1].row_off) ++si;
    if (r.sc[si].nsplit == 1) return;
    const size_t word = (size_t)cloud * r.R + w;
    float M, tot, g[3];
    merge_row(r, cloud, w, r.sc[si].nsplit, M, tot, g, false);
    const float sm = -r.eps_ln2 * (M + fast_log2(tot * r.sc[si].inv_cols));
    r.hout[word] = r.average ? 0.5f * (r.hin[word] + sm) : sm;
}

// The contract's halving tree over e[0 .. count - 1] padded with +0 to L = the power of two >= count, by one workgroup
// of kFinishThreads: thread t < L / Q folds the Q = max(1, L / kFinishThreads) elements t + (L / Q) q in registers (the
// tree's first levels touch exactly those), the remaining levels run in LDS.  The result is returned to every thread.
template <int Q>
__device__ __forceinline__ float tree_fold(const float *e, int t, int stride, int count) {
    float v[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) v[q] = t + stride * q < count ? e[t + stride * q] : 0.f;
#pragma unroll
    for (int h = Q / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int i = 0; i < h; i++) v[i] = v[i] + v[i + h];
    }
    return v[0];
}

__device__ float halving_tree(const float *e, int count, float *lds) {
    const int t = threadIdx.x;
    int L = 1;
    while (L < count) L <<= 1;
    const int Q = max(1, L / kFinishThreads), width = L / Q;
    float v = 0.f;
    if (t < width) {
        switch (Q) {
            case 1: v = tree_fold<1>(e, t, width, count); break;
            case 2: v = tree_fold<2>(e, t, width, count); break;
            case 4: v = tree_fold<4>(e, t, width, count); break;
            case 8: v = tree_fold<8>(e, t, width, count); break;
            case 16: v = tree_fold<16>(e, t, width, count); break;
            case 32: v = tree_fold<32>(e, t, width, count); break;
            default: v = tree_fold<64>(e, t, width, count); break;
        }
    }
    __syncthreads();  // (whoever read lds before is done)
    lds[t] = v;
    for (int h = width / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (t < h) lds[t] = lds[t] + lds[t + h];
    }
    __syncthreads();
    return lds[0];
}
static_assert(65536 / kFinishThreads == 64, "tree_fold<64> holds the largest cloud");

struct Finish {
    int debias;
    float inv_n, inv_m;
    float *cost, *pot_x, *pot_y, *grad_x, *grad_y;
    float *e;  // [b, n + m] the potentials the trees run over (null: no cost)
};

// The final round's partials -> f*, g*, p*, q* -> the potentials and the gradients; one thread per point of x, then of y.
__global__ __launch_bounds__(256) void sk_combine_kernel(Round r, Finish f) {
    const int cloud = blockIdx.y;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n + r.m) return;
    const int side = i >= r.n;
    if (side) i -= r.n;
    const int count = side ? r.m : r.n;
    const Scan &a = r.sc[side], &d = r.sc[f.debias ? side + 2 : side];
    float *pot = side ? f.pot_y : f.pot_x, *grad = side ? f.grad_y : f.grad_x;
    if (!pot && !grad && !f.e) return;
    float M, tot, ga[3], gd[3];
    merge_row(r, cloud, a.row_off + i, a.nsplit, M, tot, ga, grad != nullptr);
    float star = -r.eps_ln2 * (M + fast_log2(tot * a.inv_cols));
    const float ra = 1.f / tot;
    float rd = 0.f;
    if (f.debias) {
        merge_row(r, cloud, d.row_off + i, d.nsplit, M, tot, gd, grad != nullptr);
        star = star - -r.eps_ln2 * (M + fast_log2(tot * d.inv_cols));
        rd = 1.f / tot;
    }
    if (pot) pot[(size_t)cloud * count + i] = star;
    if (f.e) f.e[(size_t)cloud * (r.n + r.m) + (side ? r.n : 0) + i] = star;
    if (grad) {
        const float inv = side ? f.inv_m : f.inv_n;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = f.debias ? ga[c] * ra - gd[c] * rd : ga[c] * ra;
            grad[((size_t)cloud * count + i) * 3 + c] = inv * v;
        }
    }
}

// One workgroup per cloud: cost[b] from the two halving trees.
__global__ __launch_bounds__(kFinishThreads) void sk_cost_kernel(int n, int m, Finish f) {
    __shared__ float lds[kFinishThreads];
    const float *e = f.e + (size_t)blockIdx.x * (n + m);
    const float tx = halving_tree(e, n, lds), ty = halving_tree(e + n, m, lds);
    if (threadIdx.x == 0) f.cost[blockIdx.x] = f.inv_n * tx + f.inv_m * ty;
}

// Column slices per scan: enough that a single cloud's rows fill the device (about 4 waves on each of its 1024 SIMDs),
// no slice shorter than one tile.  A function of n and m alone: the words of a cloud do not depend on the batch.
int split_for(int n, int m, int nscan) {
    const long long rows = (long long)(n + m) * (nscan / 2);
    int s = 1;
    while (s < kMaxSplit && rows * s < 4096LL * pcc::kWave) s <<= 1;
    return s;
}

}  // namespace

extern "C" int pcc_sinkhorn(int b, int n, int m, const float *x, const float *y, int steps, const float *eps, int debias, float *cost,
                            float *pot_x, float *pot_y, float *grad_x, float *grad_y, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 1 || m < 1) return pcc::invalid("sinkhorn: bad size");
    if (n > 65536 || m > 65536) return pcc::invalid("sinkhorn: cloud too large (n, m <= 65536)");
    if (steps < 1 || steps > PCC_SINKHORN_MAX_STEPS) return pcc::invalid("sinkhorn: bad number of steps (1 .. PCC_SINKHORN_MAX_STEPS)");
    if (b > 65535) return pcc::invalid("sinkhorn: batch too large");
    if (b == 0) return PCC_OK;
    if (!x || !y || !eps) return pcc::invalid("sinkhorn: null pointer");
    for (int t = 0; t < steps; t++)
        if (!(eps[t] > 0.f) || !std::isfinite(eps[t])) return pcc::invalid("sinkhorn: eps must be finite and > 0");
    if (!cost && !pot_x && !pot_y && !grad_x && !grad_y) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool grad = grad_x || grad_y;

    Round r{};
    r.nscan = debias ? 4 : 2;
    r.n = n, r.m = m, r.x = x, r.y = y;
    r.R = (n + m) * (r.nscan / 2);
    const int forced = pcc::tuning(PCC_TUNE_SINKHORN_SPLIT);  // measurement switch: the number of column slices
    const int allow = forced >= 1 ? std::min(forced, kMaxSplit) : split_for(n, m, r.nscan);  // slices a scan may take
    int blocks = 0;
    bool split = false;
    for (int s = 0; s < r.nscan; s++) {
        Scan &sc = r.sc[s];
        sc.rows_y = s & 1, sc.cols_y = s < 2 ? !(s & 1) : (s & 1);
        sc.rows = sc.rows_y ? m : n, sc.cols = sc.cols_y ? m : n;
        sc.row_off = (s & 1 ? n : 0) + (s >= 2 ? n + m : 0);
        sc.col_off = s < 2 ? (s & 1 ? 0 : n) : sc.row_off;
        sc.chunk = std::max(kTile, pcc::ceil_div(pcc::ceil_div(sc.cols, allow), kGroup) * kGroup);
        sc.nsplit = pcc::ceil_div(sc.cols, sc.chunk);
        sc.blk0 = blocks, sc.nblk = pcc::ceil_div(sc.rows, kRows) * sc.nsplit;
        sc.inv_cols = (float)(1.0 / (double)sc.cols);
        blocks += sc.nblk;
        split |= sc.nsplit > 1;
    }
    r.S = 1;  // the slices actually taken (often fewer: none is shorter than a tile), which is what the partial arrays hold
    for (int s = 0; s < r.nscan; s++) r.S = std::max(r.S, r.sc[s].nsplit);

    // workspace: two generations of the potentials, the partials, the final round's weighted differences, the trees' input
    const size_t words = (size_t)b * r.R;
    const size_t w_part = words * r.S * 2, w_g = grad ? words * r.S * 3 : 0, w_e = cost ? (size_t)b * (n + m) : 0;
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc((2 * words + w_part + w_g + w_e) * sizeof(float), "sinkhorn: workspace allocation failed")) return rc;
    float *gen[2] = {static_cast<float *>(ws.p), static_cast<float *>(ws.p) + words};
    r.part = reinterpret_cast<float2 *>(gen[1] + words);  // (8-byte aligned: the block is, and 2 words is even)
    float *tail = gen[1] + words + w_part;
    r.gpart = grad ? tail : nullptr;
    float *e = cost ? tail + w_g : nullptr;

    const dim3 grid((unsigned)blocks, (unsigned)b), mgrid((unsigned)pcc::ceil_div(r.R, 256), (unsigned)b);
    auto set_eps = [&r](float v) {
        const double k = 1.4426950408889634 / (double)v;
        r.k = (float)k, r.nhk = (float)(-0.5 * k), r.eps_ln2 = (float)((double)v * 0.6931471805599453);
    };
    int cur = 0;  // the generation the next round writes
    for (int t = -1; t < steps; t++) {
        set_eps(eps[t < 0 ? 0 : t]);
        r.hin = t < 0 ? nullptr : gen[cur ^ 1];
        r.hout = gen[cur];
        r.average = t >= 0;
        {
            static const char *const kScanNames[] = {
                "sk_scan_kernel S=1", "sk_scan_kernel S=2", "sk_scan_kernel S=3", "sk_scan_kernel S=4",
                "sk_scan_kernel S=5", "sk_scan_kernel S=6", "sk_scan_kernel S=7", "sk_scan_kernel S=8",
                "sk_scan_kernel S=9", "sk_scan_kernel S=10", "sk_scan_kernel S=11", "sk_scan_kernel S=12",
                "sk_scan_kernel S=13", "sk_scan_kernel S=14", "sk_scan_kernel S=15", "sk_scan_kernel S=16"};  // (the slices the scans take)
            static_assert(sizeof kScanNames / sizeof kScanNames[0] == kMaxSplit, "one profile name per slice count");
            pcc::ProfScope prof(kScanNames[r.S - 1], st);
            hipLaunchKernelGGL(sk_scan_kernel<false>, grid, dim3(kRows), 0, st, r);
        }
        if (int rc = pcc::check_launch("sinkhorn(scan)")) return rc;
        if (split) {
            pcc::ProfScope prof("sk_merge_kernel", st);
            hipLaunchKernelGGL(sk_merge_kernel, mgrid, dim3(256), 0, st, r);
            if (int rc = pcc::check_launch("sinkhorn(merge)")) return rc;
        }
        cur ^= 1;
    }
    set_eps(eps[steps - 1]);
    r.hin = gen[cur ^ 1];
    r.hout = nullptr;
    r.average = 0;
    {
        pcc::ProfScope prof("sk_scan_final_kernel", st);
        if (grad) hipLaunchKernelGGL(sk_scan_kernel<true>, grid, dim3(kRows), 0, st, r);
        else hipLaunchKernelGGL(sk_scan_kernel<false>, grid, dim3(kRows), 0, st, r);
    }
    if (int rc = pcc::check_launch("sinkhorn(final scan)")) return rc;
    const Finish f{debias != 0, (float)(1.0 / (double)n), (float)(1.0 / (double)m), cost, pot_x, pot_y, grad_x, grad_y, e};
    {
        pcc::ProfScope prof("sk_combine_kernel", st);
        hipLaunchKernelGGL(sk_combine_kernel, dim3((unsigned)pcc::ceil_div(n + m, 256), (unsigned)b), dim3(256), 0, st, r, f);
    }
    if (int rc = pcc::check_launch("sinkhorn(combine)")) return rc;
    if (!cost) return PCC_OK;
    {
        pcc::ProfScope prof("sk_cost_kernel", st);
        hipLaunchKernelGGL(sk_cost_kernel, dim3((unsigned)b), dim3(kFinishThreads), 0, st, n, m, f);
    }
    return pcc::check_launch("sinkhorn(cost)");
}
