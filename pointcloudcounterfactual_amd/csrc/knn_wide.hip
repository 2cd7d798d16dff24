// k-NN graph for the calls outside the box of the kernels of knn_lowdim.hip and knn_mfma.hip (k > 32, or c > 128), gfx950, wave64.
//
// Same formulas, same rounding and the same ordering contract as those kernels (include/pcc_neighbour.h):
//   * c <= 3: difference form sum_c (x_j - x_i)^2 as an fma chain over the channels, computed inside the selection
//     kernel (exhaustive scan);
//   * c >= 4: expanded form (-2*dot + |x_j|^2) + |x_i|^2.  knn_wide_dist_kernel computes the inner products of a block of
//     128 queries x 128 candidates on v_mfma_f32_32x32x2_f32, streaming the channels in chunks of 16 through LDS and
//     carrying one accumulator across the chunks, so every inner product is ONE sequential fma chain over the channel
//     index (bit-identical to the oracle for any c).  The distances go to a workspace [query][candidate] (at most
//     kWideRowsBytes per launch pair: larger calls run in chunks of samples or of queries).
// Selection (knn_wide_select_kernel): one wave per query, the list of the L >= k smallest 64-bit keys (order-preserving
// distance bits : candidate index -- one unsigned compare is "distance, then index") spread over the lanes, element
// e = lane + 64 h in register h.  Candidates are tested 64 at a time against the current k-th key; the few that pass are
// appended to a buffer of L keys in LDS (ballot + mbcnt: no lane waits for another), and a full buffer is merged into
// the list by one bitonic sort of list + buffer in registers (the lower half is the new list).
//
// pcc_knn_cross (k neighbours of one cloud IN another, include/pcc_neighbour.h) runs the same two kernels with a second
// operand: the queries come from q[b][c][nq], the candidates from x[b][c][n]; the self search passes q = x.  The distances
// of the selected entries are recovered from the keys (the map of wide_key is invertible) when the caller asks for them.
// Few queries against many candidates (rows < 8 x CUs) would leave the chip empty with one wave per query: the selection
// then runs per (query, slice of the candidate axis), every wave writes its sorted list of L keys to workspace, and the
// same kernel, reading keys instead of distances, keeps the lowest k of a query's lists.  Keys are a total order
// (distance bits : candidate index), so the result does not depend on the number of slices.
#include <algorithm>

#include "knn.hpp"
#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"
#include "wave_sort.hpp"

namespace {

typedef unsigned long long u64;

constexpr u64 kWideKeyMax = ~0ull;                          // empty slot: above every key of a real candidate
constexpr size_t kWideRowsBytes = (size_t)256 << 20;        // distance workspace per launch pair
constexpr int kDT = 128;                                    // queries = candidates per distance workgroup
constexpr int kDCH = 16;                                    // channels per staged chunk

// Order-preserving key: -0 is first made +0 (the oracle compares with '<', so the two are equal); negative distances
// (the expanded form can round below zero) flip all bits, the others only the sign bit.  NaN is filtered by the caller.
__device__ __forceinline__ u64 wide_key(float d, int j) {
    const unsigned u = __float_as_uint(d + 0.0f);
    const unsigned o = u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
    return ((u64)o << 32) | (unsigned)j;
}

// the distance a key was made from (+0 for either zero)
__device__ __forceinline__ float wide_key_dist(u64 key) {
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float((o & 0x80000000u) ? o ^ 0x80000000u : ~o);
}

// c >= 4: distances of queries q0 + [0, nq) of q[b][c][nqt] against all n candidates of x[b][c][n], samples
// s0 + blockIdx.z, to D[blockIdx.z][q - q0][j] (sqq, sqx: the squared norms of the two clouds; the self search passes
// q = x, sqq = sqx, nqt = n).  Workgroup = 4 waves, 128 queries x 128 candidates; wave w owns queries w*32 + [0, 32) against
// the four 32-candidate tiles (four independent accumulator chains).  MFMA A = queries, B = candidates, so accumulator
// register r of lane (half, col) is query (r & 3) + 8 (r >> 2) + 4 half, candidate col: the stores of a register are
// 32 consecutive candidates of one row.
__global__ __launch_bounds__(256) void knn_wide_dist_kernel(int c, int n, int nqt, int nq, int q0, int s0,
                                                            const float *__restrict__ q, const float *__restrict__ x,
                                                            const float *__restrict__ sqq, const float *__restrict__ sqx,
                                                            float *__restrict__ D) {
    constexpr int E = kDCH * kDT / 256;  // elements per thread per operand per chunk
    __shared__ __attribute__((aligned(16))) float sQ[2][kDCH][kDT];
    __shared__ __attribute__((aligned(16))) float sC[2][kDCH][kDT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int smp = s0 + (int)blockIdx.z;
    const float *qb = q + (size_t)smp * c * nqt, *xb = x + (size_t)smp * c * n;
    const float *sqqb = sqq + (size_t)smp * nqt, *sqxb = sqx + (size_t)smp * n;
    const int qt = blockIdx.x * kDT, ct = blockIdx.y * kDT;  // first local query / first candidate of the workgroup
    const int nch = pcc::ceil_div(c, kDCH);

    float pq[E], pc[E];
    // loads at clamped addresses (issued before the MFMAs of the current chunk); the out-of-range select at commit
    auto fetch = [&](int ch0) {
#pragma unroll
        for (int i = 0; i < E; i++) {
            const int e = tid + i * 256, ch = min(ch0 + (e >> 7), c - 1), p = e & (kDT - 1);
            pq[i] = qb[(size_t)ch * nqt + min(q0 + qt + p, nqt - 1)];
            pc[i] = xb[(size_t)ch * n + min(ct + p, n - 1)];
        }
    };
    auto commit = [&](int ch0, int buf) {
#pragma unroll
        for (int i = 0; i < E; i++) {
            const int e = tid + i * 256, ch = e >> 7, p = e & (kDT - 1);
            const bool cin = ch0 + ch < c;
            sQ[buf][ch][p] = (cin && qt + p < nq) ? pq[i] : 0.f;  // (zero channels extend the chain exactly)
            sC[buf][ch][p] = (cin && ct + p < n) ? pc[i] : 0.f;
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) acc[u] = zero16();
    fetch(0);
    commit(0, 0);
    __syncthreads();
    for (int t = 0; t < nch; t++) {
        const int buf = t & 1;
        if (t + 1 < nch) fetch((t + 1) * kDCH);
#pragma unroll
        for (int ks = 0; ks < kDCH / 2; ks++) {
            const float a = sQ[buf][2 * ks + half][w * 32 + col];  // query[row = col][k = half] of channel pair ks
            float bv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) bv[u] = sC[buf][2 * ks + half][u * 32 + col];
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[u], acc[u], 0, 0, 0);
        }
        if (t + 1 < nch) commit((t + 1) * kDCH, buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = ct + u * 32 + col;
        const float sqj = sqxb[min(j, n - 1)];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int ql = qt + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (ql < nq && j < n) {
                // the reference CPU path: dist = -2*dot ; dist += |xj|^2 ; dist += |qi|^2
                const float d = (-2.0f * acc[u][r] + sqj) + sqqb[q0 + ql];
                D[((size_t)blockIdx.z * nq + ql) * n + j] = d;
            }
        }
    }
}

enum WideSrc { kSrcDiff = 0, kSrcRows = 1, kSrcKeys = 2 };  // where the selection kernel takes its candidates from

struct WideSelArgs {
    int c, n, k;
    int rows;         // queries of this launch: row r is sample s0 + r / nq, query q0 + r % nq
    int nq, q0, s0;
    int nqt;          // queries per sample of the whole call: the row stride of q and of the outputs
    int slices, slice_len;  // the candidate axis in `slices` runs of slice_len candidates (blockIdx.y); 1: one wave scans all
    const float *q;   // kSrcDiff: the query cloud [b][c][nqt]
    const float *x;   // kSrcDiff: the candidate cloud [b][c][n]
    const float *D;   // kSrcRows: distances [rows][n]
    u64 *part;        // slices > 1: the sorted lists of the slices, [rows][slices][L] (written; kSrcKeys reads them)
    int64_t *out;     // [b][nqt][k]
    float *dist;      // [b][nqt][k] or null
};

constexpr int kSelW = 4;  // waves (= queries) per selection workgroup
constexpr int wide_slots(int k) { return k <= 64 ? 64 : 128; }  // list slots L of the selection instantiation for k

// L = list slots (64 or 128, >= k).  One wave per query (per query and slice when the candidate axis is cut, with the
// list going to a.part instead of the outputs); kSrcKeys selects among the keys of a query's slice lists.  See the file
// header.
template <int L, int SRC>
__global__ __launch_bounds__(64 * kSelW) void knn_wide_select_kernel(WideSelArgs a) {
    constexpr int R = L / 64;  // list keys per lane
    constexpr bool DIFF = SRC == kSrcDiff;
    __shared__ u64 sbuf[kSelW][L];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = (int)blockIdx.x * kSelW + w;
    if (row >= a.rows) return;  // (whole wave; the kernel has no workgroup barrier)
    u64 *buf = sbuf[w];
    const int n = a.n, k = a.k;
    const int smp = a.s0 + row / a.nq, q = a.q0 + row % a.nq;
    const bool partial = SRC != kSrcKeys && a.slices > 1;
    u64 *plist = a.slices > 1 ? a.part + (size_t)row * a.slices * L : nullptr;
    // candidates [lo, hi) of this wave: indices into the cloud, or into the keys of the query's slice lists
    const int lo = partial ? (int)blockIdx.y * a.slice_len : 0;
    const int hi = SRC == kSrcKeys ? a.slices * L : (partial ? min(n, lo + a.slice_len) : n);

    const float *xb = nullptr, *drow = nullptr;
    float qc[3] = {0.f, 0.f, 0.f};
    if (DIFF) {
        xb = a.x + (size_t)smp * a.c * n;
        const float *qb = a.q + (size_t)smp * a.c * a.nqt;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) qc[ch] = ch < a.c ? qb[(size_t)ch * a.nqt + q] : 0.f;
    } else if (SRC == kSrcRows) {
        drow = a.D + (size_t)row * n;
    }
    auto dist = [&](int j) -> float {
        if (DIFF) {
            // sum over the channels in channel order: df0^2, then fma(df, df, acc)
            float acc = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                if (ch < a.c) {
                    const float df = xb[(size_t)ch * n + j] - qc[ch];
                    acc = ch == 0 ? df * df : __builtin_fmaf(df, df, acc);
                }
            }
            return acc;
        }
        return drow[j];
    };
    // the key of candidate j (j clamped into [lo, hi) by the caller), kWideKeyMax if it can never enter a list
    auto cand = [&](int j) -> u64 {
        if (SRC == kSrcKeys) return plist[j];
        const float d = dist(j);
        return d == d ? wide_key(d, j) : kWideKeyMax;  // (a NaN distance never enters)
    };

    u64 list[R];
#pragma unroll
    for (int h = 0; h < R; h++) list[h] = kWideKeyMax;
    u64 thr = kWideKeyMax;  // the k-th key of the list: nothing at or above it can end among the k nearest
    int cnt = 0;            // keys in the buffer (wave-uniform)

    auto merge = [&]() {
        __builtin_amdgcn_wave_barrier();
        u64 v[2 * R];
#pragma unroll
        for (int h = 0; h < R; h++) {
            v[h] = list[h];
            v[R + h] = lane + 64 * h < cnt ? buf[lane + 64 * h] : kWideKeyMax;
        }
        __builtin_amdgcn_wave_barrier();
        pcc::wave_bitonic(v, lane);
#pragma unroll
        for (int h = 0; h < R; h++) list[h] = v[h];
        const u64 kth = (R == 1 || k <= 64) ? list[0] : list[R - 1];
        thr = pcc::readlane_u64(kth, (k - 1) & 63);
        cnt = 0;
    };

    constexpr int U = 4;  // candidate blocks of 64 whose loads are issued together
    for (int j0 = lo; j0 < hi; j0 += 64 * U) {
        u64 key[U];
#pragma unroll
        for (int u = 0; u < U; u++) key[u] = cand(min(j0 + 64 * u + lane, hi - 1));
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int j = j0 + 64 * u + lane;
            if (j0 + 64 * u >= hi) break;  // (wave-uniform)
            bool pass = j < hi && key[u] < thr;
            u64 m = __ballot(pass);
            int np = __popcll(m);
            if (cnt + np > L) {
                merge();
                pass = pass && key[u] < thr;
                m = __ballot(pass);
                np = __popcll(m);
            }
            if (pass) buf[cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = key[u];
            cnt += np;
        }
    }
    if (cnt > 0) merge();

    if (partial) {  // this slice's list, sorted, empty slots included
        u64 *dst = plist + (size_t)blockIdx.y * L;
#pragma unroll
        for (int h = 0; h < R; h++) dst[lane + 64 * h] = list[h];
        return;
    }
    const size_t o = ((size_t)smp * a.nqt + q) * k;
#pragma unroll
    for (int h = 0; h < R; h++) {
        const int s = lane + 64 * h;
        if (s < k) {
            const unsigned j = (unsigned)list[h];
            const bool real = j < (unsigned)n;  // (an empty slot: fewer than k distances that are not NaN; +inf has a key and is listed)
            a.out[o + s] = (int64_t)(real ? (int)j : n - 1);
            if (a.dist) a.dist[o + s] = real ? wide_key_dist(list[h]) : __builtin_nanf("");
        }
    }
}

template <int L, int SRC>
void launch_select(const WideSelArgs &a, hipStream_t st) {
    // the launch profile's name: <list slots, source of the keys>, "sliced" where the candidate axis is cut (a.slices > 1:
    // partial lists to workspace, merged by the <.,keys> launch that follows)
    static const char *const kNames[2][3][2] = {
        {{"knn_wide_select_kernel<64,diff>", "knn_wide_select_kernel<64,diff> sliced"},
         {"knn_wide_select_kernel<64,rows>", "knn_wide_select_kernel<64,rows> sliced"},
         {"knn_wide_select_kernel<64,keys>", "knn_wide_select_kernel<64,keys>"}},
        {{"knn_wide_select_kernel<128,diff>", "knn_wide_select_kernel<128,diff> sliced"},
         {"knn_wide_select_kernel<128,rows>", "knn_wide_select_kernel<128,rows> sliced"},
         {"knn_wide_select_kernel<128,keys>", "knn_wide_select_kernel<128,keys>"}}};
    pcc::ProfScope prof(kNames[L == 128][SRC == kSrcDiff ? 0 : SRC == kSrcRows ? 1 : 2][a.slices > 1], st);
    hipLaunchKernelGGL((knn_wide_select_kernel<L, SRC>), dim3(pcc::ceil_div(a.rows, kSelW), SRC == kSrcKeys ? 1 : a.slices),
                       dim3(64 * kSelW), 0, st, a);
}

template <int SRC>
void launch_select(const WideSelArgs &a, hipStream_t st) {
    if (wide_slots(a.k) == 64) launch_select<64, SRC>(a, st);
    else launch_select<128, SRC>(a, st);
}

// Slices of the candidate axis for a launch of `rows` queries (pcc_knn_cross only; the self search never splits).  One wave
// per query fills the chip from 8 waves per CU on (two per SIMD); below that, enough slices to get there, at most 64
// (the query's wave then merges <= 64 lists) and none shorter than 2048 candidates.  0 CUs (query failed): no split.
int cross_slices(int rows, int n) {
    const int sw = pcc::tuning(PCC_TUNE_KNN_CROSS_SPLIT);  // measurement switch: S >= 1 forces S slices
    if (sw >= 1) return std::min(sw, 4096);
    const int target = 8 * pcc::device_cus();
    if (rows >= target) return 1;
    return std::max(1, std::min({pcc::ceil_div(target, rows), 64, n / 2048}));
}

// The selection of one launch: a.slices == 1 straight to the outputs, otherwise per slice to workspace and a second launch
// that keeps the lowest k keys of each query's lists.
template <int SRC>
int select_rows(WideSelArgs a, int slices, hipStream_t st) {
    // whole blocks of 256 candidates per slice (the loop's unit), no empty slice
    a.slice_len = pcc::ceil_div(pcc::ceil_div(a.n, slices), 256) * 256;
    a.slices = pcc::ceil_div(a.n, a.slice_len);
    if (a.slices == 1) {
        launch_select<SRC>(a, st);
        return pcc::check_launch("knn(wide select)");
    }
    pcc::WsBlock part(st);
    if (int rc = part.alloc((size_t)a.rows * a.slices * wide_slots(a.k) * sizeof(u64), "knn: workspace allocation failed")) return rc;
    a.part = static_cast<u64 *>(part.p);
    launch_select<SRC>(a, st);
    if (int rc = pcc::check_launch("knn(wide select)")) return rc;
    launch_select<kSrcKeys>(a, st);
    return pcc::check_launch("knn(wide merge)");
}

// The search behind pcc_knn's wide path (q = x, nqt = n, no distances, never split) and pcc_knn_cross.
int wide_search(int b, int c, int nqt, int n, int k, const float *q, const float *x, int64_t *indices, float *dist, bool cross,
                hipStream_t st) {
    using namespace pcc;
    WideSelArgs a{};
    a.c = c; a.n = n; a.k = k; a.nqt = nqt; a.q = q; a.x = x; a.out = indices; a.dist = dist;
    if (c <= 3) {
        a.rows = b * nqt; a.nq = nqt; a.q0 = 0; a.s0 = 0;
        return select_rows<kSrcDiff>(a, cross ? cross_slices(a.rows, n) : 1, st);
    }
    // distance rows per launch pair: whole samples while they fit, otherwise a multiple of 128 queries of one sample
    const size_t cap = kWideRowsBytes / sizeof(float);
    const size_t per_smp = (size_t)nqt * n;
    int ns, nq;
    if (per_smp <= cap) {
        ns = (int)std::min<size_t>((size_t)b, cap / per_smp);
        nq = nqt;
    } else {
        ns = 1;
        nq = (int)std::min<size_t>((size_t)nqt, std::max<size_t>(kDT, cap / n / kDT * kDT));
    }
    const bool self = q == x && nqt == n;  // one norm row serves both operands
    WsBlock sq(st), dw(st);
    if (int rc = sq.alloc(((size_t)b * n + (self ? 0 : (size_t)b * nqt)) * sizeof(float), "knn: workspace allocation failed")) return rc;
    if (int rc = dw.alloc((size_t)ns * nq * n * sizeof(float), "knn: workspace allocation failed")) return rc;
    float *sqx = static_cast<float *>(sq.p), *sqq = self ? sqx : sqx + (size_t)b * n, *D = static_cast<float *>(dw.p);
    launch_sqnorm(b, c, n, x, sqx, st);
    if (!self) launch_sqnorm(b, c, nqt, q, sqq, st);
    if (int rc = check_launch("knn(wide sqnorm)")) return rc;
    a.D = D;
    for (int s0 = 0; s0 < b; s0 += ns) {
        const int cs = std::min(ns, b - s0);
        for (int q0 = 0; q0 < nqt; q0 += nq) {
            const int cq = std::min(nq, nqt - q0);
            {
                pcc::ProfScope prof("knn_wide_dist_kernel", st);
                hipLaunchKernelGGL(knn_wide_dist_kernel, dim3(ceil_div(cq, kDT), ceil_div(n, kDT), cs), dim3(256), 0, st, c, n, nqt,
                                   cq, q0, s0, q, x, sqq, sqx, D);
            }
            if (int rc = check_launch("knn(wide distances)")) return rc;
            a.rows = cs * cq; a.nq = cq; a.q0 = q0; a.s0 = s0;
            if (int rc = select_rows<kSrcRows>(a, cross ? cross_slices(a.rows, n) : 1, st)) return rc;
        }
    }
    return PCC_OK;
}

}  // namespace

namespace pcc {

// Sizes are validated by pcc_knn: 1 <= k <= min(n, 128), b <= 65535, non-null pointers.
int knn_wide(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st) {
    return wide_search(b, c, n, n, k, x, x, indices, nullptr, false, st);
}

}  // namespace pcc

extern "C" int pcc_knn_cross(int b, int c, int nq, int n, int k, const float *q, const float *x, int64_t *indices, float *dist,
                             pcc_stream_t stream) {
    pcc::clear_error();
    bool empty;
    if (int rc = knn_check_sizes("knn_cross", "candidates", b, c, nq, n, k, &empty); rc || empty) return rc;
    if ((long long)b * nq > 0x7fffffffLL) return pcc::invalid("knn_cross: too many queries (b * nq >= 2^31)");
    if (c >= 4 && n > 65535 * kDT) return pcc::invalid("knn_cross: too many candidates for c >= 4 (n > 65535 * 128)");
    if (!q || !x || !indices) return pcc::invalid("knn_cross: null pointer");
    return wide_search(b, c, nq, n, k, q, x, indices, dist, true, static_cast<hipStream_t>(stream));
}
