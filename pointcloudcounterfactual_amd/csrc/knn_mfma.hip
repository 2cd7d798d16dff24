// k-NN graph, 4 <= c <= 128 and k <= 32, for gfx950 (MI355X), wave64: expanded-form distances with the inner product on
// v_mfma_f32_32x32x2_f32.  knn_mfma_kernel (128-query workgroups), knn_mfma_split_kernel (256-query role-split workgroups
// for launches that fill the chip) and sqnorm_kernel (the squared norms both read, also for knn_wide.hip).
// The overview of the k-NN kernels is at the top of knn.hip.
#include "knn.hpp"
#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"
#include "topk.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int kTT128 = 1;  // tiles per stage of the 128-channel MFMA instantiation

__global__ __launch_bounds__(256) void sqnorm_kernel(int c, int n, const float *__restrict__ x, float *__restrict__ sq) {
    // sq[b][i] = sum_c x[b,c,i]^2 in channel order
    const int smp = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *xb = x + (size_t)smp * c * n;
    float s = 0.f;
    for (int ch = 0; ch < c; ch++) {
        const float v = xb[(size_t)ch * n + i];
        s = __builtin_fmaf(v, v, s);
    }
    sq[(size_t)smp * n + i] = s;
}

// ---------------------------------------------------------------------------------------------------
// c >= 4: MFMA kernel.
// Workgroup = 4 waves, each wave 32 queries (columns of the 32x32 accumulator tile = lane & 31); the two
// half-waves hold different candidate rows of the tile (row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)), so each
// query has two partial top-K lists which are merged at the end.  Candidate tiles [c][32] are staged in
// LDS once per workgroup and shared by the 4 waves.  B operand (queries) lives in c/2 VGPRs per lane.
// ---------------------------------------------------------------------------------------------------
template <int K, int CP /* padded channels, multiple of 2, <= 128 */, int TT /* 32-candidate tiles per stage */>
__global__ __launch_bounds__(256, CP >= 128 ? 2 : 1) void knn_mfma_kernel(int c, int n, int k, const float *__restrict__ x,
                                                        const float *__restrict__ sq,
                                                        int64_t *__restrict__ indices) {
    constexpr int T = 256;
    constexpr int KS = CP / 2;  // MFMA k-steps (32x32x2)
    constexpr int TW = 32 * TT;  // candidates per stage
    constexpr int tile_bytes = CP * TW * 4;
    constexpr int buf_bytes = 2 * kCap * T * 4;
    constexpr int merge_bytes = 2 * 8 * K * 32 * 4;  // [wave(4)][half(2)][K][32 queries]
    constexpr int main_bytes = 2 * tile_bytes + 2 * TW * 4 + buf_bytes;
    constexpr int bytes = main_bytes > merge_bytes ? main_bytes : merge_bytes;
    __shared__ __attribute__((aligned(16))) unsigned char smem[bytes];
    float *tile = reinterpret_cast<float *>(smem);                       // [2][CP][TW]
    float *tsq = reinterpret_cast<float *>(smem + 2 * tile_bytes);      // [2][TW]
    float *buf_d = reinterpret_cast<float *>(smem + 2 * tile_bytes + 2 * TW * 4);
    int *buf_i = reinterpret_cast<int *>(smem + 2 * tile_bytes + 2 * TW * 4 + kCap * T * 4);
    float *mrg_d = reinterpret_cast<float *>(smem);
    int *mrg_i = reinterpret_cast<int *>(smem + 8 * K * 32 * 4);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, col = lane & 31;
    const int smp = blockIdx.y;
    const float *xb = x + (size_t)smp * c * n;
    const float *sqb = sq + (size_t)smp * n;
    int q = blockIdx.x * 128 + w * 32 + col;
    const bool q_ok = q < n;
    q = q_ok ? q : n - 1;
    // B operand: query[col][k = 2*ks + half]
    float bq[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        const int ch = 2 * ks + half;
        bq[ks] = ch < c ? xb[(size_t)ch * n + q] : 0.f;
    }
    const float sq_q = sqb[q];

    pcc::BufferedTopK<K, kCap, T> tk;
    tk.init(buf_d, buf_i, tid);

    const int nstages = (n + TW - 1) / TW;
    // Staging is software-pipelined by hand: the global loads of stage t+1 are all issued (unconditional, clamped
    // addresses; the select happens on the value) BEFORE the MFMAs of stage t and land in LDS after them.  Written as
    // a plain conditional copy loop the compiler emitted load -> s_waitcnt vmcnt(0) -> ds_write per element, i.e. one
    // exposed memory round trip per element (the kernel spent most of its time there).
    constexpr int E = CP * TW / T;  // elements per thread per stage
    static_assert(CP * TW % T == 0, "stage size must be a multiple of the workgroup");
    float pre[E], pre_sq = 0.f;
    // fetch only issues the loads (clamped addresses, nothing consumes the values); the out-of-range select happens at
    // commit time, behind the MFMAs -- a select next to the load makes the compiler wait for every load where it is issued.
    auto fetch = [&](int t) {
        const int j0 = t * TW;
#pragma unroll
        for (int i = 0; i < E; i++) {
            const int e = tid + i * T;
            const int ch = e / TW, j = e - ch * TW;
            pre[i] = xb[(size_t)min(ch, c - 1) * n + min(j0 + j, n - 1)];
        }
        pre_sq = sqb[min(j0 + (tid % TW), n - 1)];
    };
    auto commit = [&](int t) {
        const int j0 = t * TW;
        float *dst = tile + (t & 1) * CP * TW;
#pragma unroll
        for (int i = 0; i < E; i++) {
            const int e = tid + i * T;
            const int ch = e / TW, j = e - ch * TW;
            dst[e] = (ch < c && j0 + j < n) ? pre[i] : 0.f;
        }
        if (tid < TW) tsq[(t & 1) * TW + tid] = (j0 + tid < n) ? pre_sq : __builtin_inff();
    };
    // The two half-waves keep separate lists for the same query (lane and lane ^ 32).  Each list alone would keep
    // buffering until ITS K-th distance is beaten; but once both lists hold ceil(K/2) entries <= t, at least K candidates
    // are <= t, so nothing above t can reach the query's k nearest: after every drain the buffering threshold drops to
    // the larger of the two lists' ceil(K/2)-th entries (ties at t still pass: the threshold is the next float above t).
    auto flush_shared = [&]() {
        tk.flush();
        const float mine = tk.top.d[(K + 1) / 2 - 1];
        const float t = fmaxf(mine, __shfl_xor(mine, 32, 64));
        float up = t;  // next float above t (t is never NaN; +inf stays)
        if (t < __builtin_inff()) {
            const int bits = __float_as_int(t);
            up = t == 0.f ? __int_as_float(1) : __int_as_float(t > 0.f ? bits + 1 : bits - 1);
        }
        tk.thr = fminf(tk.thr, up);
    };
    fetch(0);
    commit(0);
    __syncthreads();
    for (int t = 0; t < nstages; t++) {
        const int slot = t & 1;
        if (t + 1 < nstages) fetch(t + 1);
        const float *cur = tile + slot * CP * TW;
        // TT independent accumulator chains: a dependent MFMA cannot issue before the previous one has left the
        // matrix pipe, so one chain per wave leaves the pipe idle half of the time (measured 166 cycles per
        // v_mfma_f32_32x32x2_f32 against the 64 it occupies)
        f32x16 acc[TT];
#pragma unroll
        for (int u = 0; u < TT; u++) acc[u] = zero16();
        // A operands are read from LDS eight k-steps ahead of the MFMAs that consume them (one ds_read + full wait
        // per MFMA left the matrix pipe idle for the LDS latency every step)
        constexpr int KB = KS < 4 ? KS : 4;
#pragma unroll
        for (int ks0 = 0; ks0 < KS; ks0 += KB) {
            float av[KB][TT];
#pragma unroll
            for (int kk = 0; kk < KB; kk++)
#pragma unroll
                for (int u = 0; u < TT; u++)
                    av[kk][u] = cur[(2 * (ks0 + kk) + half) * TW + u * 32 + col];  // candidate[row = lane&31][k] of sub-tile u
#pragma unroll
            for (int kk = 0; kk < KB; kk++)
#pragma unroll
                for (int u = 0; u < TT; u++)
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk][u], bq[ks0 + kk], acc[u], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < TT; u++) {
            if (tk.must_flush(16)) flush_shared();
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = u * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;  // candidate inside the stage
                // reference CPU path: dist = -2*dot ; dist += |xj|^2 (column term) ; dist += |xi|^2 (row term)
                const float d = (-2.0f * acc[u][r] + tsq[slot * TW + row]) + sq_q;
                tk.offer(d, t * TW + row);
            }
        }
        if (t + 1 < nstages) commit(t + 1);
        __syncthreads();
    }
    tk.flush();
    __syncthreads();
#pragma unroll
    for (int s = 0; s < K; s++) {
        mrg_d[((w * 2 + half) * K + s) * 32 + col] = tk.top.d[s];
        mrg_i[((w * 2 + half) * K + s) * 32 + col] = tk.top.i[s];
    }
    __syncthreads();
    if (half == 0 && q_ok) {
        // two-way merge of the half-wave lists; ties: lower candidate index first (the lists cover interleaved
        // row groups, so compare indices explicitly)
        const float *d0 = mrg_d + ((w * 2 + 0) * K) * 32 + col, *d1 = mrg_d + ((w * 2 + 1) * K) * 32 + col;
        const int *i0 = mrg_i + ((w * 2 + 0) * K) * 32 + col, *i1 = mrg_i + ((w * 2 + 1) * K) * 32 + col;
        int p0 = 0, p1 = 0;
        int filled = 0;  // slots that took a list entry (an empty slot of either list has index 0x7fffffff)
        int64_t *dst = indices + ((size_t)smp * n + q) * k;
        for (int o = 0; o < k; o++) {
            const float a = p0 < K ? d0[p0 * 32] : __builtin_inff();
            const float bb = p1 < K ? d1[p1 * 32] : __builtin_inff();
            const int ia = p0 < K ? i0[p0 * 32] : 0x7fffffff;
            const int ib = p1 < K ? i1[p1 * 32] : 0x7fffffff;
            const bool take0 = (a < bb) || (a == bb && ia < ib);
            const int id = take0 ? ia : ib;
            dst[o] = (int64_t)min(id, n - 1);  // (n - 1: the padding of a list that stays short)
            filled += id != 0x7fffffff ? 1 : 0;
            p0 += take0 ? 1 : 0;
            p1 += take0 ? 0 : 1;
        }
        // the lists hold finite distances only: a short row continues with its +inf distances (see fill_inf_tail)
        if (filled < k)
            fill_inf_tail(
                filled, k, n, [&](int j) { return expanded_dist(xb, sqb, c, n, q, sq_q, j); },
                [&](int slot, int j) { dst[slot] = (int64_t)j; });
    }
}

// ---------------------------------------------------------------------------------------------------
// c >= 4, role-split form of the kernel above for launches that fill the chip with 256-query workgroups.
//
// What the selection costs is instructions (tools/issue_bench.hip, tools/mfma_coissue_bench.hip: a wave issues a VALU
// instruction every 5-8 cycles, a branch costs tens, and MFMAs of one wave and VALU work of another on the same SIMD
// add up rather than overlap): knn_mfma_kernel spends ~50 k of them per wave of 32 queries, 4/5 in the 5-instructions-
// per-slot insertion chains of (distance, index) lists split over two half-waves.  Here:
//   * waves 0-3 ("matrix waves") only run MFMAs: each owns 64 queries = two 32-query accumulator tiles against the
//     staged 32-candidate tile, and stores the raw inner products of the stage to LDS as [query][candidate] rows --
//     the transposition the selection needs comes with the store;
//   * waves 4-7 ("selection waves") own ONE query per lane.  They stage the candidate tiles, and per stage
//       - test the 32 candidates of their query against a conservative bound of the K-th distance: fma, compare, and
//         the compare's carry shifted into a 32-bit mask (3 instructions per candidate, no branch, no LDS write);
//       - visit the set bits: the exact distance in the reference's order from the inner product still in LDS, and
//         where it beats the K-th distance, ONE v_med3_f32 per slot into a sorted list of distances WITHOUT indices,
//         plus an 8-byte (distance, index) record appended to the lane's log in global memory (stream-ordered
//         workspace, [slot][lane]: coalesced);
//     after the scan the k-th distance tau is final: a log record belongs to the result iff its distance is below
//     tau, or equals tau and it is among the first (k - #below) such records -- records are in candidate order, which
//     is the order equal distances are listed in.  The <= k selected records are ranked against the sorted distances
//     (equal distances: next free slot, in record order) and written out.  A log that nears its capacity is compacted
//     to the records not above the current K-th distance (fewer than 2K: a record is only written when it enters the
//     list).
// One barrier per stage; inner products and candidate tiles are double-buffered.  Same MFMA instruction, same k order
// and the same distance expression as knn_mfma_kernel: identical results, ties included.
// ---------------------------------------------------------------------------------------------------
constexpr int kSplitQ = 256;      // queries per workgroup
constexpr int kSplitPitch = 36;   // floats per query row of one stage (32 + 4: the rows' ds_read_b128 spread over all banks)
constexpr int kLogCap = 256;      // log records per query (compacted when fewer than 32 are free)

template <int K, int CP>
constexpr int split_lds_bytes() {
    constexpr int main_bytes = 2 * CP * 32 * 4 + 3 * 32 * 4 + 2 * kSplitQ * kSplitPitch * 4;
    constexpr int final_bytes = K * 256 * (8 + 4);  // selected records | output slots
    return main_bytes > final_bytes ? main_bytes : final_bytes;
}
inline size_t split_log_bytes(int b, int n) { return (size_t)b * pcc::ceil_div(n, kSplitQ) * kLogCap * 256 * sizeof(float2); }

// Largest value of a non-negative int over the wave (wave-uniform result).
__device__ __forceinline__ int wave_max_nonneg(int v) {
    v = max(v, pcc::dpp<pcc::kRowShr + 1>(v));
    v = max(v, pcc::dpp<pcc::kRowShr + 2>(v));
    v = max(v, pcc::dpp<pcc::kRowShr + 4>(v));
    v = max(v, pcc::dpp<pcc::kRowShr + 8>(v));
    v = max(v, pcc::dpp<pcc::kRowBcast15, 0xa>(v));  // (rows 1 and 3)
    v = max(v, pcc::dpp<pcc::kRowBcast31, 0xc>(v));  // (rows 2 and 3)
    return __builtin_amdgcn_readlane(v, 63);
}

// An 8-byte log record, read past the L1 (written by this lane earlier, read once).
__device__ __forceinline__ float2 log_load(const float2 *p) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = __builtin_nontemporal_load(reinterpret_cast<const f32x2 *>(p));
    return float2{v.x, v.y};
}

template <int K, int CP /* padded channels, multiple of 2, <= 128 */>
__global__ __launch_bounds__(512) void knn_mfma_split_kernel(int c, int n, int k, const float *__restrict__ x,
                                                             const float *__restrict__ sq, float2 *__restrict__ logs,
                                                             int64_t *__restrict__ indices) {
    constexpr int KS = CP / 2;  // MFMA k-steps (32x32x2)
    constexpr int tile_floats = CP * 32;
    constexpr int dist_floats = kSplitQ * kSplitPitch;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tile = reinterpret_cast<float *>(smem);                 // [2][CP][32]
    float *tsq = tile + 2 * tile_floats;                           // [3][32] (read one stage later than the tile: see commit)
    float *dist = tsq + 3 * 32;                                    // [2][256][36]

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int smp = blockIdx.y;
    const float *xb = x + (size_t)smp * c * n;
    const float *sqb = sq + (size_t)smp * n;
    const int nstages = (n + 31) / 32;

    if (w < 4) {
        // ---- matrix wave: queries blockIdx.x * 256 + w * 64 + [0, 64)
        const int half = lane >> 5, col = lane & 31;
        float bq[2][KS];  // B operand: query[col][k = 2 * ks + half] of the two query tiles
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int q = min(blockIdx.x * kSplitQ + w * 64 + u * 32 + col, n - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const int ch = 2 * ks + half;
                bq[u][ks] = ch < c ? xb[(size_t)ch * n + q] : 0.f;
            }
        }
        __syncthreads();  // stage 0 is in LDS
        for (int t = 0; t < nstages; t++) {
            const float *cur = tile + (t & 1) * tile_floats;
            f32x16 acc[2];
#pragma unroll
            for (int u = 0; u < 2; u++) acc[u] = zero16();
            constexpr int KB = KS < 8 ? KS : 8;  // A operands are read this many k-steps ahead of their MFMAs
#pragma unroll
            for (int ks0 = 0; ks0 < KS; ks0 += KB) {
                float av[KB];
#pragma unroll
                for (int kk = 0; kk < KB; kk++) av[kk] = cur[(2 * (ks0 + kk) + half) * 32 + col];  // candidate[row = col][k]
#pragma unroll
                for (int kk = 0; kk < KB; kk++)
#pragma unroll
                    for (int u = 0; u < 2; u++)
                        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bq[u][ks0 + kk], acc[u], 0, 0, 0);
            }
            // accumulator register r of lane (half, col) = candidate row (r & 3) + 8 * (r >> 2) + 4 * half of query col
            float *drow = dist + (t & 1) * dist_floats;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                float *qrow = drow + (w * 64 + u * 32 + col) * kSplitPitch + 4 * half;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    *reinterpret_cast<float4 *>(qrow + 8 * j) =
                        float4{acc[u][4 * j], acc[u][4 * j + 1], acc[u][4 * j + 2], acc[u][4 * j + 3]};
            }
            __syncthreads();
        }
        __syncthreads();  // (the selection waves reuse the stage buffers after this one)
        return;
    }

    // ---- selection wave: one query per lane
    const int ct = tid - 256;
    int q = blockIdx.x * kSplitQ + ct;
    const bool q_ok = q < n;
    q = q_ok ? q : n - 1;
    float sq_q = sqb[q];
    asm volatile("" : "+v"(sq_q));  // (consumed here: left pending, its wait lands in the rounds and drains the tile prefetch with it)
    float2 *logp = logs + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * kLogCap * 256 + ct;  // record s at logp[s * 256]
    float ld[K];  // the K smallest distances so far, ascending
#pragma unroll
    for (int s2 = 0; s2 < K; s2++) ld[s2] = __builtin_inff();
    int lcnt = 0;  // records in this lane's log
    // Pre-test bound on a = |xj|^2 - 2 xi.xj: every a whose distance fl(a + |xi|^2) is below the K-th distance W is
    // below it (W - |xi|^2 plus 64 times the rounding the sum and this expression can carry; +inf while the list is open).
    float bound = __builtin_inff();
    auto refresh_bound = [&]() {
        const float W = ld[K - 1];
        bound = (W - sq_q) + ((fabsf(W) + fabsf(sq_q)) * 0x1p-18f + 1e-30f);
    };
    // keep the records that can still belong to the result (fewer than 2K).  Rare; its memory accesses are asm for the
    // reason given at the log store in drain (a visible load or store here costs every stage of every call a drain of the
    // tile prefetch), one round trip per record.
    auto compact = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float W = ld[K - 1];
        const int m = wave_max_nonneg(lcnt);
        int kept = 0;
        for (int i = 0; i < m; i++) {
            if (i < lcnt) {
                unsigned long long rec;
                asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(rec) : "v"(logp + i * 256) : "memory");
                if (__uint_as_float((unsigned)rec) <= W) {
                    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(logp + kept * 256), "v"(rec) : "memory");
                    kept++;
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lcnt = kept;
    };

    // Tile staging: global -> registers TWO stages ahead -> LDS one stage ahead.  (One stage ahead, every stage waited
    // out a global-memory round trip -- several microseconds, more than its arithmetic -- before its barrier.)
    constexpr int E = CP * 32 / 256;  // tile elements per selection thread per stage
    float pre_a[E], pre_b[E], pre_sq_a = 0.f, pre_sq_b = 0.f;
    // fetch only issues the loads (clamped addresses, nothing consumes the values); the out-of-range select happens at
    // commit time, a stage later -- a select next to the load makes the compiler wait for every load where it is issued.
    auto fetch = [&](int t, float (&pre)[E], float &pre_sq) {
        const int j = min(t * 32 + (ct & 31), n - 1);
#pragma unroll
        for (int i = 0; i < E; i++) pre[i] = xb[(size_t)min((ct >> 5) + i * 8, c - 1) * n + j];
        pre_sq = sqb[j];
    };
    // (the norms of stage t are read by the selection of stage t one iteration after the matrix waves read its tile, while
    // another selection wave may already commit stage t + 2: three norm buffers, two tiles)
    auto commit = [&](int t, const float (&pre)[E], float pre_sq) {
        float *dst = tile + (t & 1) * tile_floats;
        const bool in = t * 32 + (ct & 31) < n;
        // (bit masks, not selects: the compiler turns the selects into a branch per element)
#pragma unroll
        for (int i = 0; i < E; i++)
            dst[ct + i * 256] = __int_as_float(__float_as_int(pre[i]) & -(int)(in && (ct >> 5) + i * 8 < c));
        if (ct < 32) tsq[(t % 3) * 32 + ct] = in ? pre_sq : __builtin_inff();
    };
    // screen: the candidates of stage t that may beat the K-th distance, as a bit mask
    auto screen = [&](int t) -> unsigned {
        const float *drow = dist + (t & 1) * dist_floats + ct * kSplitPitch;
        const float *ts = tsq + (t % 3) * 32;
        unsigned mask = 0;  // candidate e of the stage ends up in bit 31 - e
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 a0 = *reinterpret_cast<const float4 *>(drow + 8 * g);
            const float4 a1 = *reinterpret_cast<const float4 *>(drow + 8 * g + 4);
            const float4 n0 = *reinterpret_cast<const float4 *>(ts + 8 * g);
            const float4 n1 = *reinterpret_cast<const float4 *>(ts + 8 * g + 4);
            const float dot[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float nj[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float a = __builtin_fmaf(-2.0f, dot[e], nj[e]);  // == (-2*dot) + |xj|^2: the product is exact
                // mask = 2 * mask + (a < bound): the compare's carry goes straight into the add (false for NaN); the s_nop is
                // the two wait states gfx950 wants between a VALU write of vcc and a VALU read of it (the compiler puts the
                // same s_nop between its own v_cmp / v_addc pairs; it cannot see into this block)
                asm("v_cmp_lt_f32_e32 vcc, %1, %2\n\ts_nop 1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(mask) : "v"(a), "v"(bound) : "vcc");
            }
        }
        return __builtin_bitreverse32(mask);  // candidate e in bit e: visited in ascending order
    };
    // drain: one round per set bit of the fullest lane, straight-line: a lane without a bit offers +inf, and an offer
    // that does not beat the K-th distance leaves the list as it is (median of two neighbours and something not below
    // them), so only the log record is conditional -- no list value crosses a branch.
    auto drain = [&](int t, unsigned mask) {
        const float *drow = dist + (t & 1) * dist_floats + ct * kSplitPitch;
        const float *ts = tsq + (t % 3) * 32;
        if (__any(lcnt > kLogCap - 32)) compact();
        // (bottom-tested by hand: the compiler does not rotate a loop around a ballot, and copies the whole list on both
        // sides of a top test)
        if (__any(mask != 0)) {
            // (the LDS reads of the NEXT round's candidate are issued before this round's chain)
            int e = __builtin_ctz(mask | 0x80000000u);
            float dot = drow[e], nj = ts[e];
            do {
                const bool has = mask != 0;
                mask &= mask - 1;
                const int e_next = __builtin_ctz(mask | 0x80000000u);
                const float dot_next = drow[e_next], nj_next = ts[e_next];
                // reference CPU path: dist = -2*dot ; dist += |xj|^2 (column term) ; dist += |xi|^2 (row term)
                const float xe = __builtin_fmaf(-2.0f, dot, nj) + sq_q;
                const float xv = has ? xe : __builtin_inff();  // (never NaN: it passed a < bound with a finite bound)
                const float W = ld[K - 1];
                // (in place, tail first: written as asm so that no slot is copied around the loop)
#pragma unroll
                for (int s2 = K - 1; s2 > 0; s2--) asm volatile("v_med3_f32 %0, %1, %2, %0" : "+v"(ld[s2]) : "v"(ld[s2 - 1]), "v"(xv));
                asm volatile("v_min_f32 %0, %0, %1" : "+v"(ld[0]) : "v"(xv));
                if (xv < W) {
                    // (asm: with a store the compiler can see in this loop, its wait-count pass drains every load in
                    // flight -- the tile prefetch -- before the loop, once per stage; the explicit waits before the
                    // log is read back order these stores)
                    const unsigned long long rec =
                        ((unsigned long long)(unsigned)(t * 32 + e) << 32) | (unsigned long long)__float_as_uint(xv);
                    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(logp + lcnt * 256), "v"(rec) : "memory");
                }
                lcnt += xv < W ? 1 : 0;
                e = e_next;
                dot = dot_next;
                nj = nj_next;
            } while (__any(mask != 0));
        }
        refresh_bound();
    };
    auto step = [&](int t, float (&nxt)[E], float &nxt_sq, const float (&cur)[E], float cur_sq) {
        // (the loads fly during a whole stage; the commit comes BEFORE the rounds: behind the rounds' log stores its wait
        // for older loads would wait for the stores too)
        fetch(t + 2, nxt, nxt_sq);  // (unconditional, clamped past the end: behind a branch the compiler must wait as if it had not run)
        const unsigned mask = t > 0 ? screen(t - 1) : 0u;
        if (t + 1 < nstages) commit(t + 1, cur, cur_sq);
        if (t > 0) drain(t - 1, mask);
        __syncthreads();
    };
    fetch(0, pre_a, pre_sq_a);
    commit(0, pre_a, pre_sq_a);
    fetch(1, pre_b, pre_sq_b);
    __syncthreads();
    for (int t = 0; t < nstages; t += 2) {
        step(t, pre_a, pre_sq_a, pre_b, pre_sq_b);
        if (t + 1 < nstages) step(t + 1, pre_b, pre_sq_b, pre_a, pre_sq_a);
    }
    drain(nstages - 1, screen(nstages - 1));
    __syncthreads();  // every wave is done with the stage buffers

    // ---- the result from the log
    float2 *sel = reinterpret_cast<float2 *>(smem) + ct;          // [K][256] selected records below tau
    int *out = reinterpret_cast<int *>(smem + K * 256 * 8) + ct;  // [K][256] candidate of output slot o (-1: empty)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float tau = ld[0];
    int below = 0;  // list entries strictly below tau
#pragma unroll
    for (int s2 = 1; s2 < K; s2++) tau = (s2 == k - 1) ? ld[s2] : tau;
#pragma unroll
    for (int s2 = 0; s2 < K; s2++) {
        below += (s2 < k && ld[s2] < tau) ? 1 : 0;
        out[s2 * 256] = -1;
    }
    int nsel = 0, ties = below;  // ties: next output slot of a record equal to tau
    const int m = wave_max_nonneg(lcnt);
    // sixteen records in flight: the next eight are loaded before the current eight are looked at (one at a time, the
    // scan is a chain of memory round trips)
    float2 cur[8], nxt[8];
#pragma unroll
    for (int u = 0; u < 8; u++) cur[u] = log_load(logp + min(u, kLogCap - 1) * 256);
    for (int i0 = 0; i0 < m; i0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) nxt[u] = log_load(logp + min(i0 + 8 + u, kLogCap - 1) * 256);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (i0 + u < lcnt) {
                if (cur[u].x < tau) {
                    sel[nsel * 256] = cur[u];
                    nsel++;
                } else if (cur[u].x == tau && ties < k) {
                    out[ties * 256] = __float_as_int(cur[u].y);
                    ties++;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) cur[u] = nxt[u];
    }
    const int ms = wave_max_nonneg(nsel);
    for (int j = 0; j < ms; j++) {
        if (j < nsel) {
            const float2 e = sel[j * 256];
            int pos = 0;
#pragma unroll
            for (int s2 = 0; s2 < K; s2++) pos += ld[s2] < e.x ? 1 : 0;
            while (out[pos * 256] != -1) pos++;  // equal distances: the next free slot, in record (= candidate) order
            out[pos * 256] = __float_as_int(e.y);
        }
    }
    // `ties` slots are filled.  Fewer than k: the list holds finite distances only (nothing at +inf passes a strict
    // compare, in the screen or in the rounds), so the row continues with its +inf distances (see fill_inf_tail)
    if (ties < k)
        fill_inf_tail(
            ties, k, n, [&](int j) { return expanded_dist(xb, sqb, c, n, q, sq_q, j); },
            [&](int slot, int j) { out[slot * 256] = j; });
    // a wave writes the rows of its 64 queries with consecutive lanes on consecutive words
    __builtin_amdgcn_wave_barrier();
    const int wq = (w - 4) * 64;  // first local query of this wave
    const int q0 = blockIdx.x * kSplitQ + wq;
    const int *wout = reinterpret_cast<const int *>(smem + K * 256 * 8) + wq;
    int64_t *dst = indices + ((size_t)smp * n + q0) * k;
    const int total = min(64, n - q0) * k;
    for (int e = lane; e < total; e += 64) {
        const int ql = e / k, o = e - ql * k;
        const int v = wout[o * 256 + ql];
        dst[e] = (int64_t)((unsigned)v < (unsigned)n ? v : n - 1);  // (an empty slot: fewer than k distances that are not NaN)
    }
}

// padded channel counts of the instantiations
constexpr int kCPs[] = {8, 16, 32, 64, 128};

// f(std::integral_constant<int, CP>) for the smallest CP >= max(c, MinCP) (c <= 128); nothing below MinCP is instantiated
template <int MinCP, int I = 0, class F>
int with_cp(int c, F &&f) {
    if constexpr (kCPs[I] < MinCP) {
        return with_cp<MinCP, I + 1>(c, f);
    } else {
        if constexpr (I + 1 < (int)(sizeof kCPs / sizeof kCPs[0])) {
            if (c > kCPs[I]) return with_cp<MinCP, I + 1>(c, f);
        }
        return f(std::integral_constant<int, kCPs[I]>{});
    }
}

constexpr int cp_index(int CP) {
    int i = 0;
    for (int v : kCPs) i += v < CP;
    return i;
}
// the launch profile's names of the instantiations, [slot_index(K)][cp_index(CP)]: <K,CP,tiles per stage> and <K,CP>
static_assert(kTT128 == 1, "the profile names say one tile per stage at 128 channels");
const char *const kMfmaNames[][5] = {
    {"knn_mfma_kernel<4,8,1>", "knn_mfma_kernel<4,16,1>", "knn_mfma_kernel<4,32,1>", "knn_mfma_kernel<4,64,1>", "knn_mfma_kernel<4,128,1>"},
    {"knn_mfma_kernel<8,8,1>", "knn_mfma_kernel<8,16,1>", "knn_mfma_kernel<8,32,1>", "knn_mfma_kernel<8,64,1>", "knn_mfma_kernel<8,128,1>"},
    {"knn_mfma_kernel<16,8,1>", "knn_mfma_kernel<16,16,1>", "knn_mfma_kernel<16,32,1>", "knn_mfma_kernel<16,64,1>", "knn_mfma_kernel<16,128,1>"},
    {"knn_mfma_kernel<20,8,1>", "knn_mfma_kernel<20,16,1>", "knn_mfma_kernel<20,32,1>", "knn_mfma_kernel<20,64,1>", "knn_mfma_kernel<20,128,1>"},
    {"knn_mfma_kernel<25,8,1>", "knn_mfma_kernel<25,16,1>", "knn_mfma_kernel<25,32,1>", "knn_mfma_kernel<25,64,1>", "knn_mfma_kernel<25,128,1>"},
    {"knn_mfma_kernel<32,8,1>", "knn_mfma_kernel<32,16,1>", "knn_mfma_kernel<32,32,1>", "knn_mfma_kernel<32,64,1>", "knn_mfma_kernel<32,128,1>"}};
const char *const kSplitNames[][5] = {
    {"", "knn_mfma_split_kernel<4,16>", "knn_mfma_split_kernel<4,32>", "knn_mfma_split_kernel<4,64>", "knn_mfma_split_kernel<4,128>"},
    {"", "knn_mfma_split_kernel<8,16>", "knn_mfma_split_kernel<8,32>", "knn_mfma_split_kernel<8,64>", "knn_mfma_split_kernel<8,128>"},
    {"", "knn_mfma_split_kernel<16,16>", "knn_mfma_split_kernel<16,32>", "knn_mfma_split_kernel<16,64>", "knn_mfma_split_kernel<16,128>"},
    {"", "knn_mfma_split_kernel<20,16>", "knn_mfma_split_kernel<20,32>", "knn_mfma_split_kernel<20,64>", "knn_mfma_split_kernel<20,128>"},
    {"", "knn_mfma_split_kernel<25,16>", "knn_mfma_split_kernel<25,32>", "knn_mfma_split_kernel<25,64>", "knn_mfma_split_kernel<25,128>"},
    {"", "knn_mfma_split_kernel<32,16>", "knn_mfma_split_kernel<32,32>", "knn_mfma_split_kernel<32,64>", "knn_mfma_split_kernel<32,128>"}};

template <int K, int CP>
int launch_split(int b, int c, int n, int k, const float *x, const float *sq, int64_t *indices, hipStream_t st) {
    constexpr int lds = split_lds_bytes<K, CP>();
    if (const hipError_t attr = pcc::allow_lds<knn_mfma_split_kernel<K, CP>>(lds)) {
        pcc::set_error((int)attr, "knn: cannot reserve the role-split kernel's LDS");
        return (int)attr;
    }
    pcc::WsBlock logs(st);  // the selection waves' records (stream-ordered: freed behind the kernel)
    if (int rc = logs.alloc(split_log_bytes(b, n), "knn: workspace allocation failed")) return rc;
    pcc::ProfScope prof(kSplitNames[slot_index(K)][cp_index(CP)], st);
    hipLaunchKernelGGL((knn_mfma_split_kernel<K, CP>), dim3(pcc::ceil_div(n, kSplitQ), b), dim3(512), lds, st, c, n, k, x, sq,
                       reinterpret_cast<float2 *>(logs.p), indices);
    return PCC_OK;
}

template <int K>
int launch_mfma(int b, int c, int n, int k, const float *x, const float *sq, int64_t *indices, hipStream_t st) {
    // 256-query role-split workgroups (one per CU) once they fill three quarters of the chip; the 128-query kernel below
    // that (measured at n = 2048, k = 25: B = 32 c = 64 / 128: 286 / 417 us against 372 / 514; B = 16: 287 / 417 against 295 / 362)
    const int sw = pcc::tuning(PCC_TUNE_KNN_NOSPLIT);  // measurement switch: 1 = never, 2 = always
    // (and while the selection log -- 512 KB per workgroup -- stays a modest workspace)
    if (sw == 2 || (sw == 0 && (long long)pcc::ceil_div(n, kSplitQ) * b * 4 >= 3LL * pcc::device_cus() && split_log_bytes(b, n) <= (1ull << 30))) {
        return with_cp<16>(c, [&](auto CP) { return launch_split<K, CP>(b, c, n, k, x, sq, indices, st); });
    }
    const dim3 grid(pcc::ceil_div(n, 128), b);
    // two 32-candidate tiles (two accumulator chains) per stage while the double-buffered tiles leave room for two
    // workgroups per CU; 128 channels keep one
    return with_cp<8>(c, [&](auto CP) {
        pcc::ProfScope prof(kMfmaNames[slot_index(K)][cp_index(CP)], st);
        hipLaunchKernelGGL((knn_mfma_kernel<K, CP, (CP == 128 ? kTT128 : 1)>), grid, dim3(256), 0, st, c, n, k, x, sq, indices);
        return PCC_OK;
    });
}

}  // namespace

void pcc::launch_sqnorm(int b, int c, int n, const float *x, float *sq, hipStream_t st) {
    hipLaunchKernelGGL(sqnorm_kernel, dim3(pcc::ceil_div(n, 256), b), dim3(256), 0, st, c, n, x, sq);
}

int pcc::knn_mfma(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st) {
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc((size_t)b * n * sizeof(float), "knn: workspace allocation failed")) return rc;
    float *sq = static_cast<float *>(ws.p);
    pcc::launch_sqnorm(b, c, n, x, sq, st);
    if (int rc = pcc::check_launch("knn(sqnorm)")) return rc;
    if (int rc = with_slots(k, [&](auto K) { return launch_mfma<K>(b, c, n, k, x, sq, indices, st); })) return rc;
    return pcc::check_launch("knn(mfma)");
}

