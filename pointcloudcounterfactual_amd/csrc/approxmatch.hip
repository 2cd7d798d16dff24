// Approximate EMD (multi-scale soft matching) for gfx950 (MI355X), wave64.
//
// Replaces approxmatchkernel / matchcostkernel / matchcostgrad{1,2}kernel and their launchers
// (external/pytorch_structural_losses/src/approxmatch.cu:3-326).  Same recurrence, same outputs
// (match[b,m,n], temp[b,2(n+m)], cost[b], grad1, grad2); a different machine mapping:
//
//   reference                                   | here
//   --------------------------------------------+----------------------------------------------------
//   one 512-thread block per sample (32 blocks)  | every pass is a chip-wide launch: workgroup = 64*R
//   runs all 27 all-pairs passes serially        | owners x whole candidate cloud (SoA in LDS), S waves
//                                                | split the candidates, partial sums merged in LDS in a
//                                                | fixed order (deterministic)
//   pass C of level j and pass A of level j-1    | fused ("CA"): one distance evaluation feeds both
//   are separate sweeps                          | exponentials -> 19 launches instead of 27 sweeps
//   match zero-filled, then read-modify-written  | per-level ratio vectors (18(n+m) floats per sample)
//   once per level (9 x 1 GiB of traffic at      | are kept in a workspace and match is materialised by
//   B=32,N=2048)                                 | ONE write-only pass that re-evaluates the 9 levels in
//                                                | registers, summing them in the reference's order
//   exp via __expf(level*d2)                     | v_exp_f32((level*log2e)*d2): level is a power of 4, so
//                                                | the single rounded product is the same real number
//   matchcost re-reads match                     | pcc_approxmatch_cost: cost accumulated by the pass that writes match
//                                                | (stored match: matchcost.hip; never stored: am_pair.hip)
//   every pass evaluates all n*m pairs           | only terms that are not EXACTLY zero in float32: both clouds are
//                                                | Hilbert-sorted once per call (cloud_sort.hip); at the
//                                                | fine levels (64-owner group, 16-candidate block) pairs whose box
//                                                | distance makes every exp2(level*d2) underflow are skipped
//                                                | (V_CULL), and points whose capacity is used up drop out as
//                                                | candidates (V_CLIST) and as owners (V_COWN)
//   one stream, one block per sample             | a large batch runs as two half-batch lanes on two streams so
//                                                | that the dependent launch chains fill each other's bubbles
//
// Rooflines: the 19 phase launches and the materialise pass are f32-VALU / transcendental bound.
#include "approxmatch.hpp"
#include "pcc_test_hooks.h"
#include "wave_ops.hpp"

#include <algorithm>
#include <functional>
#include <mutex>
#include <type_traits>

namespace {

using pcc::sq3;
using pcc::WsView;

// ---------------------------------------------------------------------------------------------------
// Phase kernels: for every owner point o, S_c(o) = sum over candidates q of exp2(c_c * |o-q|^2) * w_c[q].
//   PH_A  (first level only): owners = set1, w0 = multiR (constant)      -> ratioL_0          (:29-62)
//   PH_B : owners = set2, w0 = ratioL_i                                  -> ratioR_i, remainR (:78-111)
//   PH_CA: owners = set1, w0 = ratioR_i, w1 = remainR, two exponents     -> remainL, ratioL_{i+1}
//          (pass C :130-163 without the match write, fused with pass A of the next level :29-62)
//   PH_C : last level, pass C only.
// ---------------------------------------------------------------------------------------------------
enum Phase { PH_A = 0, PH_B = 1, PH_CA = 2, PH_C = 3 };

// The per-owner recurrence of the passes (approxmatch.cu:37,61 / 106-109 / 154-162), shared by every pass kernel; each
// caller keeps its own stores.  Same operation order as the reference, nothing contracted (-ffp-contract=off).
//   pass A: ratioL = remainL / (1e-9 + sum_l e * remainR[l])
__device__ __forceinline__ float pass_a_ratio(float remL, float sum) { return remL / (1e-9f + sum); }
//   pass B: sumr = sum_k e * ratioL[k] * remainR ; ratioR = min(remainR / (sumr + 1e-9), 1) * remainR ;
//           remainR = max(0, remainR - sumr)
struct PassB {
    float ratio, remain;
};
__device__ __forceinline__ PassB pass_b(float remR, float sum) {
    const float sumr = sum * remR;
    const float consumption = __builtin_fminf(remR / (sumr + 1e-9f), 1.0f);
    return {consumption * remR, __builtin_fmaxf(0.0f, remR - sumr)};
}
//   pass C: remainL = max(0, remainL - sum_l e * ratioL[k] * ratioR[l])
__device__ __forceinline__ float pass_c_left(float remL, float ratioL, float sum) { return __builtin_fmaxf(0.0f, remL - ratioL * sum); }

struct PhaseArgs {
    int n_own, n_cand, tiles, batch;   // tiles = ceil(n_own / (64 R))
    int own_n4, cand_n4, own_nb, cand_nb;
    const float *own_soa, *cand_soa;   // [b][3][n4] Hilbert-sorted coordinates
    const float *cand_box;             // [b][nb][8] per 16 sorted candidates (min xyz, 0, max xyz, 0)
    const float *own_box16;            // [b][own_nb][8] per 16 sorted owners (am_fine_kernel)
    const float *w0, *w1;              // per-candidate weights in sorted order (w0 may be null => w0c)
    long long w0_stride, w1_stride;    // per-sample strides in floats
    float w0c;
    float c0, c1;
    float cut2;                        // skip a candidate block when its box is farther than sqrt(cut2)
    float cut2_fine;                   // pass C/A: the radius of the FINER of its two levels (am_fine_kernel: one exponential beyond it)
    int first;                         // first level: remain* still hold their initial constants
    int level;                         // 0..8 (host bookkeeping only)
    float multiL, multiR;
    // epilogue operands, all indexed [sample * stride + owner (sorted position)]
    float *remain;                     // remainL (CA/C, updated in place by its owner) or remainR before pass B
    float *remain_out;                 // pass B: remainR after the pass (a second buffer: other workgroups of the
                                       // launch still read `remain` to find the live owners)
    long long remain_stride;
    const float *ratio_in;             // CA/C: ratioL_i
    float *ratio_out;                  // A: ratioL_0 ; B: ratioR_i ; CA: ratioL_{i+1}
    long long ratio_stride;            // per-sample stride of the level arrays
    float *clist;                      // dense candidate list [b][5][cl_n4]: x | y | z | ratioR | remainR (V_COWN writes, V_CLIST reads)
    int *clist_cnt;                    // [b] entries in the list
    int cl_n4;
    const unsigned *mask_in;           // [b][kLevels][mask_words] bit o of row i: set2 point o is live entering pass B of level i (V_COWN)
    unsigned *mask_out;                // row i + 1 (pass B of level 2 writes row 3 whole; later ones clear the bits of the owners they exhaust)
    int mask_words;
    const int *live_in;                // [b] live owners (remain != 0) of this pass B, counted by the previous pass B (V_COWN)
    int *live_out;                     // [b] pass B: live owners of the next level's pass B (integer atomics: order-free)
};

// Work-skipping variants of a pass launch.  All of them only drop terms that are EXACTLY zero:
//   V_CULL  (levels 0-2, am_fine_kernel): a (16-owner group, 16-candidate block) pair is skipped when the box distance
//           makes every exp2(c*d2) underflow to 0;
//   V_COWN  (pass B from level 3 on): a query point whose capacity is used up has remainR == ratioR == 0 from then on
//           (approxmatch.cu:108-109; 54 % of them by level 3 and 95 % by level 8 on the bench clouds): its outputs are
//           ratioR = 0, remainR = 0 whatever the sum is, so only the live owners are gathered into tiles (the level
//           arrays are zero-filled beforehand) and workgroups beyond the live count leave at once;
//   V_CLIST (pass C/A from level 3 on): the same exhausted points as CANDIDATES: the live owners of the preceding
//           V_COWN pass B ARE the candidates with a non-zero weight (ratioR_i = consumption * remainR != 0 exactly for
//           them), so that pass writes their coordinates and new weights as a dense list and this one stages it with
//           straight float4 copies (no scan, no scattered LDS stores).
enum Var { V_PLAIN = 0, V_CULL = 1, V_COWN = 3, V_CLIST = 4 };

// Everything a pass needs is derived from this small description of one approxmatch call: the same function
// builds the arguments of pass p.
//   p = 0: pass A of level 0;  p = 1 + 2i: pass B of level i;  p = 2 + 2i: pass C of level i fused with pass A of
//   level i+1 (plain pass C for the last level).
struct Sched {
    int n, m, n4, m4, nb1, nb2;
    const float *soa1, *soa2, *box1, *box2;
    float *rem, *lv;               // sorted space: remain row = remainL(n4) | remainR ping(m4) | pong(m4); level rows
    float multiL, multiR;
    float *clist;                  // dense candidate list handed from pass B to pass C/A (null: pass C/A compacts itself)
    int *clist_cnt;
    int *live_cnt;                 // [b][kLiveRow] live set2 points entering pass B of level i (zeroed by the sort; i >= 1)
    unsigned *live_mask;           // [b][kLevels][ceil(m4 / 32)] live bits of set2 per level (rows 4.. preset to ones by the sort)
    int skip;                      // work-skipping variants enabled
    LevelConsts lc;
};

inline int sched_phases() { return 2 * kLevels + 1; }

inline PhaseArgs build_phase(const Sched &sc, int p, int *mode_out, int *var_out) {
    const long long nm4 = (long long)sc.n4 + sc.m4;
    const long long rs = (long long)sc.n4 + 2LL * sc.m4;
    PhaseArgs a{};
    a.multiL = sc.multiL;
    a.multiR = sc.multiR;
    const bool set1_owns = (p == 0) || (p % 2 == 0);
    if (set1_owns) {  // owners = set1, candidates = set2
        a.n_own = sc.n; a.n_cand = sc.m; a.own_n4 = sc.n4; a.cand_n4 = sc.m4; a.own_nb = sc.nb1; a.cand_nb = sc.nb2;
        a.own_soa = sc.soa1; a.cand_soa = sc.soa2; a.cand_box = sc.box2;
        a.own_box16 = sc.box1;
    } else {          // owners = set2, candidates = set1
        a.n_own = sc.m; a.n_cand = sc.n; a.own_n4 = sc.m4; a.cand_n4 = sc.n4; a.own_nb = sc.nb2; a.cand_nb = sc.nb1;
        a.own_soa = sc.soa2; a.cand_soa = sc.soa1; a.cand_box = sc.box1;
        a.own_box16 = sc.box2;
    }
    int mode, var;
    if (p == 0) {
        mode = PH_A;
        var = sc.skip ? V_CULL : V_PLAIN;
        a.level = 0;
        a.w0 = nullptr; a.w0c = sc.multiR; a.c0 = sc.lc.c[0]; a.first = 1;
        a.cut2 = zero_cut2(sc.lc, 0);
        a.ratio_out = sc.lv; a.ratio_stride = kLevels * nm4;
    } else {
        const int i = (p - 1) / 2;
        float *ratioL = sc.lv + (size_t)i * nm4, *ratioR = ratioL + sc.n4;
        a.level = i;
        a.first = (i == 0);
        a.c0 = sc.lc.c[i];
        if (p % 2 == 1) {  // pass B of level i
            mode = PH_B;
            // box culling while the zero radius is small against the cloud (levels 0-2), live-owner compaction after
            var = !sc.skip ? V_PLAIN : i <= 2 ? V_CULL : V_COWN;
            a.w0 = ratioL; a.w0_stride = kLevels * nm4;
            a.cut2 = zero_cut2(sc.lc, i);
            a.remain = sc.rem + sc.n4 + (i & 1) * sc.m4;
            a.remain_out = sc.rem + sc.n4 + ((i + 1) & 1) * sc.m4;
            a.remain_stride = rs;
            a.ratio_out = ratioR; a.ratio_stride = kLevels * nm4;
            if (var == V_COWN) { a.clist = sc.clist; a.clist_cnt = sc.clist_cnt; a.cl_n4 = sc.m4; }
            if (sc.live_mask) {
                const int words = mask_words(sc.m4);
                a.mask_words = words;
                if (i + 1 < kLevels && (var == V_COWN || i == 2)) a.mask_out = sc.live_mask + (size_t)(i + 1) * words;
                if (var == V_COWN) {
                    a.mask_in = sc.live_mask + (size_t)i * words;
                    // liveness comes from the mask, so remainR is updated IN PLACE by its owner from level 3 on (level 2
                    // left it in the second buffer): an exhausted owner holds 0 from the pass that exhausted it
                    a.remain = a.remain_out = sc.rem + sc.n4 + sc.m4;
                }
            }
            if (sc.live_cnt) {  // strided by kLiveRow ints per sample: the kernels index [smp * kLiveRow]
                a.live_in = (var == V_COWN && i >= 1) ? sc.live_cnt + i : nullptr;
                a.live_out = i + 1 < kLevels ? sc.live_cnt + i + 1 : nullptr;
            }
        } else {           // pass C of level i (+ pass A of level i+1)
            mode = i + 1 < kLevels ? PH_CA : PH_C;
            // (the cull radius is the one of level i+1); from level 3 on pass B has left the dense candidate list
            // (level 2: the (16 x 16) boxes still drop half of the pairs at level 3's radius, more than compacting away
            // the exhausted candidates did)
            var = !sc.skip ? V_PLAIN : i <= 2 ? V_CULL : V_CLIST;
            if (var == V_CLIST) { a.clist = sc.clist; a.clist_cnt = sc.clist_cnt; a.cl_n4 = sc.m4; }
            a.w0 = ratioR; a.w0_stride = kLevels * nm4;
            a.w1 = sc.rem + sc.n4 + ((i + 1) & 1) * sc.m4; a.w1_stride = rs;
            a.remain = sc.rem; a.remain_stride = rs;
            a.ratio_in = ratioL; a.ratio_stride = kLevels * nm4;
            const int lc_i = i + 1 < kLevels ? i + 1 : i;
            a.cut2 = zero_cut2(sc.lc, lc_i);  // the coarser of the two levels decides what is 0
            a.cut2_fine = zero_cut2(sc.lc, i);
            if (i + 1 < kLevels) {
                a.c1 = sc.lc.c[i + 1];
                a.ratio_out = sc.lv + (size_t)(i + 1) * nm4;
            }
        }
    }
    *mode_out = mode;
    *var_out = var;
    return a;
}

// LDS footprint of one phase (floats / ints)
template <int NW, int R, int S, int CH>
struct PhaseLds {
    static constexpr int kC = (3 + NW) * CH;          // x | y | z | w0 | (w1)
    static constexpr int kRed = NW * S * 64 * R;      // partial sums [NW][S][TQ]
    static constexpr int kOwn = 64 * R;               // live-owner tile (ints)
    static constexpr int kWave = S;                   // (ints)
    static constexpr int floats = kC + kRed + kOwn + kWave + 4;
};

// G > 1 (owner-compacted passes of the late levels only): a wave holds 64 / G owners, each on G lanes that split the
// 16-candidate blocks among them (G-fold shorter pair loop for the few live owners left; the partial sums of the G
// lanes meet through log2(G) shuffles, in a fixed order).
template <int MODE, int R, int S, int CH, int VAR, int G = 1>
__device__ __forceinline__ void am_phase_body(const PhaseArgs &a, int smp, int tile, float *smem) {
    constexpr int T = 64 * S;
    constexpr int TQ = 64 * R / G;     // owners per workgroup
    constexpr int PQ = 64 * R;         // pitch of the partial-sum rows in LDS
    static_assert(G == 1 || (VAR == V_COWN && R == 1), "lane-split owners: owner-compacted launches only");
    constexpr int NW = (MODE == PH_CA) ? 2 : 1;
    constexpr bool W0_CONST = (MODE == PH_A);
    constexpr bool COWN = VAR == V_COWN, CLIST = VAR == V_CLIST;
    static_assert(VAR == V_PLAIN || COWN || CLIST, "the box-culled passes run on am_fine_kernel");
    static_assert(!(CLIST && W0_CONST), "pass A of the first level has constant weights");
    static_assert(TQ <= T, "one epilogue owner per thread");
    using L = PhaseLds<NW, R, S, CH>;  // (four candidate rows for the single-weight passes: 36 KB, four workgroups per CU)
    float *lds_c = smem;                               // x | y | z | w0 | (w1)
    float *red = smem + L::kC;                         // [NW][S][TQ]
    int *own_idx = reinterpret_cast<int *>(red + L::kRed);
    int *wave_cnt = own_idx + L::kOwn;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sub = G > 1 ? lane / TQ : 0;  // which share of every candidate block this lane takes
    const float *O = a.own_soa + (size_t)smp * 3 * a.own_n4;
    const float *C = a.cand_soa + (size_t)smp * 3 * a.cand_n4;
    const float *W0 = W0_CONST ? nullptr : a.w0 + (size_t)smp * a.w0_stride;
    const float *W1 = (NW == 2) ? a.w1 + (size_t)smp * a.w1_stride : nullptr;

    // ---- which owners does this workgroup hold? ----
    if (!COWN && tile * TQ >= a.n_own) return;
    // Candidate staging, split in two: the loads of a chunk (one float4 group per thread and row: CH / 4 <= T) and its
    // LDS stores.  The owner-compacted passes issue the loads of the first chunk HERE, above their owner scan, whose
    // round trips they then share.
    static_assert(CH / 4 <= T, "one float4 group per thread and chunk");
    float4 st_x, st_y, st_z, st_0, st_1;
    auto stage_load = [&](const float *Cc, const float *W0c, const float *W1c, int pitch, int q0, int ngroups) {
        const int i = min(tid, max(ngroups - 1, 0));  // (clamped: every thread loads, only tid < ngroups stores)
        st_x = reinterpret_cast<const float4 *>(Cc + q0)[i];
        st_y = reinterpret_cast<const float4 *>(Cc + (size_t)pitch + q0)[i];
        st_z = reinterpret_cast<const float4 *>(Cc + (size_t)2 * pitch + q0)[i];
        st_0 = make_float4(a.w0c, a.w0c, a.w0c, a.w0c);
        st_1 = st_0;
        if (!W0_CONST) st_0 = *reinterpret_cast<const float4 *>(W0c + q0 + 4 * i);
        if (NW == 2) st_1 = *reinterpret_cast<const float4 *>(W1c + q0 + 4 * i);
    };
    if (COWN) stage_load(C, W0, W1, a.cand_n4, 0, (min(CH, a.n_cand) + 3) / 4);
    int n_valid = min(TQ, a.n_own - tile * TQ);  // owners of this tile (sorted positions tile*TQ ...)
    if (COWN) {
        // live owners of the sample, in order; this workgroup takes the tile-th group of TQ.  Liveness is one bit per
        // owner (row `level` of the mask: written whole by pass B of level 2, later rows = the row before with the bits of
        // the owners exhausted since cleared): a thread takes one 32-owner word -- one count, ONE block scan, and the set
        // bits of the word dealt to the tile's slots.  (Until round 3 every workgroup scanned the 2048 remainR floats, 16
        // per thread, and carried the zeros of the exhausted owners into the second remainR buffer: 3-4 us at the head of
        // each of the six passes, timed inside the kernel.)
        const int lo = tile * TQ, hi = lo + TQ;
        const unsigned *mk = a.mask_in + (size_t)smp * kLevels * a.mask_words;
        unsigned *mnext = (tile == 0 && a.mask_out) ? a.mask_out + (size_t)smp * kLevels * a.mask_words : nullptr;
        const int wpt = (a.mask_words + T - 1) / T;  // words per thread: 1 up to 32 T = 16384 points
        unsigned word = 0;
        int mine = 0;
        if (wpt == 1) {
            word = mk[min(tid, a.mask_words - 1)];
            word &= -(unsigned)(tid < a.mask_words);
            if (mnext && tid < a.mask_words) atomicAnd(&mnext[tid], word);  // the next row starts as this one (its preset is all ones)
            mine = __popc(word);
        } else {
            for (int j = tid * wpt; j < min(tid * wpt + wpt, a.mask_words); j++) {
                const unsigned wj = mk[j];
                if (mnext) atomicAnd(&mnext[j], wj);
                mine += __popc(wj);
            }
        }
        // exclusive scan of `mine` over the workgroup: wave scan + S-entry LDS scan
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            incl += lane >= off ? v : 0;
        }
        if (lane == 63) wave_cnt[w] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < S; i++) {
            const int c = __builtin_amdgcn_readfirstlane(wave_cnt[i]);  // (uniform: the S counts stay in scalar registers)
            before += i < w ? c : 0;
            total += c;
        }
        int pos = before + incl - mine - lo;  // slot of this thread's first live owner in the tile
        auto deal = [&](unsigned bits, int first_owner) {
            while (bits) {
                const int bit = __builtin_ctz(bits);
                bits &= bits - 1;
                if ((unsigned)pos < (unsigned)TQ) own_idx[pos] = first_owner + bit;
                pos++;
            }
        };
        if (wpt == 1) {
            deal(word, tid * 32);
        } else {
            for (int j = tid * wpt; j < min(tid * wpt + wpt, a.mask_words); j++) deal(mk[j], j * 32);
        }
        if (a.clist_cnt && tile == 0 && tid == 0) a.clist_cnt[smp] = total;  // pass C/A stages exactly the live owners
        n_valid = min(TQ, total - lo);
        if (n_valid <= 0) return;  // wave-uniform: nothing live in this tile
        (void)hi;
        __syncthreads();
    }
    int own_e = -1;  // sorted position of the owner this THREAD finishes in the epilogue
    if (tid < TQ && tid < n_valid) own_e = COWN ? own_idx[tid] : tile * TQ + tid;

    float ox[R], oy[R], oz[R], s0[R], s1[R];
    float t0x = 0.f, t1x = 0.f;  // second accumulators of the R == 1 shapes
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int e = G > 1 ? (lane & (TQ - 1)) : r * 64 + lane;
        int o = COWN ? own_idx[e < n_valid ? e : 0] : tile * TQ + e;
        o = o < a.n_own ? o : a.n_own - 1;
        ox[r] = O[o];
        oy[r] = O[a.own_n4 + o];
        oz[r] = O[2 * a.own_n4 + o];
        s0[r] = 0.f;
        s1[r] = 0.f;
    }
    // operands of the epilogue do not depend on the pair loop: fetch them now, behind the staging traffic
    // (for every thread, from a clamped index: issued with the owner coordinates above, one round trip for all)
    float pre_rem = 0.f, pre_ratio = 0.f;
    {
        const int oe = max(own_e, 0);
        if (MODE != PH_A && !a.first) pre_rem = a.remain[(size_t)smp * a.remain_stride + oe];
        if (MODE == PH_CA || MODE == PH_C) pre_ratio = a.ratio_in[(size_t)smp * a.ratio_stride + oe];
    }
    const float4 *X4 = reinterpret_cast<const float4 *>(lds_c);
    const float4 *Y4 = X4 + CH / 4;
    const float4 *Z4 = Y4 + CH / 4;
    const float4 *A4 = Z4 + CH / 4;
    const float4 *B4 = A4 + CH / 4;
    const float c0 = a.c0, c1 = a.c1;

    const int n_cand = CLIST ? __builtin_amdgcn_readfirstlane(a.clist_cnt[smp]) : a.n_cand;
    if (CLIST) {  // dense list of this sample: x | y | z | ratioR (w0) | remainR (w1), rows of cl_n4 floats
        C = a.clist + (size_t)smp * 5 * a.cl_n4;
        W0 = C + (size_t)3 * a.cl_n4;
        W1 = C + (size_t)4 * a.cl_n4;
    }
    const int cand_pitch = CLIST ? a.cl_n4 : a.cand_n4;
    for (int q0 = 0; q0 < n_cand; q0 += CH) {
        const int cnt = min(CH, n_cand - q0);
        int ngroups = (cnt + 3) / 4;
        if (q0) __syncthreads();
        {
            // sorted SoA rows and the weight rows are padded to a multiple of 4 (zeros): straight float4 copies
            float4 *dst4 = reinterpret_cast<float4 *>(lds_c);
            if (!(COWN && q0 == 0)) stage_load(C, W0, W1, cand_pitch, q0, ngroups);
            const int i = tid;
            if (i < ngroups) {
                float4 vx = st_x, vy = st_y, vz = st_z, v0 = st_0, v1 = st_1;
                if (CLIST && i * 4 + 3 >= cnt) {
                    // the dense list's tail is stale scratch: a padded candidate gets weight 0 below AND finite
                    // coordinates here (0 * exp2(NaN) would be NaN, not the exact 0 a padded candidate must add)
                    vx.y = i * 4 + 1 < cnt ? vx.y : 0.f; vx.z = i * 4 + 2 < cnt ? vx.z : 0.f; vx.w = 0.f;
                    vy.y = i * 4 + 1 < cnt ? vy.y : 0.f; vy.z = i * 4 + 2 < cnt ? vy.z : 0.f; vy.w = 0.f;
                    vz.y = i * 4 + 1 < cnt ? vz.y : 0.f; vz.z = i * 4 + 2 < cnt ? vz.z : 0.f; vz.w = 0.f;
                }
                if ((W0_CONST || CLIST) && i * 4 + 3 >= cnt) {  // padded candidates must weigh 0 (the list's tail is stale)
                    v0.x = i * 4 + 0 < cnt ? v0.x : 0.f;
                    v0.y = i * 4 + 1 < cnt ? v0.y : 0.f;
                    v0.z = i * 4 + 2 < cnt ? v0.z : 0.f;
                    v0.w = 0.f;
                    if (NW == 2) {
                        v1.x = i * 4 + 0 < cnt ? v1.x : 0.f;
                        v1.y = i * 4 + 1 < cnt ? v1.y : 0.f;
                        v1.z = i * 4 + 2 < cnt ? v1.z : 0.f;
                        v1.w = 0.f;
                    }
                }
                dst4[i] = vx;
                dst4[CH / 4 + i] = vy;
                dst4[2 * (CH / 4) + i] = vz;
                dst4[3 * (CH / 4) + i] = v0;
                if (NW == 2) dst4[4 * (CH / 4) + i] = v1;
            }
        }
        const int nblk = (ngroups + 3) / 4;  // blocks of 16 candidates (4 groups)
        __syncthreads();
        // the S waves take the 16-candidate blocks round-robin
        for (int blk = w; blk < nblk; blk += S) {
            const int g_end = min(blk * 4 + 4, ngroups);
            for (int g = blk * 4 + sub; g < g_end; g += G) {
                const float4 x = X4[g], y = Y4[g], z = Z4[g], wa = A4[g];
                float4 wb;
                if (NW == 2) wb = B4[g];
#pragma unroll
                for (int r = 0; r < R; r++) {
                    // (x2-x1)^2+(y2-y1)^2+(z2-z1)^2 with the oracle's rounding order (approxmatch.cu:54)
                    const float d0 = sq3(x.x - ox[r], y.x - oy[r], z.x - oz[r]);
                    const float d1 = sq3(x.y - ox[r], y.y - oy[r], z.y - oz[r]);
                    const float d2 = sq3(x.z - ox[r], y.z - oy[r], z.z - oz[r]);
                    const float d3 = sq3(x.w - ox[r], y.w - oy[r], z.w - oz[r]);
                    if (R == 1) {
                        // one owner per lane: a lone wave per SIMD would stall on a single dependent fma chain, so
                        // even and odd candidates go to two accumulators (added once, after the loop)
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d0), wa.x, s0[r]);
                        t0x = __builtin_fmaf(fast_exp2(c0 * d1), wa.y, t0x);
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d2), wa.z, s0[r]);
                        t0x = __builtin_fmaf(fast_exp2(c0 * d3), wa.w, t0x);
                        if (NW == 2) {
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d0), wb.x, s1[r]);
                            t1x = __builtin_fmaf(fast_exp2(c1 * d1), wb.y, t1x);
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d2), wb.z, s1[r]);
                            t1x = __builtin_fmaf(fast_exp2(c1 * d3), wb.w, t1x);
                        }
                    } else {
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d0), wa.x, s0[r]);
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d1), wa.y, s0[r]);
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d2), wa.z, s0[r]);
                        s0[r] = __builtin_fmaf(fast_exp2(c0 * d3), wa.w, s0[r]);
                        if (NW == 2) {
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d0), wb.x, s1[r]);
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d1), wb.y, s1[r]);
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d2), wb.z, s1[r]);
                            s1[r] = __builtin_fmaf(fast_exp2(c1 * d3), wb.w, s1[r]);
                        }
                    }
                }
            }
        }
    }
    if (R == 1) {
        s0[0] += t0x;
        s1[0] += t1x;
    }
    if (G > 1) {  // the G lanes of an owner: a + b is the same float on both sides, so all of them end with the same sum
        s0[0] += __shfl_xor(s0[0], TQ, 64);
        if (G == 4) s0[0] += __shfl_xor(s0[0], 2 * TQ, 64);
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        red[(0 * S + w) * PQ + r * 64 + lane] = s0[r];
        if (NW == 2) red[(1 * S + w) * PQ + r * 64 + lane] = s1[r];
    }
    __syncthreads();
    if (own_e < 0) return;
    {
        const int e = tid;
        const int o = own_e;
        float t0 = red[e], t1 = 0.f;
        if (NW == 2) t1 = red[(1 * S) * PQ + e];
#pragma unroll
        for (int s = 1; s < S; s++) {
            t0 += red[(0 * S + s) * PQ + e];
            if (NW == 2) t1 += red[(1 * S + s) * PQ + e];
        }
        if (MODE == PH_A) {
            a.ratio_out[(size_t)smp * a.ratio_stride + o] = pass_a_ratio(a.multiL, t0);  // (remainL == multiL)
        } else if (MODE == PH_B) {
            const PassB pb = pass_b(a.first ? a.multiR : pre_rem, t0);
            const float ratio_new = pb.ratio, remain_new = pb.remain;
            a.ratio_out[(size_t)smp * a.ratio_stride + o] = ratio_new;
            a.remain_out[(size_t)smp * a.remain_stride + o] = remain_new;
            if (a.live_out) {  // owners still live after this level = the owner count of the next pass B
                const unsigned long long alive = __ballot(remain_new != 0.f);
                if (lane == 0) atomicAdd(&a.live_out[(size_t)smp * kLiveRow], (int)__popcll(alive));
            }
            if (COWN && a.mask_out && remain_new == 0.f)  // exhausted here: not an owner from the next level on
                atomicAnd(&a.mask_out[(size_t)smp * kLevels * a.mask_words + (o >> 5)], ~(1u << (o & 31)));
            if (COWN && a.clist) {
                // this owner is the (tile * TQ + e)-th live one of its sample == its place in the next pass's candidate list
                float cx = ox[0], cy = oy[0], cz = oz[0];  // thread e = w * 64 + lane holds owner e in slot r = w
#pragma unroll
                for (int r = 1; r < R; r++) {
                    cx = w == r ? ox[r] : cx;
                    cy = w == r ? oy[r] : cy;
                    cz = w == r ? oz[r] : cz;
                }
                float *cl = a.clist + (size_t)smp * 5 * a.cl_n4 + tile * TQ + e;
                cl[0] = cx;
                cl[(size_t)a.cl_n4] = cy;
                cl[(size_t)2 * a.cl_n4] = cz;
                cl[(size_t)3 * a.cl_n4] = ratio_new;
                cl[(size_t)4 * a.cl_n4] = remain_new;
            }
        } else {
            const float left = pass_c_left(a.first ? a.multiL : pre_rem, pre_ratio, t0);
            a.remain[(size_t)smp * a.remain_stride + o] = left;
            if (MODE == PH_CA) a.ratio_out[(size_t)smp * a.ratio_stride + o] = pass_a_ratio(left, t1);  // pass A of the next level
        }
    }
}

template <int MODE, int R, int S, int CH, int VAR, int G = 1>
__global__ __launch_bounds__(64 * S) void am_phase_kernel(PhaseArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[PhaseLds<(MODE == PH_CA ? 2 : 1), R, S, CH>::floats];
    // V_COWN packs the live owners into the low tiles: dispatch those first (tile-major order), so the workgroups
    // that have nothing to do and exit after the scan are not in front of the ones that carry the launch
    constexpr bool COWN = VAR == V_COWN;
    // XCD affinity (cdna_hip_programming.md T1): blocks with equal blockIdx % 8 share an XCD and its L2.  All workgroups
    // of a sample stage the same candidate cloud at the same moment, so a sample's workgroups are given block ids of one
    // residue class: its cloud crosses the fabric once per launch instead of once per XCD (a pure speed choice).
    int smp, tile;
    const int bid = (int)blockIdx.x, nwg = (int)gridDim.x;
    if (COWN) {
        if (a.batch % 8 == 0) {  // samples congruent to the XCD label, tile-major inside the class
            const int per = a.batch / 8, i = bid / 8;
            smp = (bid % 8) + 8 * (i % per);
            tile = i / per;
        } else {
            smp = bid % a.batch;
            tile = bid / a.batch;
        }
        // the previous pass B counted the owners that are still live: workgroups beyond them leave at once (tile 0
        // stays: it carries the zeros of the exhausted owners into the output buffer)
        if (a.live_in && tile > 0 && tile * (64 * R / G) >= a.live_in[(size_t)smp * kLiveRow]) return;
    } else {
        const int lid = pcc::xcd_contiguous(bid, nwg);  // the blocks of one residue class get a contiguous run of logical ids
        smp = lid / a.tiles;
        tile = lid - smp * a.tiles;
    }
    am_phase_body<MODE, R, S, CH, VAR, G>(a, smp, tile, smem);
}

// ---------------------------------------------------------------------------------------------------
// Fine-grained culling for the passes of the fine levels (0-2, where the kernel radius is small against the cloud).
// am_phase_kernel's V_CULL tests (64-owner group, 16-candidate block) pairs of boxes; on Hilbert-sorted clouds a run of
// 64 points is several kernel radii wide, and 75-80 % of the pairs it keeps are still exact zeros.  Here a workgroup
// still owns 64 consecutive sorted owners and stages the candidate cloud once, but the owners are tested and walked in
// four groups of 16: a wave holds ONE group, each owner on 4 lanes that take one float4 (4 candidates) of every
// surviving 16-candidate block, and two waves share the block list of a group.  Measured on the bench clouds the
// (16 x 16) boxes keep 10 / 14 / 23 % of the pairs at levels 0 / 1 / 2 instead of 22 / 25 / 37 %.  Same sums as everywhere
// else in this file: only exact zeros are dropped, partial sums meet in a fixed order (two accumulators per lane,
// shuffles over the 4 lanes of an owner, the two waves of a group in LDS).
// ---------------------------------------------------------------------------------------------------
constexpr int kFineS = 8;                // waves per workgroup
constexpr int kFineOG = 16;              // owners per culling group (== kBox: the sort's 16-point boxes serve both sides)
constexpr int kFineGroups = 64 / kFineOG;
constexpr int kFineQ = 4;                // owners per lane

// The steps of a fine-level pass, one copy for am_fine_kernel (one launch per pass) and am_fine_persist_kernel (levels
// 0-2 in one launch).  The two kernels keep their own LDS layouts and hand in the row base pointers.  Thread
// (tg, tb) = (tid / NBLK, tid % NBLK) holds the test of owner group tg of the tile against candidate block tb; wave w
// walks the block list of group og = w % kFineGroups, share cs = w / kFineGroups of it; lane = (candidate cl of a block,
// owner quad).
struct FineOwners {  // the kFineQ owners of a lane: group-local 4 quad .. 4 quad + 3
    float x[kFineQ], y[kFineQ], z[kFineQ];
};
struct FineRows {  // LDS rows of the staged candidates: coordinates, weights of the first / second exponential
    const float *x, *y, *z, *w0, *w1;
};

// bounding box of 16-owner group g16 of sample smp (an empty box beyond the cloud: it is near no block)
__device__ __forceinline__ void fine_group_box(const float *own_box, int own_nb, int smp, int g16, float4 &lo, float4 &hi) {
    lo = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.f);
    hi = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), 0.f);
    if (g16 < own_nb) {
        const float4 *ob = reinterpret_cast<const float4 *>(own_box + ((size_t)smp * own_nb + g16) * 8);
        lo = ob[0];
        hi = ob[1];
    }
}

// squared distance between a group's box and the box of a candidate block (cand_box points at its 8 floats)
__device__ __forceinline__ float fine_box_d2(const float4 &glo, const float4 &ghi, const float *cand_box) {
    const float4 *cb = reinterpret_cast<const float4 *>(cand_box);
    const float4 lo = cb[0], hi = cb[1];
    const float dx = fmaxf(fmaxf(glo.x - hi.x, lo.x - ghi.x), 0.f);
    const float dy = fmaxf(fmaxf(glo.y - hi.y, lo.y - ghi.y), 0.f);
    const float dz = fmaxf(fmaxf(glo.z - hi.z, lo.z - ghi.z), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

// The surviving blocks of every group, compacted in block order into items[group][] (bit 7: outer_only, the finer level
// of pass C/A is exactly 0 for the whole pair of boxes) and flagged in need[]: the two waves 2 tg and 2 tg + 1 hold the
// tests of group tg, wave_cnt[] their counts.  need[] must be free (the previous chunk / pass has staged); ends with a
// barrier behind which the lists are complete.
template <int NBLK>
__device__ __forceinline__ void fine_block_list(bool keep, bool outer_only, int tid, int tg, int tb, int w, int lane,
                                                int *wave_cnt, unsigned char (*items)[NBLK], unsigned char *need) {
    if (tid < NBLK) need[tid] = 0;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_cnt[w] = __popcll(bal);
    __syncthreads();
    const int before = (w & 1) ? wave_cnt[w - 1] : 0;
    if (keep) {
        items[tg][before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned char)(tb | (outer_only ? 128 : 0));  // (tb < 128)
        need[tb] = 1;  // (same value from every writer)
    }
    __syncthreads();
}

// A wave walks its half (cs) of its group's block list (nitems entries): a lane holds ONE candidate of the block (five
// scalar LDS reads, 16 distinct addresses per wave) against its four owners in registers -- four independent fma chains.
template <int NW>
__device__ __forceinline__ void fine_walk(const FineRows &rows, const unsigned char *list, int nitems, int cs, int cl, float c0,
                                          float c1, const FineOwners &own, float (&s0)[kFineQ], float (&s1)[kFineQ]) {
    for (int it = cs; it < nitems; it += 2) {
        const int item = __builtin_amdgcn_readfirstlane((int)list[it]);
        const int ci = (item & 127) * kBox + cl;
        const float x = rows.x[ci], y = rows.y[ci], z = rows.z[ci];
        if (NW == 2 && (item & 128)) {  // (wave-uniform) beyond the finer level's radius: its terms are exact zeros
            const float wb = rows.w1[ci];
#pragma unroll
            for (int j = 0; j < kFineQ; j++) s1[j] = __builtin_fmaf(fast_exp2(c1 * sq3(x - own.x[j], y - own.y[j], z - own.z[j])), wb, s1[j]);
            continue;
        }
        const float wa = rows.w0[ci];
        float wb = 0.f;
        if (NW == 2) wb = rows.w1[ci];
#pragma unroll
        for (int j = 0; j < kFineQ; j++) {
            const float d = sq3(x - own.x[j], y - own.y[j], z - own.z[j]);
            s0[j] = __builtin_fmaf(fast_exp2(c0 * d), wa, s0[j]);
            if (NW == 2) s1[j] = __builtin_fmaf(fast_exp2(c1 * d), wb, s1[j]);
        }
    }
}

// the 16 candidate lanes of an owner meet through four butterfly steps (a + b is the same float on both sides, so every
// lane ends with the same sum); lane cl == 0 of each quad hands the four sums to red[exponential][cs][group-local owner]
template <int NW>
__device__ __forceinline__ void fine_reduce(float (&s0)[kFineQ], float (&s1)[kFineQ], float (*red)[2][64], int cs, int cl, int og, int quad) {
    const auto add = [](float a, float b) { return a + b; };
#pragma unroll
    for (int j = 0; j < kFineQ; j++) {
        s0[j] = pcc::row_reduce16(s0[j], add);
        if (NW == 2) s1[j] = pcc::row_reduce16(s1[j], add);
    }
    if (cl == 0) {
#pragma unroll
        for (int j = 0; j < kFineQ; j++) {
            red[0][cs][og * kFineOG + quad * kFineQ + j] = s0[j];
            if (NW == 2) red[1][cs][og * kFineOG + quad * kFineQ + j] = s1[j];
        }
    }
}

template <int MODE, int CH>
// (<= 64 VGPRs for passes A and B: with their 34 KB of LDS four workgroups -- the 2 x 512 of the two half-batch lanes --
// then fit a CU together; at 70 VGPRs three fitted, a quarter of every launch's workgroups waited for a slot, and these
// launches are bound by a workgroup's own critical path: 445 -> 439 us per match_cost call, A/B across library builds.
// Pass C/A keeps its 81 registers and 43 KB -- three per CU: its second weight row read from global memory instead of
// LDS, to fit four, measured 454 us.)
__global__ __launch_bounds__(64 * kFineS, MODE == PH_CA ? 4 : 8) void am_fine_kernel(PhaseArgs a) {
    constexpr int T = 64 * kFineS;
    constexpr int NW = (MODE == PH_CA) ? 2 : 1;
    constexpr bool W0_CONST = (MODE == PH_A);
    constexpr int NBLK = CH / kBox;      // candidate blocks per staged chunk
    static_assert(kFineGroups * NBLK == T, "one (owner group, candidate block) box test per thread");
    static_assert(kFineOG == kBox && kFineOG * kFineQ == 64, "a wave = 16 candidates x 4 owner quads");
    __shared__ __attribute__((aligned(16))) float lds_c[(3 + NW) * CH];  // x | y | z | w0 | (w1)
    __shared__ float red[NW][2][64];
    __shared__ unsigned char items[kFineGroups][NBLK];
    __shared__ unsigned char need[NBLK];
    __shared__ int wave_cnt[kFineS];

    const int lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);  // a sample's workgroups share an XCD (see am_phase_kernel)
    const int smp = lid / a.tiles;
    const int tile = lid - smp * a.tiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int og = w & (kFineGroups - 1);      // owner group of this wave
    const int cs = w / kFineGroups;            // its share of the group's block list (0 / 1)
    const int cl = lane & (kBox - 1);          // the candidate of a block this lane holds
    const int quad = lane / kBox;              // its four owners: group-local 4 quad .. 4 quad + 3
    const float *O = a.own_soa + (size_t)smp * 3 * a.own_n4;
    const float *C = a.cand_soa + (size_t)smp * 3 * a.cand_n4;
    const float *W0 = W0_CONST ? nullptr : a.w0 + (size_t)smp * a.w0_stride;
    const float *W1 = (NW == 2) ? a.w1 + (size_t)smp * a.w1_stride : nullptr;

    FineOwners own;
    float s0[kFineQ], s1[kFineQ];
#pragma unroll
    for (int j = 0; j < kFineQ; j++) {
        int o = tile * 64 + og * kFineOG + quad * kFineQ + j;
        o = o < a.n_own ? o : a.n_own - 1;
        own.x[j] = O[o];
        own.y[j] = O[a.own_n4 + o];
        own.z[j] = O[2 * a.own_n4 + o];
        s0[j] = 0.f;
        s1[j] = 0.f;
    }
    // epilogue operands (thread e < 64 finishes owner tile * 64 + e): fetched now, behind the staging traffic
    const int own_e = (tid < 64 && tile * 64 + tid < a.n_own) ? tile * 64 + tid : -1;
    // (for every thread, from a clamped index: issued with the owner coordinates above, one round trip for all)
    float pre_rem = 0.f, pre_ratio = 0.f;
    {
        const int oe = max(own_e, 0);
        if (MODE != PH_A && !a.first) pre_rem = a.remain[(size_t)smp * a.remain_stride + oe];
        if (MODE == PH_CA || MODE == PH_C) pre_ratio = a.ratio_in[(size_t)smp * a.ratio_stride + oe];
    }
    // box of the owner group this THREAD tests
    const int tg = tid / NBLK, tb = tid - tg * NBLK;
    float4 glo, ghi;
    fine_group_box(a.own_box16, a.own_nb, smp, tile * kFineGroups + tg, glo, ghi);
    const float c0 = a.c0, c1 = a.c1, cut2 = a.cut2;
    const FineRows rows = {lds_c, lds_c + CH, lds_c + 2 * CH, lds_c + 3 * CH, lds_c + 4 * CH};

    for (int q0 = 0; q0 < a.n_cand; q0 += CH) {
        const int cnt = min(CH, a.n_cand - q0);
        const int ngroups = (cnt + 3) / 4;
        const int nblk = (ngroups + 3) / 4;
        if (q0) __syncthreads();
        bool keep = false, outer_only = false;
        if (tb < nblk) {
            const float bd2 = fine_box_d2(glo, ghi, a.cand_box + ((size_t)smp * a.cand_nb + q0 / kBox + tb) * 8);
            keep = !(bd2 > cut2);  // farther: every exponential of the pair of boxes is exactly 0
            // pass C/A walks the radius of the COARSER level; between the two radii the finer level's exponential is
            // exactly 0 for the whole pair of boxes: such a block is marked and costs one exponential, not two
            outer_only = NW == 2 && bd2 > a.cut2_fine;
        }
        fine_block_list<NBLK>(keep, outer_only, tid, tg, tb, w, lane, wave_cnt, items, need);
        {   // stage the blocks some group of this workgroup needs (on the fine levels a fraction of the cloud): the sorted
            // SoA rows and weight rows are padded to a multiple of 4 (zeros), so these are straight float4 copies
            float4 *dst4 = reinterpret_cast<float4 *>(lds_c);
            const float4 *sx = reinterpret_cast<const float4 *>(C + q0);
            const float4 *sy = reinterpret_cast<const float4 *>(C + (size_t)a.cand_n4 + q0);
            const float4 *sz = reinterpret_cast<const float4 *>(C + (size_t)2 * a.cand_n4 + q0);
            // (one float4 group per thread, no loop: as a loop over i += T every row pointer became a 64-bit induction
            // variable in a VGPR pair, hoisted out of the chunk loop -- most of what pass A / B spilled)
            static_assert(CH / 4 <= T, "one float4 group per thread and chunk");
            const int i = tid;
            if (i < nblk * 4 && need[i >> 2]) {
                float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx, vz = vx, v0 = vx, v1 = vx;
                if (i < ngroups) {
                    vx = sx[i]; vy = sy[i]; vz = sz[i];
                    v0 = W0_CONST ? make_float4(a.w0c, a.w0c, a.w0c, a.w0c) : *reinterpret_cast<const float4 *>(W0 + q0 + 4 * i);
                    if (NW == 2) v1 = *reinterpret_cast<const float4 *>(W1 + q0 + 4 * i);
                    if (W0_CONST && i * 4 + 3 >= cnt) {  // padded candidates must weigh 0
                        v0.x = i * 4 + 0 < cnt ? v0.x : 0.f;
                        v0.y = i * 4 + 1 < cnt ? v0.y : 0.f;
                        v0.z = i * 4 + 2 < cnt ? v0.z : 0.f;
                        v0.w = 0.f;
                    }
                }
                dst4[i] = vx;
                dst4[CH / 4 + i] = vy;
                dst4[2 * (CH / 4) + i] = vz;
                dst4[3 * (CH / 4) + i] = v0;
                if (NW == 2) dst4[4 * (CH / 4) + i] = v1;
            }
        }
        __syncthreads();
        fine_walk<NW>(rows, items[og], wave_cnt[2 * og] + wave_cnt[2 * og + 1], cs, cl, c0, c1, own, s0, s1);
    }
    fine_reduce<NW>(s0, s1, red, cs, cl, og, quad);
    __syncthreads();
    if (own_e < 0) return;
    const float sum0 = red[0][0][tid] + red[0][1][tid];
    const float sum1 = NW == 2 ? red[NW - 1][0][tid] + red[NW - 1][1][tid] : 0.f;
    if (MODE == PH_A) {
        a.ratio_out[(size_t)smp * a.ratio_stride + own_e] = pass_a_ratio(a.multiL, sum0);  // (remainL == multiL)
    } else if (MODE == PH_B) {
        const PassB pb = pass_b(a.first ? a.multiR : pre_rem, sum0);
        a.ratio_out[(size_t)smp * a.ratio_stride + own_e] = pb.ratio;
        a.remain_out[(size_t)smp * a.remain_stride + own_e] = pb.remain;
        if (a.live_out) {  // owners still live after this level = the owner count of the next pass B
            const unsigned long long alive = __ballot(pb.remain != 0.f);
            if (lane == 0) atomicAdd(&a.live_out[(size_t)smp * kLiveRow], (int)__popcll(alive));
            if (a.mask_out && lane == 0) {  // ... and their bits: this tile's 64 owners are two whole words of the next row
                unsigned *mo = a.mask_out + (size_t)smp * kLevels * a.mask_words;
                if (2 * tile < a.mask_words) mo[2 * tile] = (unsigned)alive;
                if (2 * tile + 1 < a.mask_words) mo[2 * tile + 1] = (unsigned)(alive >> 32);
            }
        }
    } else {
        const float left = pass_c_left(a.first ? a.multiL : pre_rem, pre_ratio, sum0);
        a.remain[(size_t)smp * a.remain_stride + own_e] = left;
        if (MODE == PH_CA) a.ratio_out[(size_t)smp * a.ratio_stride + own_e] = pass_a_ratio(left, sum1);  // pass A of the next level
    }
}

// ---------------------------------------------------------------------------------------------------
// The seven passes of the fine levels (A0 B0 CA0 B1 CA1 B2 CA2) as ONE resident launch.
// On am_fine_kernel these passes are bound by their fixed costs -- a dependent launch (~5 us of gap plus a cold L2:
// the producer ran on other XCDs) and ~5 us of workgroup prologue for 1-4 us of arithmetic -- 97 us of each lane's
// chain at B=32, N=2048.  Here a workgroup keeps tile t of BOTH clouds (64 + 64 owners) for all seven passes:
//   * the two sorted clouds are staged in LDS once (coordinates never change), the (16-owner group, 16-candidate block)
//     box distances are computed once and kept in a register per direction -- the balls of the levels nest, so a pass
//     only compares that distance with its own radius;
//   * an owner's running state (remainL, ratioL_i, remainR) stays in the register of the thread that finishes it;
//   * per pass only the weights of the blocks some group needs are re-read (agent-scope loads: written by other
//     workgroups during this launch) and one or two values per owner are written (agent-scope stores);
//   * a pass boundary is a per-SAMPLE barrier (one counter per sample in the live-counter row; tiles of a sample get
//     consecutive block ids of one XCD): no launch, no cache-wide fence.
// The box test, block lists, pair walk, reductions and epilogue formulas are am_fine_kernel's (the same helpers): the
// level rows carry the same bits as with one launch per pass (tests/test_gpu_structural.py::test_resident_fine_levels_equal_one_launch_per_pass).
// Residency: a sample's barrier needs its `tiles` workgroups resident together, and the hardware does NOT dispatch
// workgroups strictly in block-id order (measured: a launch of more workgroups than the chip holds leaves samples
// half-resident for milliseconds -- B=32 as two 512-workgroup lanes ran 4 ms per call, with barrier time-outs).  So, like
// the auction's cluster kernel, the host uses this form only when the WHOLE launch fits the device with room to spare
// (batch x tiles <= compute units while two workgroups fit a CU: b <= 8 at N = 2048, the reference's default
// per-device batch, default_train.yaml:6), and a pcc::CoresidentGate keeps every other co-resident launch off the device
// meanwhile.  Spins are bounded all the same: a barrier that times out raises the sample's error slot (the
// finish and unpermute kernels then report NaN for the sample) and a sticky host word (the next call on the device fails) instead
// of hanging.  Measured (N=2048, b=8): 68 us against 91 us for the seven launches -- the passes are bound by the
// latency of one workgroup's own work (list, weights, walk, reduction: ~10 us), not by the launch boundary.
// ---------------------------------------------------------------------------------------------------
constexpr int kFpPasses = 7;   // A0 B0 CA0 B1 CA1 B2 CA2
constexpr int kFpCH = 2048;    // largest cloud the resident form takes

struct FinePersistArgs {
    int n, m, n4, m4, nb1, nb2, tiles;
    const float *soa1, *soa2, *box1, *box2;
    float *rem, *lv;               // sorted space (see Sched)
    float multiL, multiR;
    float c[4], cut2[4];           // levels 0..3
    int *live_cnt;                 // [b][kLiveRow]
    unsigned *live_mask;           // [b][kLevels][mask_words] (row 3 is written here: PhaseArgs::mask_out)
    int mask_words;
    unsigned *host_err;            // sticky word in mapped host memory (pcc::CoresidentGate)
    int inject;                    // test hook: every sample fails at its first barrier
};

__global__ __launch_bounds__(64 * kFineS) void am_fine_persist_kernel(FinePersistArgs a) {
    constexpr int T = 64 * kFineS, CH = kFpCH, NBLK = CH / kBox;
    static_assert(kFineGroups * NBLK == T, "one (owner group, candidate block) box test per thread and direction");
    __shared__ __attribute__((aligned(16))) float lds_p[2][3 * CH];  // sorted coordinates x | y | z of set1, set2
    __shared__ __attribute__((aligned(16))) float lds_w[2][CH];      // w0 | w1 of the current pass
    __shared__ float red[2][2][64];
    __shared__ unsigned char items[kFineGroups][NBLK];
    __shared__ unsigned char need[NBLK];
    __shared__ int wave_cnt[kFineS];

    const int lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int smp = lid / a.tiles;
    const int tile = lid - smp * a.tiles;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int og = w & (kFineGroups - 1), cs = w / kFineGroups;
    const int cl = lane & (kBox - 1), quad = lane / kBox;
    const long long nm4 = (long long)a.n4 + a.m4, rs = (long long)a.n4 + 2LL * a.m4;
    const float *S1 = a.soa1 + (size_t)smp * 3 * a.n4;
    const float *S2 = a.soa2 + (size_t)smp * 3 * a.m4;
    float *LV = a.lv + (size_t)smp * kLevels * nm4;
    float *REM = a.rem + (size_t)smp * rs;
    int *row = a.live_cnt + (size_t)smp * kLiveRow;
    unsigned *bar = reinterpret_cast<unsigned *>(row + kBarSlot);
    unsigned *err = reinterpret_cast<unsigned *>(row + kErrSlot);

    // ---- once: both clouds into LDS (rows are padded to a multiple of 4 with zeros; beyond that zeros: a padded
    // candidate sits at the origin with weight 0) ----
    for (int s = 0; s < 2; s++) {
        const float *S = s ? S2 : S1;
        const int p4 = s ? a.m4 : a.n4, ngroups = p4 / 4, nblk = (ngroups + 3) / 4;
        float4 *dst4 = reinterpret_cast<float4 *>(lds_p[s]);
        const float4 *sx = reinterpret_cast<const float4 *>(S);
        const float4 *sy = reinterpret_cast<const float4 *>(S + p4);
        const float4 *sz = reinterpret_cast<const float4 *>(S + 2 * (size_t)p4);
        for (int i = tid; i < nblk * 4; i += T) {
            float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx, vz = vx;
            if (i < ngroups) { vx = sx[i]; vy = sy[i]; vz = sz[i]; }
            dst4[i] = vx;
            dst4[CH / 4 + i] = vy;
            dst4[2 * (CH / 4) + i] = vz;
        }
    }
    // ---- once: this lane's owners of both roles, and the box distance of its (group, block) test per direction ----
    FineOwners set1, set2;
#pragma unroll
    for (int j = 0; j < kFineQ; j++) {
        const int o = tile * 64 + og * kFineOG + quad * kFineQ + j;
        const int o1 = min(o, a.n - 1), o2 = min(o, a.m - 1);
        set1.x[j] = S1[o1]; set1.y[j] = S1[a.n4 + o1]; set1.z[j] = S1[2 * a.n4 + o1];
        set2.x[j] = S2[o2]; set2.y[j] = S2[a.m4 + o2]; set2.z[j] = S2[2 * a.m4 + o2];
    }
    const int tg = tid / NBLK, tb = tid - tg * NBLK;
    auto box_d2 = [&](const float *own_box, int own_nb, const float *cand_box, int cand_nb) -> float {
        float4 glo, ghi;
        fine_group_box(own_box, own_nb, smp, tile * kFineGroups + tg, glo, ghi);
        if (tb >= cand_nb) return __builtin_inff();
        return fine_box_d2(glo, ghi, cand_box + ((size_t)smp * cand_nb + tb) * 8);
    };
    const float d2_role0 = box_d2(a.box1, a.nb1, a.box2, a.nb2);  // set1 owners against set2 candidate blocks
    const float d2_role1 = box_d2(a.box2, a.nb2, a.box1, a.nb1);  // set2 owners against set1 candidate blocks
    // running state of the owner thread e < 64 finishes in each role
    const int own1 = (tid < 64 && tile * 64 + tid < a.n) ? tile * 64 + tid : -1;
    const int own2 = (tid < 64 && tile * 64 + tid < a.m) ? tile * 64 + tid : -1;
    float remL = 0.f, ratL = 0.f, remR = 0.f;
    unsigned arrivals = 0;
    bool ok = true;

    // one pass: MODE decides the role (A / CA: set1 owners, B: set2 owners); i = level
    auto pass = [&](auto mode_tag, int i) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int NW = MODE == PH_CA ? 2 : 1;
        constexpr int ROLE = MODE == PH_B ? 1 : 0;
        const int n_cand = ROLE ? a.n : a.m, cand_n4 = ROLE ? a.n4 : a.m4;
        const int nblk = (cand_n4 / 4 + 3) / 4;
        const float c0 = a.c[i], c1 = a.c[MODE == PH_CA ? i + 1 : i];
        const float cut2 = a.cut2[MODE == PH_CA ? i + 1 : i];  // the coarser of the two levels decides what is 0
        const float *P = lds_p[ROLE ? 0 : 1];
        const float bd2 = ROLE ? d2_role1 : d2_role0;
        const bool keep = tb < nblk && !(bd2 > cut2);
        const bool outer_only = NW == 2 && bd2 > a.cut2[i];  // beyond the finer level's radius (see am_fine_kernel)
        fine_block_list<NBLK>(keep, outer_only, tid, tg, tb, w, lane, wave_cnt, items, need);
        // weights of the blocks some group needs
        {
            const float *W0 = MODE == PH_A ? nullptr : MODE == PH_B ? LV + (size_t)i * nm4 : LV + (size_t)i * nm4 + a.n4;
            const float *W1 = MODE == PH_CA ? REM + a.n4 + (size_t)((i + 1) & 1) * a.m4 : nullptr;
            for (int idx = tid; idx < nblk * kBox; idx += T) {
                if (!need[idx >> 4]) continue;
                float v0, v1 = 0.f;
                if (MODE == PH_A) v0 = idx < n_cand ? a.multiR : 0.f;
                else v0 = idx < cand_n4 ? pcc::agent_ld(W0 + idx) : 0.f;
                if (NW == 2) v1 = idx < cand_n4 ? pcc::agent_ld(W1 + idx) : 0.f;
                lds_w[0][idx] = v0;
                if (NW == 2) lds_w[1][idx] = v1;
            }
        }
        __syncthreads();
        float s0[kFineQ], s1[kFineQ];
#pragma unroll
        for (int j = 0; j < kFineQ; j++) s0[j] = s1[j] = 0.f;
        const FineRows rows = {P, P + CH, P + 2 * CH, lds_w[0], lds_w[1]};
        fine_walk<NW>(rows, items[og], wave_cnt[2 * og] + wave_cnt[2 * og + 1], cs, cl, c0, c1, ROLE ? set2 : set1, s0, s1);
        fine_reduce<NW>(s0, s1, red, cs, cl, og, quad);
        __syncthreads();
        const int own_e = ROLE ? own2 : own1;
        if (own_e >= 0) {
            const float sum0 = red[0][0][tid] + red[0][1][tid];
            const float sum1 = NW == 2 ? red[1][0][tid] + red[1][1][tid] : 0.f;
            if (MODE == PH_A) {
                ratL = pass_a_ratio(a.multiL, sum0);
                pcc::agent_st(LV + own_e, ratL);
            } else if (MODE == PH_B) {
                const PassB pb = pass_b(i == 0 ? a.multiR : remR, sum0);
                pcc::agent_st(LV + (size_t)i * nm4 + a.n4 + own_e, pb.ratio);
                pcc::agent_st(REM + a.n4 + (size_t)((i + 1) & 1) * a.m4 + own_e, pb.remain);
                remR = pb.remain;
                if (i == 2) {  // owners still live after level 2 = the owner count of pass B of level 3 (V_COWN)
                    const unsigned long long alive = __ballot(pb.remain != 0.f);
                    if (lane == 0) {
                        atomicAdd(&row[3], (int)__popcll(alive));
                        unsigned *mo = a.live_mask + ((size_t)smp * kLevels + 3) * a.mask_words;  // ... and their bits
                        if (2 * tile < a.mask_words) mo[2 * tile] = (unsigned)alive;
                        if (2 * tile + 1 < a.mask_words) mo[2 * tile + 1] = (unsigned)(alive >> 32);
                    }
                }
            } else {
                remL = pass_c_left(i == 0 ? a.multiL : remL, ratL, sum0);
                pcc::agent_st(REM + own_e, remL);
                ratL = pass_a_ratio(remL, sum1);  // pass A of the next level
                pcc::agent_st(LV + (size_t)(i + 1) * nm4 + own_e, ratL);
            }
        }
    };
    // pcc::coresident_barrier; the failure code for the host: 1 | barrier << 4 | arrivals seen << 8 | sample << 20
    auto barrier = [&]() -> bool {
        arrivals += (unsigned)a.tiles;
        return pcc::coresident_barrier<1, (1u << 22)>(bar, arrivals, err, a.host_err, [&] {
            const unsigned seen = pcc::agent_ld(bar);
            return 1u | ((arrivals / (unsigned)a.tiles) << 4) | ((seen & 0xfffu) << 8) | ((unsigned)smp << 20);
        });
    };
    if (a.inject && tile == 0 && tid == 0) pcc::coresident_fail(err, a.host_err, 1u | ((unsigned)smp << 20));
    __syncthreads();  // clouds staged
    pass(std::integral_constant<int, PH_A>{}, 0);
    for (int i = 0; i < 3 && ok; i++) {
        ok = barrier();
        if (!ok) break;
        pass(std::integral_constant<int, PH_B>{}, i);
        ok = barrier();
        if (!ok) break;
        pass(std::integral_constant<int, PH_CA>{}, i);
    }
}

// The phases run in Hilbert-sorted index space; this puts the nine (ratioL | ratioR) level vectors back into
// the caller's point order for the materialise pass (contiguous loads there) and fills
// temp = remainL | remainR | ratioL | ratioR of the last level (approxmatch.cu:4).  A sample whose resident fine-level
// passes did not complete (kErrSlot of its live-counter row, am_fine_persist_kernel) gets NaN rows, hence NaN match and
// cost, as on the implicit path.
__global__ __launch_bounds__(256) void am_unpermute_kernel(int n, int m, int n4, int m4,
                                                            const float *__restrict__ lv_sorted,
                                                            const float *__restrict__ rem_sorted,
                                                            const int *__restrict__ rank1,
                                                            const int *__restrict__ rank2,
                                                            const int *__restrict__ flags,
                                                            float *__restrict__ lv, float *__restrict__ temp) {
    // sorted-space rows are [ratioL (n4) | ratioR (m4)] (16-byte aligned halves); outputs are dense [n | m]
    const int smp = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n + m) return;
    const int s = i < n ? rank1[(size_t)smp * n + i] : n4 + rank2[(size_t)smp * m + (i - n)];
    const size_t nm = (size_t)n + m, nm4 = (size_t)n4 + m4;
    const float *src = lv_sorted + (size_t)smp * kLevels * nm4;
    float *dst = lv + (size_t)smp * kLevels * nm;
    const bool failed = flags[(size_t)smp * kLiveRow + kErrSlot] != 0;
    float last = 0.f;
#pragma unroll
    for (int l = 0; l < kLevels; l++) {
        last = failed ? __builtin_nanf("") : src[(size_t)l * nm4 + s];
        dst[(size_t)l * nm + i] = last;
    }
    // remain row: remainL (n4) | remainR ping (m4) | pong (m4); the nine passes B leave the final remainR in pong
    float *tb = temp + (size_t)smp * 2 * nm;
    tb[i] = failed ? __builtin_nanf("") : rem_sorted[(size_t)smp * (nm4 + m4) + (i < n ? s : s + m4)];
    tb[nm + i] = last;
}

// ---------------------------------------------------------------------------------------------------
// Materialise: match[b,l,k] = sum_i (exp2(c_i d2) * ratioL_i[k]) * ratioR_i[l], i = 0..8 in the
// reference's accumulation order (approxmatch.cu:154-155).  Write-only on match (float4 rows).
// Optionally also accumulates cost partials sum match*sqrt(d2) (matchcost, :207-208) so that the
// Python-level match_cost forward needs no second pass over match.
// ---------------------------------------------------------------------------------------------------
constexpr int kMatLT = 64;   // l rows per workgroup
constexpr int kMatKT = 256;  // k columns per workgroup (4 per lane)

template <bool COST, bool VEC>
__global__ __launch_bounds__(256) void am_materialise_kernel(int n, int m, const float *__restrict__ xyz1,
                                                              const float *__restrict__ xyz2,
                                                              const float *__restrict__ lv, LevelConsts lc,
                                                              float *__restrict__ match,
                                                              float *__restrict__ cost_part) {
    __shared__ float4 lds_l[kMatLT][3];  // (x,y,z,rr0) (rr1..rr4) (rr5..rr8)
    __shared__ float lds_red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int smp = blockIdx.z;
    const int l0 = blockIdx.y * kMatLT;
    const int k0 = blockIdx.x * kMatKT + lane * 4;
    const size_t lvs = (size_t)kLevels * (n + m);
    const float *lvb = lv + (size_t)smp * lvs;
    const float *p1 = xyz1 + (size_t)smp * n * 3;
    const float *p2 = xyz2 + (size_t)smp * m * 3;
    const int lcnt = min(kMatLT, m - l0);

    if (tid < lcnt) {
        const int l = l0 + tid;
        float rr[kLevels];
#pragma unroll
        for (int i = 0; i < kLevels; i++) rr[i] = lvb[(size_t)i * (n + m) + n + l];
        lds_l[tid][0] = make_float4(p2[l * 3 + 0], p2[l * 3 + 1], p2[l * 3 + 2], rr[0]);
        lds_l[tid][1] = make_float4(rr[1], rr[2], rr[3], rr[4]);
        lds_l[tid][2] = make_float4(rr[5], rr[6], rr[7], rr[8]);
    }
    float x1[4], y1[4], z1[4], rl[kLevels][4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int k = k0 + q;
        k = k < n ? k : n - 1;
        x1[q] = p1[k * 3 + 0];
        y1[q] = p1[k * 3 + 1];
        z1[q] = p1[k * 3 + 2];
#pragma unroll
        for (int i = 0; i < kLevels; i++) rl[i][q] = lvb[(size_t)i * (n + m) + k];
    }
    __syncthreads();
    float csum = 0.f;
    for (int li = w; li < lcnt; li += 4) {
        const float4 A = lds_l[li][0], B = lds_l[li][1], Cc = lds_l[li][2];
        const float rr[kLevels] = {A.w, B.x, B.y, B.z, B.w, Cc.x, Cc.y, Cc.z, Cc.w};
        // A query point whose capacity is used up has ratioR == 0 exactly at every later level (remainR is
        // clamped to 0, approxmatch.cu:109, and ratioR = consumption * remainR, :108): that level adds exactly 0
        // to the whole row, so its exponentials are skipped (wave-uniform).  Typically 4 of 9 levels are live.
        int live[kLevels];
#pragma unroll
        for (int i = 0; i < kLevels; i++) live[i] = __builtin_amdgcn_readfirstlane((int)(rr[i] != 0.f));
        float d[4], acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            d[q] = sq3(A.x - x1[q], A.y - y1[q], A.z - z1[q]);
            acc[q] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < kLevels; i++) {
            if (live[i]) {
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] += (fast_exp2(lc.c[i] * d[q]) * rl[i][q]) * rr[i];
            }
        }
        float out[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            out[q] = acc[q];
            if (COST && k0 + q < n) csum = __builtin_fmaf(acc[q], __builtin_amdgcn_sqrtf(d[q]), csum);
        }
        float *row = match + ((size_t)smp * m + (l0 + li)) * n;
        if (VEC) {
            if (k0 + 3 < n) {
                // match is written once and read back only after the whole 512 MiB (far beyond the 256 MiB Infinity
                // Cache): non-temporal stores (A/B on MI355X: materialise 150 -> 127 us)
                v4f o4 = {out[0], out[1], out[2], out[3]};
                __builtin_nontemporal_store(o4, reinterpret_cast<v4f *>(row + k0));
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (k0 + q < n) row[k0 + q] = out[q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (k0 + q < n) row[k0 + q] = out[q];
        }
    }
    if (COST) {
        csum = pcc::wave_sum_down(csum);
        if (lane == 0) lds_red[w] = csum;
        __syncthreads();
        if (tid == 0)
            cost_part[(size_t)smp * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] =
                ((lds_red[0] + lds_red[1]) + lds_red[2]) + lds_red[3];
    }
}

// ---- host side -------------------------------------------------------------------------------------
constexpr int kPhCH = 2048;
// the dense list of pass C/A holds the LIVE candidates only (under half of the cloud from level 3 on): chunks of 1024
// (25-29 KB of LDS: five or six workgroups per CU instead of three; a longer list takes a second chunk)
constexpr int kClistCH = 1024;

static bool cull_enabled() {  // measurement switch (pcc_test_hooks.h): every work-skipping variant off
    return pcc::tuning(PCC_TUNE_AM_NOCULL) == 0;
}

// The launch profile's name of a pass: mode, level, and which kernel variant ran it -- [0] "plain" (no skip logic: what
// am_nocull runs everywhere), [1] the level's work-skipping variant: "fine" (V_CULL, am_fine_kernel), "own" (V_COWN) or
// "list" (V_CLIST).
template <int MODE>
const char *phase_name(int level, bool skipping) {
    static const char *const names[4][kLevels][2] = {
        {{"am_phase_kernel<A> L0 plain", "am_phase_kernel<A> L0 fine"}, {"", ""}, {"", ""}, {"", ""}, {"", ""},
         {"", ""}, {"", ""}, {"", ""}, {"", ""}},
        {{"am_phase_kernel<B> L0 plain", "am_phase_kernel<B> L0 fine"},
         {"am_phase_kernel<B> L1 plain", "am_phase_kernel<B> L1 fine"},
         {"am_phase_kernel<B> L2 plain", "am_phase_kernel<B> L2 fine"},
         {"am_phase_kernel<B> L3 plain", "am_phase_kernel<B> L3 own"},
         {"am_phase_kernel<B> L4 plain", "am_phase_kernel<B> L4 own"},
         {"am_phase_kernel<B> L5 plain", "am_phase_kernel<B> L5 own"},
         {"am_phase_kernel<B> L6 plain", "am_phase_kernel<B> L6 own"},
         {"am_phase_kernel<B> L7 plain", "am_phase_kernel<B> L7 own"},
         {"am_phase_kernel<B> L8 plain", "am_phase_kernel<B> L8 own"}},
        {{"am_phase_kernel<CA> L0 plain", "am_phase_kernel<CA> L0 fine"},
         {"am_phase_kernel<CA> L1 plain", "am_phase_kernel<CA> L1 fine"},
         {"am_phase_kernel<CA> L2 plain", "am_phase_kernel<CA> L2 fine"},
         {"am_phase_kernel<CA> L3 plain", "am_phase_kernel<CA> L3 list"},
         {"am_phase_kernel<CA> L4 plain", "am_phase_kernel<CA> L4 list"},
         {"am_phase_kernel<CA> L5 plain", "am_phase_kernel<CA> L5 list"},
         {"am_phase_kernel<CA> L6 plain", "am_phase_kernel<CA> L6 list"},
         {"am_phase_kernel<CA> L7 plain", "am_phase_kernel<CA> L7 list"}, {"", ""}},
        {{"", ""}, {"", ""}, {"", ""}, {"", ""}, {"", ""}, {"", ""}, {"", ""}, {"", ""},
         {"am_phase_kernel<C> L8 plain", "am_phase_kernel<C> L8 list"}}};
    return names[MODE][level][skipping];
}

template <int MODE, int R, int S, int G = 1>
int launch_phase_rs(PhaseArgs a, int b, int var, hipStream_t st, const char *what) {
    a.tiles = pcc::ceil_div(a.n_own, 64 * R / G);
    a.batch = b;
    const long long grid = (long long)b * a.tiles;
    if (grid > 0x7fffffffLL) return pcc::invalid("approxmatch: grid too large");
    {
        const bool skipping = (var == V_CLIST && (MODE == PH_CA || MODE == PH_C)) || (var == V_COWN && MODE == PH_B);
        pcc::ProfScope prof(phase_name<MODE>(a.level, skipping), st);
        const dim3 g((unsigned)grid), blk(64 * S);
        // only the combinations the schedule uses are instantiated
        if (var == V_CLIST && (MODE == PH_CA || MODE == PH_C))
            hipLaunchKernelGGL((am_phase_kernel<(MODE == PH_CA || MODE == PH_C) ? MODE : PH_C, R, S, kClistCH, V_CLIST>), g, blk, 0, st, a);
        else if (var == V_COWN && MODE == PH_B)
            hipLaunchKernelGGL((am_phase_kernel<PH_B, (G > 1 ? 1 : R), S, kPhCH, V_COWN, G>), g, blk, 0, st, a);
        else hipLaunchKernelGGL((am_phase_kernel<MODE, R, S, kPhCH, V_PLAIN>), g, blk, 0, st, a);
    }
    return pcc::check_launch(what);
}

template <int MODE>
int launch_fine(PhaseArgs a, int b, hipStream_t st, const char *what) {
    a.tiles = pcc::ceil_div(a.n_own, 64);
    a.batch = b;
    const long long grid = (long long)b * a.tiles;
    if (grid > 0x7fffffffLL) return pcc::invalid("approxmatch: grid too large");
    {
        pcc::ProfScope prof(phase_name<MODE>(a.level, true), st);
        hipLaunchKernelGGL((am_fine_kernel<(MODE == PH_C ? PH_CA : MODE), kPhCH>), dim3((unsigned)grid), dim3(64 * kFineS), 0, st, a);
    }
    return pcc::check_launch(what);
}

template <int MODE>
int launch_phase(const PhaseArgs &a, int b, int var, hipStream_t st, const char *what) {
    // the box-culled passes of the fine levels: 16-owner groups
    if (var == V_CULL) return launch_fine<MODE>(a, b, st, what);
    // Owner compaction packs the live owners into the first tiles; a full tile takes as long as before (just on fewer
    // CUs), so these launches use the smallest tile (64 owners x 8 waves), and where few owners are left (recon / uniform
    // clouds: ~25 % live at level 5, 5 % at level 8) an owner is spread over 2 / 4 lanes: the pair loop of a workgroup,
    // which is the launch's critical path, gets that much shorter (first levels 3 / 4 and 4 / 6: 2-5 us slower)
    if (var == V_COWN) {
        if (a.live_in && a.level >= 5) return launch_phase_rs<MODE, 1, 8, 4>(a, b, var, st, what);
        if (a.live_in && a.level >= 4) return launch_phase_rs<MODE, 1, 8, 2>(a, b, var, st, what);
        return launch_phase_rs<MODE, 1, 8>(a, b, var, st, what);
    }
    // Workgroup shape: R owners per lane x S candidate slices (waves).  One wave can issue a VALU instruction only every
    // 4 cycles while a SIMD retires one every 2, so a phase needs >= 2 (better 4) waves per SIMD = 2048-4096 waves on
    // 256 CUs; R is spent only once the chip is full (each LDS broadcast read is then amortised over R owners).
    // (A large batch arrives here as two concurrent half-batch lanes: 32768 owners per launch at B=32, N=2048, where
    // 128-owner tiles measured 492 us per forward+backward against 509 us for 64-owner tiles.)
    const long long owners = (long long)b * a.n_own;
    // pass C/A on the dense list of live candidates: 25 KB of LDS per 64-owner workgroup (chunks of kClistCH), so the
    // 2 x 512 workgroups of two half-batch lanes are resident together and every owner's loop is half as long as on the
    // 128-owner tile (432.9 -> 429.1 us per match_cost call; with the 45 KB carve of 2048-candidate chunks it measured slower)
    if (var == V_CLIST && owners < 4LL * 65536) return launch_phase_rs<MODE, 1, 8>(a, b, var, st, what);
    if (owners >= 4LL * 65536) return launch_phase_rs<MODE, 4, 8>(a, b, var, st, what);
    if (owners >= 32768) return launch_phase_rs<MODE, 2, 8>(a, b, var, st, what);
    return launch_phase_rs<MODE, 1, 8>(a, b, var, st, what);
}

size_t cost_parts(int n, int m) { return (size_t)pcc::ceil_div(n, kMatKT) * pcc::ceil_div(m, kMatLT); }

// Workspace carve (bytes, every section 16-byte aligned).  The implicit path (match_cost_implicit_impl) passes its
// am_pair_kernel tiling: its three sections follow the others and are empty on the materialising path.
struct WsLayout : pcc::AmDims {
    int b;
    int col_blocks, row_tiles;
    bool grad;
    size_t total;
    WsLayout(int b_, int n_, int m_, int col_blocks_ = 0, int row_tiles_ = 0, bool grad_ = false)
        : AmDims(n_, m_), b(b_), col_blocks(col_blocks_), row_tiles(row_tiles_), grad(grad_) {
        WsView unused;
        total = carve(0, 0, unused);
    }
    WsView view(char *base, int s) const {
        WsView v;
        carve(reinterpret_cast<uintptr_t>(base), (size_t)s, v);
        return v;
    }

  private:
    // The sections in order: points every pointer of `v` at sample s of the workspace at `base`; returns the end offset.
    size_t carve(uintptr_t base, size_t s, WsView &v) const {
        size_t o = 0;
        auto sec = [&](auto *&p, size_t per) {  // per: elements per sample
            using T = std::remove_reference_t<decltype(*p)>;
            p = reinterpret_cast<T *>(base + o + s * per * sizeof(T));
            o = (o + (size_t)b * per * sizeof(T) + 15) & ~(size_t)15;
        };
        sec(v.soa1, 3 * (size_t)n4);
        sec(v.soa2, 3 * (size_t)m4);
        sec(v.rank1, n);
        sec(v.rank2, m);
        sec(v.perm1, n);
        sec(v.perm2, m);
        sec(v.box1, (size_t)nb1 * 8);
        sec(v.box2, (size_t)nb2 * 8);
        sec(v.rem, rem_floats());
        sec(v.lv, lv_floats());
        sec(v.lv_orig, kLevels * ((size_t)n + m));
        sec(v.cpart, cost_parts(n, m));
        sec(v.clist, 5 * (size_t)m4);
        sec(v.clist_cnt, 1);
        sec(v.live_cnt, kLiveRow);
        sec(v.live_mask, (size_t)kLevels * mask_words(m4));
        sec(v.aos1, n);
        sec(v.aos2, m);
        sec(v.pair_cost, (size_t)col_blocks * row_tiles);
        sec(v.part1, grad ? (size_t)row_tiles * n4 * 3 : 0);
        sec(v.part2, grad ? (size_t)col_blocks * m4 * 3 : 0);
        return o;
    }
};

// One internal side stream per device: the second half of a large batch runs its 19 dependent phase launches there
// while the first half runs on the caller's stream, so that one half's kernels fill the launch / drain bubbles of
// the other's (each launch is a chain link of ~20 us with 4-8 us of fixed cost).  Fork and join are events on the
// caller's stream: for the caller the call still is "enqueue on `stream`, no host synchronisation".
constexpr int kMaxLanes = 2;
hipStream_t side_stream() {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!streams[dev]) {
        // HIP multiplexes the streams of a process onto a few hardware queues per PRIORITY class, in creation order: a
        // plain side stream created after an application has made many streams of its own (RCCL does, at
        // init_process_group) can land on the hardware queue of the caller's stream, and the two lanes then serialise
        // (measured: 0.53 -> 0.73 ms per bench step).  A high-priority stream comes from a different queue pool than the
        // caller's normal-priority stream.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
            (void)hipGetLastError();
            least = greatest = 0;
        }
        if (hipStreamCreateWithPriority(&streams[dev], hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            if (hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking) != hipSuccess) {
                streams[dev] = nullptr;
                (void)hipGetLastError();
            }
        }
    }
    return streams[dev];
}

struct ForkJoin {  // the side stream waits for everything enqueued on main so far; at scope exit main waits for it
    hipStream_t main, side = nullptr;
    ForkJoin(hipStream_t m, bool fork) : main(m) {
        if (!fork) return;
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return;
        if (hipEventRecord(ev, main) == hipSuccess) {
            hipStream_t s = side_stream();
            if (s && hipStreamWaitEvent(s, ev, 0) == hipSuccess) side = s;
        }
        (void)hipEventDestroy(ev);  // released once the recorded work has completed
    }
    ~ForkJoin() {
        if (!side) return;
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamSynchronize(side);  // cannot order the streams any other way
            return;
        }
        (void)hipEventRecord(ev, side);
        (void)hipStreamWaitEvent(main, ev, 0);
        (void)hipEventDestroy(ev);
    }
};

static bool resident_enabled() {  // measurement switch (pcc_test_hooks.h): one launch per pass at the fine levels too
    return pcc::tuning(PCC_TUNE_AM_NORESIDENT) == 0;
}
// the seven fine-level passes of the samples of `sc` as one resident launch; returns -1 when the device / the sizes do
// not qualify (the caller then runs one launch per pass)
int launch_fine_resident(const Sched &sc, int bc, hipStream_t st) {
    if (!sc.skip || !sc.live_cnt || !sc.live_mask || !resident_enabled()) return -1;
    if (sc.n > kFpCH || sc.m > kFpCH || sc.n < 1 || sc.m < 1) return -1;
    const int tiles = pcc::ceil_div(std::max(sc.n, sc.m), 64);
    FinePersistArgs a{};
    a.n = sc.n; a.m = sc.m; a.n4 = sc.n4; a.m4 = sc.m4; a.nb1 = sc.nb1; a.nb2 = sc.nb2; a.tiles = tiles;
    a.soa1 = sc.soa1; a.soa2 = sc.soa2; a.box1 = sc.box1; a.box2 = sc.box2;
    a.rem = sc.rem; a.lv = sc.lv; a.multiL = sc.multiL; a.multiR = sc.multiR;
    for (int i = 0; i < 4; i++) {
        a.c[i] = sc.lc.c[i];
        a.cut2[i] = zero_cut2(sc.lc, i);
    }
    a.live_cnt = sc.live_cnt;
    a.live_mask = sc.live_mask;
    a.mask_words = mask_words(sc.m4);
    static const int per_cu = [] {  // resident workgroups per CU (0 if the query fails)
        int r = 0;
        const void *k = reinterpret_cast<const void *>(am_fine_persist_kernel);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r, k, 64 * kFineS, 0) != hipSuccess) (void)hipGetLastError();
        return r;
    }();
    // the whole launch resident at once on half of the device's workgroup slots
    if (per_cu < 2 || (long long)bc * tiles > pcc::device_cus()) return -1;
    pcc::CoresidentGate gate(pcc::kFineResident, st);  // declines while `st` is being captured
    if (!gate.ok) return -1;
    a.host_err = gate.sticky;
    a.inject = gate.inject;
    {
        pcc::ProfScope prof("am_fine_persist_kernel", st);
        hipLaunchKernelGGL(am_fine_persist_kernel, dim3((unsigned)(bc * tiles)), dim3(64 * kFineS), 0, st, a);
    }
    return pcc::check_launch("approxmatch(resident fine levels)");
}

// The schedule of one lane: the samples of the workspace view `v`.
Sched lane_sched(const WsLayout &L, const WsView &v, const LevelConsts &lc) {
    Sched sc{};
    sc.n = L.n; sc.m = L.m; sc.n4 = L.n4; sc.m4 = L.m4; sc.nb1 = L.nb1; sc.nb2 = L.nb2;
    sc.soa1 = v.soa1; sc.soa2 = v.soa2; sc.box1 = v.box1; sc.box2 = v.box2; sc.rem = v.rem; sc.lv = v.lv;
    // approxmatch.cu:6-12 (integer division)
    if (L.n >= L.m) { sc.multiL = 1; sc.multiR = (float)(L.n / L.m); }
    else { sc.multiL = (float)(L.m / L.n); sc.multiR = 1; }
    sc.skip = cull_enabled() ? 1 : 0;
    sc.lc = lc;
    sc.clist = v.clist; sc.clist_cnt = v.clist_cnt;
    if (sc.skip) { sc.live_cnt = v.live_cnt; sc.live_mask = v.live_mask; }
    return sc;
}

// Sort + the 19 passes: leaves the nine (ratioL | ratioR) level rows and remainL | remainR in the workspace, in the
// Hilbert-sorted index space.
int run_levels(const WsLayout &L, char *base, const float *xyz1, const float *xyz2, const LevelConsts &lc, hipStream_t st,
               const std::function<int(int, int, hipStream_t)> &lane_tail = nullptr,
               const std::function<int(int, int, hipStream_t)> &after_sort = nullptr) {
    if (const unsigned fw = pcc::take_coresident_failure(pcc::kFineResident)) {
        char buf[320];
        std::snprintf(buf, sizeof buf, "approxmatch: an earlier call on this device did not complete (a sample barrier of the resident "
                      "fine-level launch timed out: barrier %u of sample %u saw %u arrivals; the implicit path reported NaN for those "
                      "samples); this call was not started", (fw >> 4) & 0xfu, fw >> 20, (fw >> 8) & 0xfffu);
        return pcc::invalid(buf);
    }
    const bool split_enabled = pcc::tuning(PCC_TUNE_AM_NOSPLIT) == 0;  // (measurement switch: everything on the caller's stream)

    // Lanes: disjoint sample ranges that run the same schedule on different streams.  Two lanes when each half still
    // is a sizeable launch (B=32, N=2048: EMD forward+backward 530 -> 49x us); a lane is the same schedule on the
    // workspace view at its first sample.
    struct Lane {
        int s0, bc;
        hipStream_t st;
        WsView v;
        Sched sc;
    };
    Lane lanes[kMaxLanes];
    int nlanes = 1;
    bool fork = false;
    if (split_enabled && L.b >= 8 && (long long)L.b * std::max(L.n, L.m) >= 32768) {
        fork = !pcc::capturing(st);  // a capture stays a single-stream chain
    }
    ForkJoin fj(st, fork);
    if (fj.side) nlanes = 2;
    for (int l = 0; l < nlanes; l++) {
        Lane &ln = lanes[l];
        ln.s0 = (int)((long long)L.b * l / nlanes);
        ln.bc = (int)((long long)L.b * (l + 1) / nlanes) - ln.s0;
        ln.st = l == 0 ? st : fj.side;
        ln.v = L.view(base, ln.s0);
        ln.sc = lane_sched(L, ln.v, lc);
    }
    int rc = PCC_OK;
    auto enqueue_head = [&](int l) -> int {
        const Lane &ln = lanes[l];
        const size_t s0 = (size_t)ln.s0;
        int r = pcc::sort_clouds(L, ln.v, ln.bc, xyz1 + s0 * L.n * 3, xyz2 + s0 * L.m * 3, (bool)after_sort, ln.st);
        // work that only needs the sorted clouds of this lane's samples (pcc_chamfer_emd: the nearest-neighbour search).
        // Even lanes run it here, odd lanes behind their passes: two searches at the same moment halve each other (each
        // wants every SIMD); against the other lane's pass chain a search costs less (chamfer_emd 447.7 -> 440.4 us, step
        // 470 -> 462.6 us; before passes 3 / 7 / 11 / 15 of the odd lane: 451 / 445 / 445 / 445 us; on a
        // stream of its own: 522 us).
        if (!r && after_sort && l % 2 == 0) r = after_sort(ln.s0, ln.bc, ln.st);
        return r;
    };
    auto enqueue_pass = [&](int l, int p) -> int {
        const Lane &ln = lanes[l];
        int mode, var;
        const PhaseArgs a = build_phase(ln.sc, p, &mode, &var);
        switch (mode) {
        case PH_A: return launch_phase<PH_A>(a, ln.bc, var, ln.st, "approxmatch(A)");
        case PH_B: return launch_phase<PH_B>(a, ln.bc, var, ln.st, "approxmatch(B)");
        case PH_CA: return launch_phase<PH_CA>(a, ln.bc, var, ln.st, "approxmatch(CA)");
        default: return launch_phase<PH_C>(a, ln.bc, var, ln.st, "approxmatch(C)");
        }
    };
    int first_pass[kMaxLanes] = {};
    {
        for (int l = 0; l < nlanes && !rc; l++) rc = enqueue_head(l);
        if (rc) return rc;
        {
            // pass p of every lane is enqueued before pass p+1 of any: the streams advance together
            pcc::ProfScope seq0("am_phase_sequence", lanes[0].st, true);
            pcc::ProfScope seq1("am_phase_sequence", lanes[nlanes > 1 ? 1 : 0].st, true, nlanes >= 2);
            // the seven passes of levels 0-2 as one resident launch per lane where the device and the sizes allow it
            for (int l = 0; l < nlanes && !rc; l++) {
                const int r = launch_fine_resident(lanes[l].sc, lanes[l].bc, lanes[l].st);
                if (r > 0) rc = r;
                else if (r == 0) first_pass[l] = kFpPasses;
            }
            for (int p = 0; p < sched_phases() && !rc; p++)
                for (int l = 0; l < nlanes && !rc; l++)
                    if (p >= first_pass[l]) rc = enqueue_pass(l, p);
            if (rc) return rc;
        }
        // what follows the passes for one lane's samples (the implicit path's pair + finish kernels) goes on that lane's
        // stream: the lane that finishes its passes first starts at once instead of waiting for the join
        if (after_sort)
            for (int l = 1; l < nlanes; l += 2)
                if (int rc2 = after_sort(lanes[l].s0, lanes[l].bc, lanes[l].st)) return rc2;
        if (lane_tail) {
            for (int l = 0; l < nlanes; l++)
                if (int rc2 = lane_tail(lanes[l].s0, lanes[l].bc, lanes[l].st)) return rc2;
        }
    }
    return PCC_OK;
}

int approxmatch_impl(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                     void *workspace, size_t workspace_bytes, float *cost_out, hipStream_t st) {
    const WsLayout L(b, n, m);
    if (workspace_bytes < L.total) return pcc::invalid("approxmatch: workspace too small");
    if (!aligned16(workspace)) return pcc::invalid("approxmatch: workspace must be 16-byte aligned");
    char *base = static_cast<char *>(workspace);
    const LevelConsts lc = make_levels();
    int rc = run_levels(L, base, xyz1, xyz2, lc, st);
    if (rc) return rc;
    const WsView v = L.view(base, 0);
    // (v.live_cnt: the flags written by this call's sort and passes)
    hipLaunchKernelGGL(am_unpermute_kernel, dim3(pcc::ceil_div(n + m, 256), b), dim3(256), 0, st, n, m, L.n4, L.m4, v.lv, v.rem,
                       v.rank1, v.rank2, v.live_cnt, v.lv_orig, temp);
    rc = pcc::check_launch("approxmatch(unpermute)");
    if (rc) return rc;
    const dim3 grid(pcc::ceil_div(n, kMatKT), pcc::ceil_div(m, kMatLT), b);
    const bool vec = (n % 4 == 0) && aligned16(match);
    if (cost_out) {
        {
            pcc::ProfScope prof("am_materialise_kernel<cost>", st);
            if (vec) hipLaunchKernelGGL((am_materialise_kernel<true, true>), grid, dim3(256), 0, st, n, m, xyz1, xyz2, v.lv_orig, lc, match, v.cpart);
            else hipLaunchKernelGGL((am_materialise_kernel<true, false>), grid, dim3(256), 0, st, n, m, xyz1, xyz2, v.lv_orig, lc, match, v.cpart);
        }
        rc = pcc::check_launch("approxmatch(materialise+cost)");
        if (rc) return rc;
        pcc::launch_reduce_rows(b, (int)cost_parts(n, m), v.cpart, cost_out, st);
        return pcc::check_launch("approxmatch(cost reduce)");
    }
    {
        pcc::ProfScope prof("am_materialise_kernel", st);
        if (vec) hipLaunchKernelGGL((am_materialise_kernel<false, true>), grid, dim3(256), 0, st, n, m, xyz1, xyz2, v.lv_orig, lc, match, nullptr);
        else hipLaunchKernelGGL((am_materialise_kernel<false, false>), grid, dim3(256), 0, st, n, m, xyz1, xyz2, v.lv_orig, lc, match, nullptr);
    }
    return pcc::check_launch("approxmatch(materialise)");
}

int match_cost_implicit_impl(int b, int n, int m, const float *xyz1, const float *xyz2, const float *grad_cost,
                             float *cost, float *grad1, float *grad2, hipStream_t st,
                             const pcc::ChamferOut *chamfer = nullptr) {
    const bool grad = grad1 && grad2;
    const int col_blocks = pcc::ceil_div(n, 64 * kPairQ), row_tiles = pcc::ceil_div(m, kPairRT);
    const WsLayout L(b, n, m, col_blocks, row_tiles, grad);
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc(L.total, "workspace allocation failed")) return rc;
    char *base = static_cast<char *>(ws.p);
    const LevelConsts lc = make_levels();
    auto tail = [&](int s0, int bc, hipStream_t lst) -> int {
        return pcc::launch_pair_finish(L, L.view(base, s0), s0, bc, col_blocks, row_tiles, grad_cost, cost, grad1, grad2, chamfer, lst);
    };
    auto nn_after_sort = [&](int s0, int bc, hipStream_t lst) -> int {
        return pcc::launch_nn_sorted(L, L.view(base, s0), s0, bc, chamfer, lst);
    };
    if (chamfer) return run_levels(L, base, xyz1, xyz2, lc, st, tail, nn_after_sort);
    return run_levels(L, base, xyz1, xyz2, lc, st, tail);
}

// pcc_approxmatch (with_cost false) and pcc_approxmatch_cost: the same checks, each under its own name
int approxmatch_entry(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp, bool with_cost,
                      float *cost, hipStream_t st) {
    pcc::clear_error();
    if (int rc = check_sizes(with_cost ? "approxmatch_cost" : "approxmatch", b, n, m)) return rc;
    const char *null_ptr = with_cost ? "approxmatch_cost: null pointer" : "approxmatch: null pointer";
    if (b == 0) return PCC_OK;
    if (with_cost && !cost) return pcc::invalid(null_ptr);
    if (n == 0 || m == 0)  // nothing to match (reference: empty loops)
        return with_cost ? zero_fill_empty(b, n, m, cost, nullptr, nullptr, st, "approxmatch_cost: memset failed") : PCC_OK;
    if (!xyz1 || !xyz2 || !match || !temp) return pcc::invalid(null_ptr);
    pcc::WsBlock ws(st);
    const size_t bytes = WsLayout(b, n, m).total;
    if (int rc = ws.alloc(bytes, "workspace allocation failed")) return rc;
    return approxmatch_impl(b, n, m, xyz1, xyz2, match, temp, ws.p, bytes, cost, st);
}

}  // namespace

namespace pcc {
int match_cost_with_chamfer(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *grad1,
                            float *grad2, hipStream_t st, const ChamferOut &chamfer) {
    return match_cost_implicit_impl(b, n, m, xyz1, xyz2, nullptr, cost, grad1, grad2, st, &chamfer);
}

}  // namespace pcc

extern "C" {

size_t pcc_approxmatch_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return WsLayout(b, n, m).total;
}

int pcc_approxmatch_ws(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                       void *workspace, size_t workspace_bytes, pcc_stream_t stream) {
    pcc::clear_error();
    if (int rc = check_sizes("approxmatch", b, n, m)) return rc;
    if (b == 0 || n == 0 || m == 0) return PCC_OK;  // nothing to match (reference: empty loops)
    if (!xyz1 || !xyz2 || !match || !temp || !workspace) return pcc::invalid("approxmatch: null pointer");
    return approxmatch_impl(b, n, m, xyz1, xyz2, match, temp, workspace, workspace_bytes, nullptr,
                            static_cast<hipStream_t>(stream));
}

int pcc_approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                    pcc_stream_t stream) {
    return approxmatch_entry(b, n, m, xyz1, xyz2, match, temp, false, nullptr, static_cast<hipStream_t>(stream));
}

int pcc_approxmatch_cost(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                         float *cost, pcc_stream_t stream) {
    return approxmatch_entry(b, n, m, xyz1, xyz2, match, temp, true, cost, static_cast<hipStream_t>(stream));
}

int pcc_match_cost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *grad_cost, float *cost,
                   float *grad1, float *grad2, pcc_stream_t stream) {
    pcc::clear_error();
    if (int rc = check_sizes("match_cost", b, n, m)) return rc;
    if (b == 0) return PCC_OK;
    if (!cost) return pcc::invalid("match_cost: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0 || m == 0) return zero_fill_empty(b, n, m, cost, grad1, grad2, st, "match_cost: memset failed");
    if (!xyz1 || !xyz2) return pcc::invalid("match_cost: null pointer");
    if ((grad1 == nullptr) != (grad2 == nullptr)) return pcc::invalid("match_cost: grad1 and grad2 go together");
    return match_cost_implicit_impl(b, n, m, xyz1, xyz2, grad_cost, cost, grad1, grad2, st);
}

void approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                 pcc_stream_t stream) {
    (void)pcc_approxmatch(b, n, m, xyz1, xyz2, match, temp, stream);
}

}  // extern "C"
