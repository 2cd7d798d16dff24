// What the files of the approximate EMD share (approxmatch.hip, cloud_sort.hip, nn_sorted.hip, am_pair.hip, matchcost.hip).
#pragma once
#include "pcc_common.hpp"

namespace {  // (per translation unit on purpose: LevelConsts is a parameter type of am_materialise_kernel, whose name stays)

using pcc::v4f;  // for __builtin_nontemporal_load/store

constexpr int kLevels = 9;       // j = 7 .. -1, level = -4^j            (approxmatch.cu:24-25)
constexpr float kLog2e = 1.44269504088896340736f;

struct LevelConsts {
    float c[kLevels];            // level_j * log2(e), exact scalings of fl(log2 e)
};

inline LevelConsts make_levels() {
    LevelConsts lc;
    float level = -16384.0f;     // -4^7
    for (int i = 0; i < kLevels; i++) {
        lc.c[i] = level * kLog2e;
        level *= 0.25f;
    }
    return lc;
}

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

using pcc::kBox;
constexpr int kLiveRow = 16;      // ints per sample in the live-owner counters (one per level, padded)
constexpr int kInfSlot = 13;      // live-counter row, slots 13 / 14: set1 / set2 of the sample holds an infinite coordinate
constexpr float kZeroExp = 151.f; // exp2(x) == 0 exactly for x <= -150 (below the smallest f32 subnormal)
constexpr int kBarSlot = 12;      // live-counter row: the sample's barrier counter of the resident passes (cleared by the sort kernel)
constexpr int kErrSlot = 15;      // live-counter row: the sample's resident passes did not complete
constexpr int kPairRT = 128;      // am_pair_kernel: rows per workgroup (32 per wave; 256: partials halve, 437 vs 432 us per call)
constexpr int kPairQ = 4;         // ... and columns per lane (2 measured slower)

inline int mask_words(int m4) { return (m4 + 31) / 32; }

// squared radius beyond which every exp2(c * d2) of level constant c is exactly 0
inline float zero_cut2(const LevelConsts &lc, int i) { return kZeroExp / -lc.c[i]; }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Every entry that goes through here launches at least one grid with the batch in y or z (am_row_kernel, am_grad_fused_kernel,
// reduce_splits_kernel, am_unpermute_kernel, am_materialise_kernel, pair_finish_kernel): 65535 is the most those take.
inline int check_sizes(const char *who, int b, int n, int m) {
    if (b < 0 || n < 0 || m < 0) return pcc::invalidf("%s: bad size", who);
    if ((long long)n * 3 > 0x7fffffffLL || (long long)m * 3 > 0x7fffffffLL) return pcc::invalidf("%s: bad size", who);
    if (b > 65535) return pcc::invalidf("%s: batch too large", who);
    return PCC_OK;
}

// n == 0 or m == 0: the sums are empty, so cost[b] and the gradients that have elements are 0 (null: not requested)
inline int zero_fill_empty(int b, int n, int m, float *cost, float *grad1, float *grad2, hipStream_t st, const char *what) {
    int rc = PCC_OK;
    if (cost) rc = pcc::zero_async(cost, (size_t)b * sizeof(float), st, what);
    if (n && grad1 && !rc) rc = pcc::zero_async(grad1, (size_t)b * n * 3 * sizeof(float), st, what);
    if (m && grad2 && !rc) rc = pcc::zero_async(grad2, (size_t)b * m * 3 * sizeof(float), st, what);
    return rc;
}

}  // namespace

namespace pcc {

// sizes of one call: padded row lengths and 16-point box counts of the two clouds
struct AmDims {
    int n, m, n4, m4, nb1, nb2;
    AmDims(int n_, int m_) : n(n_), m(m_), n4((n_ + 3) & ~3), m4((m_ + 3) & ~3), nb1(ceil_div(n_, kBox)), nb2(ceil_div(m_, kBox)) {}
    size_t rem_floats() const { return (size_t)n4 + 2 * (size_t)m4; }   // per sample
    size_t lv_floats() const { return kLevels * ((size_t)n4 + m4); }
};

// Every workspace section offset to one sample (each is indexed [sample][...]): a lane of samples [s0, s0 + bc) runs
// on the view at s0.  Sizes below are per sample.
struct WsView {
    float *soa1, *soa2;                // [3][n4] / [3][m4] Hilbert-sorted coordinates
    int *rank1, *rank2, *perm1, *perm2;  // [n] / [m] caller's index -> sorted position, and back
    float *box1, *box2;                // [nb][8] per 16 sorted points
    float *rem;                        // sorted space: remainL (n4) | remainR ping (m4) | pong (m4)
    float *lv;                         // [kLevels][n4 + m4] sorted space: ratioL | ratioR
    float *lv_orig;                    // [kLevels][n + m] the level rows in the caller's order
    float *cpart;                      // [cost_parts] cost partials of the materialise pass
    float *clist;                      // [5][m4] dense candidate list handed from pass B to pass C/A
    int *clist_cnt;                    // [1]
    int *live_cnt;                     // [kLiveRow] live-owner counters and flags
    unsigned *live_mask;               // [kLevels][mask_words] live bits of set2 per level (V_COWN)
    float4 *aos1, *aos2;               // [n] / [m] packed sorted points for the nearest-neighbour search of pcc_chamfer_emd
    float *pair_cost, *part1, *part2;  // implicit path only: am_pair_kernel's cost and gradient partials (PairArgs)
};

// cloud_sort.hip: sorts the bc samples of the view `v` (xyz1 / xyz2: their first sample); `aos`: also the packed rows aos1 / aos2
int sort_clouds(const AmDims &L, const WsView &v, int bc, const float *xyz1, const float *xyz2, bool aos, hipStream_t st);
// nn_sorted.hip, am_pair.hip: what follows the sort / the passes for the samples [s0, s0 + bc), `v` the view at s0
int launch_nn_sorted(const AmDims &L, const WsView &v, int s0, int bc, const ChamferOut *chamfer, hipStream_t lst);
int launch_pair_finish(const AmDims &L, const WsView &v, int s0, int bc, int col_blocks, int row_tiles, const float *grad_cost,
                       float *cost, float *grad1, float *grad2, const ChamferOut *chamfer, hipStream_t lst);
void launch_reduce_rows(int b, int parts, const float *part, float *out, hipStream_t st);  // matchcost.hip: reduce_rows_kernel

}  // namespace pcc
