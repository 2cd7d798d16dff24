// Wave-level helpers of the k-NN and nearest-neighbour searches (knn_lowdim.hip, knn_wide.hip, nn_sorted.hip) and of the
// sliced Wasserstein sort (sliced_wasserstein.hip), gfx950 wave64.
#pragma once
#include "pcc_common.hpp"
#include "wave_ops.hpp"

namespace pcc {

// 64-bit key (distance bits : index) above every real candidate: +inf distance, index INT_MAX
constexpr unsigned long long kKeyInf = ((unsigned long long)0x7f800000u << 32) | 0x7fffffffull;

// Ascending bitonic sort of the wave's 64 E keys (unsigned or unsigned long long), element e = lane + 64 h in v[h].
template <class T, int E>
__device__ __forceinline__ void wave_bitonic(T (&v)[E], int lane) {
#pragma unroll
    for (int kk = 2; kk <= 64 * E; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
                const int hj = j >> 6;
#pragma unroll
                for (int h = 0; h < E; h++) {
                    if (h & hj) continue;
                    const bool asc = ((lane + 64 * h) & kk) == 0;
                    const T a = v[h], b = v[h | hj];
                    const bool sw = asc ? b < a : a < b;
                    v[h] = sw ? b : a;
                    v[h | hj] = sw ? a : b;
                }
            } else {
#pragma unroll
                for (int h = 0; h < E; h++) {
                    const int i = lane + 64 * h;
                    T o;
                    if constexpr (sizeof(T) == 8) o = shfl_xor_u64(v[h], j);
                    else o = (T)__shfl_xor((int)v[h], j, 64);
                    const bool take_min = ((i & j) == 0) == ((i & kk) == 0);
                    v[h] = take_min ? (o < v[h] ? o : v[h]) : (o < v[h] ? v[h] : o);
                }
            }
        }
    }
}

// The same network on the other layout: element e = lane E + h in v[h] (a lane holds E consecutive elements), 64-bit keys.
// The steps j < E stay inside a lane (one comparison per pair of registers, no cross-lane traffic) and the steps j >= E
// meet lane ^ (j / E): through DPP where the ISA has the pattern (lane ^ 1, ^ 2: quad_perm; ^ 8: row_ror 8), through
// ds_bpermute otherwise.  Sorting 64 E keys takes 21 cross-lane steps for any E (14 of them DPP) where the layout of
// wave_bitonic takes 21 + 6 log2(E); what the k-NN paths sort is E <= 2 keys per lane, and their layout is part of
// their merges, so they keep theirs.
__device__ __forceinline__ unsigned long long lane_xor_u64(unsigned long long v, int x) {
    if (x == 1) return dpp_u64<kQuadXor1>(v);
    if (x == 2) return dpp_u64<kQuadXor2>(v);
    if (x == 8) return dpp_u64<kRowRor + 8>(v);
    return shfl_xor_u64(v, x);
}
// The steps j = j0, j0 / 2 .. 1 (j0 <= 32 E): elements e and e ^ j meet, the lower one keeps the smaller key where
// (e & kk) == 0 and the larger one elsewhere; kk = 0: ascending everywhere (the tail of a merge whose steps j >= 64 E ran
// between waves, sliced_wasserstein.hip).
template <int E>
__device__ __forceinline__ void lane_major_bitonic_steps(unsigned long long (&v)[E], int lane, int kk, int j0) {
#pragma unroll
    for (int j = j0; j > 0; j >>= 1) {
        if (j < E) {
#pragma unroll
            for (int h = 0; h < E; h++) {
                if (h & j) continue;
                const bool asc = ((lane * E + h) & kk) == 0;
                const unsigned long long a = v[h], b = v[h | j];
                const bool sw = asc ? b < a : a < b;
                v[h] = sw ? b : a;
                v[h | j] = sw ? a : b;
            }
        } else {
#pragma unroll
            for (int h = 0; h < E; h++) {
                const int i = lane * E + h;
                const unsigned long long o = lane_xor_u64(v[h], j / E);
                const bool take_min = ((i & j) == 0) == ((i & kk) == 0);
                v[h] = take_min == (o < v[h]) ? o : v[h];
            }
        }
    }
}
// Ascending bitonic sort of the wave's 64 E distinct keys, element e = lane E + h in v[h].
template <int E>
__device__ __forceinline__ void lane_major_bitonic(unsigned long long (&v)[E], int lane) {
#pragma unroll
    for (int kk = 2; kk <= 64 * E; kk <<= 1) lane_major_bitonic_steps(v, lane, kk, kk >> 1);
}

// One window of the sorted searches: the candidate blocks b0 + [0, 128) of sample smp (boxes box[smp][nb][8]: lo xyz,
// pad, hi xyz, pad) ordered nearest first by the gap between their box and the group's box [glo, ghi].  A block's key is
// chain(dx, dy, dz) of the three gaps -- the caller's own distance chain: every step is monotone, so in f32 it is a true
// lower bound of every distance the caller computes between the two boxes -- with its 7 lowest mantissa bits replaced by
// the block's slot (positive floats order like unsigned integers; the truncation only lowers the bound).  Blocks past nb
// key as 0xffffffff.  The sorted keys are element lane + 64 h of key[h]; window_key reads the p-th.
template <class Chain>
__device__ __forceinline__ void sort_box_window(unsigned (&key)[2], const float *box, int smp, int nb, int b0, float4 glo,
                                                float4 ghi, int lane, Chain chain) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int blk = b0 + lane + 64 * h;
        key[h] = 0xffffffffu;
        if (blk < nb) {
            const float4 *cb = reinterpret_cast<const float4 *>(box + ((size_t)smp * nb + blk) * 8);
            const float4 lo = cb[0], hi = cb[1];
            const float dx = fmaxf(fmaxf(glo.x - hi.x, lo.x - ghi.x), 0.f);
            const float dy = fmaxf(fmaxf(glo.y - hi.y, lo.y - ghi.y), 0.f);
            const float dz = fmaxf(fmaxf(glo.z - hi.z, lo.z - ghi.z), 0.f);
            key[h] = (__float_as_uint(chain(dx, dy, dz)) & ~127u) | (unsigned)(lane + 64 * h);
        }
    }
    wave_bitonic(key, lane);
}

// the p-th key of a window sorted by sort_box_window (p wave-uniform, < 128)
__device__ __forceinline__ unsigned window_key(const unsigned (&key)[2], int p) {
    const int pl = __builtin_amdgcn_readfirstlane(p) & 63;
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)key[0], pl);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)key[1], pl);
    return p < 64 ? lo : hi;
}

}  // namespace pcc
