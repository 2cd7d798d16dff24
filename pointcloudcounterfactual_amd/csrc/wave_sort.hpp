// Wave-level helpers of the k-NN and nearest-neighbour searches (knn_lowdim.hip, knn_wide.hip, nn_sorted.hip), gfx950 wave64.
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
