// What the files of the k-NN graph share (knn.hip, knn_lowdim.hip, knn_mfma.hip, knn_wide.hip).
#pragma once
#include "pcc_common.hpp"

#include <type_traits>

namespace {  // (per translation unit on purpose: kernels and their parameter types keep their names)

typedef float f32x16 __attribute__((ext_vector_type(16)));  // accumulator of v_mfma_f32_32x32x2_f32

constexpr int kCap = 16;     // FIFO slots per lane
constexpr int kSortedMaxN = 16384;  // the sort kernel orders up to 16384 points per cloud

__device__ __forceinline__ f32x16 zero16() {
    return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// The +inf tail of a list.  The exhaustive k <= 32 kernels (knn_small_kernel, knn_mfma_kernel, knn_mfma_split_kernel) take a
// candidate with a strict `x < threshold`, the threshold starting at +inf, and use +inf as their "no candidate" value: a
// +inf distance (a norm or a squared difference that overflows) never enters their lists, though the contract lists it
// like any other distance -- only NaN is left out.  So when the scan ends with fewer than k entries, everything still
// missing is at +inf or NaN, and the row's owner completes it here: the candidates whose distance is exactly +inf, in
// index order, into the slots filled .. k - 1.  dist(j) is the kernel's own distance expression, store(slot, j) writes a
// slot.  Finite clouds never get here; the loop is a plain walk over the cloud in global memory.  -> slots filled.
template <class DistF, class StoreF>
__device__ __forceinline__ int fill_inf_tail(int filled, int k, int n, DistF &&dist, StoreF &&store) {
    for (int j = 0; j < n && filled < k; j++) {
        if (dist(j) == __builtin_inff()) {
            store(filled, j);
            filled++;
        }
    }
    return filled;
}

// the expanded-form distance of candidate j to query q of one cloud xb[c][n], as the MFMA kernels round it: the inner
// product one fma chain in channel order, then (-2 dot + |x_j|^2) + |x_q|^2
__device__ __forceinline__ float expanded_dist(const float *xb, const float *sqb, int c, int n, int q, float sq_q, int j) {
    float dot = 0.f;
    for (int ch = 0; ch < c; ch++) dot = __builtin_fmaf(xb[(size_t)ch * n + j], xb[(size_t)ch * n + q], dot);
    return __builtin_fmaf(-2.0f, dot, sqb[j]) + sq_q;
}

// list slots of the instantiations for k <= 32
constexpr int kSlots[] = {4, 8, 16, 20, 25, 32};

// f(std::integral_constant<int, K>) for the fewest slots K >= k (1 <= k <= 32)
template <int I = 0, class F>
int with_slots(int k, F &&f) {
    if constexpr (I + 1 < (int)(sizeof kSlots / sizeof kSlots[0])) {
        if (k > kSlots[I]) return with_slots<I + 1>(k, f);
    }
    return f(std::integral_constant<int, kSlots[I]>{});
}

// position of the instantiation K in kSlots (the row of a launcher's table of profile names)
constexpr int slot_index(int K) {
    int i = 0;
    for (int s : kSlots) i += s < K;
    return i;
}

// the next smaller instantiation (0 below the first): the sorted kernel of K serves k in (prev_slots(K), K]
constexpr int prev_slots(int K) {
    int p = 0;
    for (int s : kSlots) p = s < K ? s : p;
    return p;
}

// The entry checks pcc_knn ("knn", "points", nq = n) and pcc_knn_cross ("knn_cross", "candidates") share.  *empty: the
// call has nothing to do (PCC_OK).
inline int knn_check_sizes(const char *who, const char *what, int b, int c, int nq, int n, int k, bool *empty) {
    *empty = false;
    if (b < 0 || c < 1 || nq < 0 || n < 0 || k < 1) return pcc::invalidf("%s: bad size", who);
    if (b == 0 || nq == 0) return *empty = true, PCC_OK;
    if (k > n) return pcc::invalidf("%s: k exceeds the number of %s (torch.topk raises too)", who, what);
    if (k > 128) return pcc::invalidf("%s: k > 128 is not supported", who);
    if (b > 65535) return pcc::invalidf("%s: batch too large", who);
    return PCC_OK;
}

}  // namespace

namespace pcc {

// The paths of pcc_knn.  Sizes and pointers already validated by pcc_knn: 1 <= k <= min(n, 128), b <= 65535.
// c <= 3, n <= kSortedMaxN, k <= 32: search on the Hilbert-sorted cloud (knn_lowdim.hip)
int knn_sorted(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st);
// c <= 3, k <= 32: exhaustive scan (knn_lowdim.hip)
int knn_small(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st);
// 4 <= c <= 128, k <= 32: the MFMA kernels (knn_mfma.hip)
int knn_mfma(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st);
// k-NN graph outside the range of those kernels (knn_wide.hip): any c >= 1, 1 <= k <= min(n, 128)
int knn_wide(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st);

// sq[b][n] = sum_c x[b][c][n]^2 as one fma chain in channel order (the oracle's |x_j|^2; knn_mfma.hip's sqnorm_kernel)
void launch_sqnorm(int b, int c, int n, const float *x, float *sq, hipStream_t st);

}  // namespace pcc
