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
