// k-nearest-neighbour graph for gfx950 (MI355X), wave64: pcc_knn, its entry checks and the choice of path.  The kernels
// are in knn_lowdim.hip (c <= 3), knn_mfma.hip (4 <= c <= 128) and knn_wide.hip.
//
// Replaces knn / pykeops_knn (reference src/utils/neighbour_ops.py:63-82: a PyKeOps argKmin over a lazy
// (B,N,N) squared-distance tensor) -- PyKeOps has no ROCm backend.  Four kernels:
//   * knn_sorted_kernel (c <= 3, n <= 16384): exact difference-form distances on the f32 VALU, the formula the GPU
//     reference evaluates (pykeops_square_distance, :35-40), on the Hilbert-sorted cloud: only the candidate boxes
//     that can still hold one of a query's k nearest are visited (see the kernel).
//   * knn_small_kernel (c <= 3, larger clouds): the same distances, exhaustive.  A lane owns one query; the candidate cloud sits
//     in LDS as SoA rows (x is already channels-major, so staging is a straight coalesced copy); S waves
//     scan disjoint candidate ranges; per-lane buffered top-K (topk.hpp); the S sorted lists are merged
//     with strict '<' in range order, so equal distances come out in ascending index order.
//   * knn_mfma_kernel (c >= 4): expanded form |xi|^2 + |xj|^2 - 2 xi.xj with the inner product on
//     v_mfma_f32_32x32x2_f32 (exact f32 FMA chain per output) -- the formula of the reference's CPU path
//     (self_square_distance, :53-60) and a genuine dense contraction (C = 64..128 in the DGCNN encoder).
//     The 32x32 accumulator tile is oriented with the QUERY on the lane (column) and 16 candidates in
//     the lane's accumulator registers, so the same per-lane top-K consumes distances straight from
//     registers: the (B,N,N) distance matrix never exists in memory.
//   * knn_mfma_split_kernel (c >= 4, launches that fill the chip): the same arithmetic with the matrix waves and the
//     selection waves of a workgroup apart, one query per selection lane (see the kernel).
// These cover k <= 32 and c <= 128; every other call (k up to 128, any c) goes to knn_wide.hip, with the same formulas
// and the same ordering contract.
#include "knn.hpp"
#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"

extern "C" int pcc_knn(int b, int c, int n, int k, const float *x, int64_t *indices, pcc_stream_t stream) {
    pcc::clear_error();
    bool empty;
    if (int rc = knn_check_sizes("knn", "points", b, c, n, n, k, &empty); rc || empty) return rc;
    if (!x || !indices) return pcc::invalid("knn: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // outside the box of the kernels above: knn_wide.hip (the test switch sends every call there)
    if (k > 32 || c > 128 || pcc::tuning(PCC_TUNE_KNN_WIDE) == 1) return pcc::knn_wide(b, c, n, k, x, indices, st);
    if (c <= 3 && n <= kSortedMaxN) return pcc::knn_sorted(b, c, n, k, x, indices, st);
    if (c <= 3) return pcc::knn_small(b, c, n, k, x, indices, st);  // clouds too large for the one-workgroup sort: exhaustive scan
    return pcc::knn_mfma(b, c, n, k, x, indices, st);  // (which of the two MFMA kernels: see launch_mfma)
}
