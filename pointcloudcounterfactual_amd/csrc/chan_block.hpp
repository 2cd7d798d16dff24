// Channel-block workgroups of the index-driven copies (graph_ops.hip, grouping.hip): a workgroup owns CB channels of one
// sample and keeps their rows of x, or their gradient bins, in LDS.  How the ids are dealt, how much LDS a workgroup may
// take, how CB is chosen and how the kernel template is picked for it.
#pragma once
#include <cstddef>
#include <type_traits>

#include "pcc_common.hpp"

namespace pcc {

// The CB channels of one sample a workgroup owns: sample `smp`, channels c0 .. c0 + CB - 1 (those below c exist).
// One-dimensional launch, sample-major on XCD-contiguous ids: the channel blocks of a sample share an L2 (they all
// stream the sample's index list; side by side on eight XCDs each would fetch it over the fabric).
struct ChanBlock {
    int smp, c0;
};
template <int CB>
__device__ __forceinline__ ChanBlock chan_block(int c) {
    const int nblk = (c + CB - 1) / CB, lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int smp = lid / nblk;
    return {smp, (lid - smp * nblk) * CB};
}

// LDS per workgroup, in bytes: all of a CU's; that less room for a kernel's static LDS; and the rows or bins of a
// workgroup where two should share a CU
constexpr size_t kLdsWg = 160 * 1024, kLdsWgDyn = kLdsWg - 256, kLdsHalfCu = 64 * 1024;

// channels per workgroup: the largest CB in {cb_max, cb_max / 2, ..., 1} of which `row_bytes` each fit `bytes` (1 if none does)
inline int fit_cb(int cb_max, size_t row_bytes, size_t bytes = kLdsHalfCu) {
    int cb = cb_max;
    while (cb > 1 && cb * row_bytes > bytes) cb >>= 1;
    return cb;
}

// f(std::integral_constant<int, cb>) for cb a power of two <= CB_MAX
template <int CB_MAX = 8, class F>
void dispatch_cb(int cb, F &&f) {
    if constexpr (CB_MAX > 1) {
        if (cb < CB_MAX) return dispatch_cb<CB_MAX / 2>(cb, f);
    }
    f(std::integral_constant<int, CB_MAX>{});
}

}  // namespace pcc
