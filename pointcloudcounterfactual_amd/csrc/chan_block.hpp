// Channel-block workgroups of the index-driven copies (graph_ops.hip, grouping.hip, interpolate.hip, attention.hip,
// kpconv.hip): a workgroup owns CB channels of one sample and keeps their rows of x, or their gradient bins, in LDS.  How
// the ids are dealt, how much LDS a workgroup may take, how CB is chosen, how the kernel template is picked for it, how the
// list of a sample is split over several such workgroups and how many threads each gets, the protocol of the bins, and the
// padded tile of list rows that attention.hip and kpconv.hip stage.
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

// position of cb in {1, 2, 4, 8, 16}: the row of a launcher's table of launch-profile names, which carry the instantiation
inline int cb_index(int cb) { return cb >= 16 ? 4 : cb >= 8 ? 3 : cb >= 4 ? 2 : cb >= 2 ? 1 : 0; }

// f(std::integral_constant<int, cb>) for cb a power of two <= CB_MAX
template <int CB_MAX = 8, class F>
void dispatch_cb(int cb, F &&f) {
    if constexpr (CB_MAX > 1) {
        if (cb < CB_MAX) return dispatch_cb<CB_MAX / 2>(cb, f);
    }
    f(std::integral_constant<int, CB_MAX>{});
}

// ---- CB channels of a sample x a split of a per-sample list (grouping.hip: the m * k slots; interpolate.hip: the m dense
// points; attention.hip: the dense points forward, the slots backward; kpconv.hip: the slots backward) ----
constexpr int kWgThreads = 1024;         // threads of such a workgroup at the most
constexpr int kCbDirect = 8;             // channels per workgroup of the direct path (nothing to fit)
constexpr long long kMaxGrid = 1 << 20;  // workgroups per launch; the kernels stride over the units beyond
inline unsigned grid_for(long long units) { return (unsigned)(units < kMaxGrid ? units : kMaxGrid); }

// What one pass of a workgroup covers: channels c0 .. c0 + cb - 1 of sample smp, entries lo .. hi - 1 of its list of `len`.
// Unit u of b * nblk * nsplit, the splits of a channel block innermost; consecutive units share an XCD (xcd_contiguous).
struct ListUnit {
    int smp, c0, cb;
    unsigned lo, hi;
};
template <int CB>
__device__ __forceinline__ ListUnit list_unit(long long u, int c, unsigned len, int nsplit, unsigned chunk) {
    const int nblk = (c + CB - 1) / CB;
    const long long blk = u / nsplit;
    const unsigned s = (unsigned)(u - blk * nsplit);
    const int smp = (int)(blk / nblk), c0 = (int)(blk - (long long)smp * nblk) * CB;
    const unsigned lo = s * chunk;  // (< len: no overflow, len < 2^31 and chunk <= len + 63)
    return {smp, c0, min(CB, c - c0), lo, min(len, lo + chunk)};
}

// The gradient bins of a unit in LDS, `words` = cb * n of them, shared by the nt threads of the workgroup: zeroed once the
// previous unit's bins are written out; added into (ds_add_f32); then written out whole once every add is done, so every
// element of the unit's slice of the gradient is written and the host zero-fills nothing.
__device__ __forceinline__ void bins_clear(float *bins, int words, int tid, int nt) {
    __syncthreads();
    for (int i = tid; i < words; i += nt) bins[i] = 0.f;
    __syncthreads();
}
__device__ __forceinline__ void bins_store(float *dst, const float *bins, int words, int tid, int nt) {
    __syncthreads();
    for (int i = tid; i < words; i += nt) dst[i] = bins[i];
}

// Where slot q of a tile of rows of k slots lies in LDS: row q / k (`row`, where the caller has it for more) at the odd
// stride k | 1, so that the lanes of a wave, each walking its own row, hit distinct banks.
__device__ __forceinline__ unsigned padded_at(unsigned q, unsigned k, unsigned row) { return row * (k | 1u) + (q - row * k); }
__device__ __forceinline__ unsigned padded_at(unsigned q, unsigned k) { return padded_at(q, k, q / k); }

// How a call is cut into such workgroups: the path, CB, and into how many pieces the list of a sample is split.
struct ListPlan {
    bool lds;
    int cb, nsplit;
    unsigned chunk;
    size_t lds_bytes;
    long long units;
    unsigned grid() const { return grid_for(units); }
    // Threads per workgroup where they are not simply kWgThreads: one per item of a pass over a unit, or one per 8 words
    // of its LDS tile (staged, or zeroed and written out) if that is more; whole waves, 64 .. kWgThreads.  A unit shorter
    // than a full workgroup's reach (len = 512: 128 lanes with four entries each) would otherwise hold a CU's wave slots
    // with waves that have nothing to do.
    unsigned threads_for(unsigned long long items) const {
        const unsigned long long by_tile = lds_bytes / 32, want = items > by_tile ? items : by_tile;
        const unsigned t = (unsigned)((want > (unsigned)kWgThreads ? (unsigned)kWgThreads : want) + 63) / 64 * 64;
        return t < 64 ? 64 : t;
    }
    // ... where a lane takes `per` entries of a unit of a list of `len`
    unsigned threads(unsigned len, unsigned per) const { return threads_for(((chunk < len ? chunk : len) + per - 1) / per); }
    // LDS bins tie a channel block to one workgroup, and that workgroup walks the whole list of its sample, one LDS atomic
    // per run and channel: while a backward has fewer workgroups than there are compute units, halve the block.  Each
    // halving costs what a workgroup does once per entry whatever its CB: one more read of the index list (attention.hip),
    // one more evaluation of the influences (kpconv.hip).
    void spread_bins(int b, int c) {
        while (lds && cb > 1 && units < device_cus_or(256)) {
            cb /= 2;
            lds_bytes /= 2;
            units = (long long)b * ceil_div(c, cb);
        }
    }
};

// LDS wherever the rows (or bins) of at least one channel of n floats fit a workgroup, the direct path otherwise;
// `forced_path` is the caller's tuning switch (PCC_TUNE_..._PATH): 2 forces the direct path, and a forced LDS path that
// cannot hold n is ignored.  `split_lds`: the entries of a channel block may go to several workgroups (a
// forward, and a backward's direct path: LDS bins cannot be shared) -- used while the call would leave compute units
// idle, down to `min_chunk` entries per workgroup.
inline ListPlan make_list_plan(int b, int c, int n, unsigned len, bool split_lds, unsigned min_chunk, int forced_path) {
    ListPlan p;
    const int cb_lds = fit_cb(8, (size_t)n * sizeof(float));
    const bool fits = (size_t)cb_lds * n * sizeof(float) <= kLdsWg;
    p.lds = fits && forced_path != 2;
    p.cb = p.lds ? cb_lds : kCbDirect;
    p.lds_bytes = p.lds ? (size_t)p.cb * n * sizeof(float) : 0;
    const long long blocks = (long long)b * ceil_div(c, p.cb);
    long long want = 1;
    if (!p.lds || split_lds) {
        want = (2LL * device_cus_or(256) + blocks - 1) / blocks;  // two workgroups per compute unit
        const long long most = (len + min_chunk - 1) / min_chunk;
        want = want < most ? want : most;
        want = want < 1 ? 1 : want;
    }
    p.chunk = (unsigned)(((len + want - 1) / want + 63) / 64 * 64);  // (a multiple of 64: whole waves, whole float4 groups)
    p.nsplit = p.chunk ? (int)((len + p.chunk - 1) / p.chunk) : 1;
    p.units = blocks * p.nsplit;
    return p;
}

}  // namespace pcc
