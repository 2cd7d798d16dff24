// Cross-lane idioms of the kernels, gfx950 wave64: DPP moves under their names, reductions over a row of 16 lanes and
// over the wave, the segmented prefix sum and the run scatter of the backwards along an index list.  A DPP operand is a cross-lane VALU read: no trip through the LDS crossbar (ds_bpermute, what __shfl_*
// compiles to).  A row is 16 consecutive lanes, a quad 4.
#pragma once
#include <hip/hip_runtime.h>

namespace pcc {

// dpp_ctrl words: which lane a lane reads.
enum DppCtrl : int {
    kQuadXor1 = 0xB1,       // quad_perm:[1,0,3,2]: lane ^ 1
    kQuadXor2 = 0x4E,       // quad_perm:[2,3,0,1]: lane ^ 2
    kRowShr = 0x110,        // + n, 1..15: row_shr:n, lane i - n of the row (the first n lanes of a row have no source)
    kRowRor = 0x120,        // + n, 1..15: row_ror:n, lane i - n of the row, rotating (n = 8: lane ^ 8)
    kRowMirror = 0x140,     // row_mirror: lane 15 - i of the row
    kRowHalfMirror = 0x141, // row_half_mirror: lane 7 - i of the half row
    kRowBcast15 = 0x142,    // row_bcast:15: lane 15 of the row before (rows without one: none)
    kRowBcast31 = 0x143,    // row_bcast:31: lane 31, for rows 2 and 3
};

// The value of the lane CTRL selects.  A lane without a source, or in a row outside ROW_MASK (bit r: row r), gets `old`
// (BOUND_CTRL: 0 instead of `old` for a missing source).
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ int dpp(int v, int old = 0) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, BOUND_CTRL); }
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ unsigned dpp(unsigned v, unsigned old = 0) { return (unsigned)dpp<CTRL, ROW_MASK, BOUND_CTRL>((int)v, (int)old); }
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp(float v, float old = 0.f) { return __int_as_float(dpp<CTRL, ROW_MASK, BOUND_CTRL>(__float_as_int(v), __float_as_int(old))); }
template <int N, class T>
__device__ __forceinline__ T row_ror(T v) { return dpp<kRowRor + N>(v); }

// op (commutative) over the 16 lanes of a row, in every lane: pairs, quads, half rows, rows -- the xor butterfly's tree:
template <class Op>
__device__ __forceinline__ float row_reduce16(float v, Op op) {
    v = op(v, dpp<kQuadXor1, 0xf, true>(v));
    v = op(v, dpp<kQuadXor2, 0xf, true>(v));
    v = op(v, dpp<kRowHalfMirror, 0xf, true>(v));
    return op(v, dpp<kRowMirror, 0xf, true>(v));
}
// ... and by four rotations of the row (another tree: not the same bits for a sum):
template <class Op>
__device__ __forceinline__ float row_reduce16_ror(float v, Op op) {
    v = op(v, row_ror<8>(v));
    v = op(v, row_ror<4>(v));
    v = op(v, row_ror<2>(v));
    return op(v, row_ror<1>(v));
}

// Sums over the 64 lanes.  `down` (offsets 32 .. 1) leaves the result in lane 0 only; `xor` (offsets 1 .. 32) in every
// lane.  The two trees differ: for a float sum they are not the same bits, so a site keeps its form.
__device__ __forceinline__ float wave_sum_down(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const int lo = __shfl_xor((int)(unsigned)v, m, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), m, 64);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// How many lanes below this one have their bit set in `mask` (a __ballot): the slot of a lane that appends to a list
// the wave fills in lane order (v_mbcnt_lo / v_mbcnt_hi).
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// u where keep is all ones, +0 where it is 0.  Bit arithmetic and not a select: see seg_prefix_sum.
__device__ __forceinline__ float keep_bits(float u, int keep) { return __int_as_float(__float_as_int(u) & keep); }

// Segmented inclusive prefix sum over the 64 lanes: every lane ends with the sum of its segment's lanes up to itself.
// Six steps, fixed order (so fixed bits): row_shr 1 2 4 8 inside the rows of 16 lanes, then lane 15 / 47 into the next
// row (rows 1 and 3), then lane 31 into the upper half (rows 2 and 3).  The caller says, per lane and step, whether the
// step's partner belongs to the lane's segment (all ones) or not (0; also where the step gives the lane no partner);
// the masks depend on the segments alone, so one set serves every value summed over them.
// The partner's value is taken by ALL lanes and then masked with bit arithmetic: written as a select, the compiler moves
// the DPP move under the mask's exec mask, and a lane whose own mask is clear is then an inactive -- invalid -- source
// for its neighbour.
struct SegMasks {
    int shr1, shr2, shr4, shr8, bcast15, bcast31;
};
__device__ __forceinline__ float seg_prefix_sum(float v, const SegMasks &m) {
    v += keep_bits(dpp<kRowShr + 1>(v), m.shr1);
    v += keep_bits(dpp<kRowShr + 2>(v), m.shr2);
    v += keep_bits(dpp<kRowShr + 4>(v), m.shr4);
    v += keep_bits(dpp<kRowShr + 8>(v), m.shr8);
    v += keep_bits(dpp<kRowBcast15, 0xa>(v), m.bcast15);
    return v + keep_bits(dpp<kRowBcast31, 0xc>(v), m.bcast31);
}

// The runs of equal consecutive targets t among the 64 lanes of a wave (consecutive entries of an index list), as the
// segments of seg_prefix_sum.  Bit l of `heads` = lane l opens a run, `head` is the lane that opens this lane's run; a
// lane adds its partner at a step of the prefix sum iff the partner is not before the head of the lane's run.  `tail`:
// the lane is the last of its run and the run's target is a point (t >= 0; the entries without one form runs of -1,
// summed like any other but never added anywhere).  Every lane of the wave must be here (shuffle, ballot, and the DPP
// moves that follow): the caller walks its list in whole waves under a wave-uniform bound.
struct WaveRuns {
    SegMasks masks;
    bool tail;
};
__device__ __forceinline__ WaveRuns wave_runs(int t, int lane) {
    const int lr = lane & 15;
    const int tp = __shfl_up(t, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || tp != t);
    const int head = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    return {{-(int)(lr >= 1 && lane - 1 >= head), -(int)(lr >= 2 && lane - 2 >= head), -(int)(lr >= 4 && lane - 4 >= head),
             -(int)(lr >= 8 && lane - 8 >= head), -(int)((lane & 16) != 0 && lane - lr - 1 >= head),
             -(int)(lane >= 32 && 31 >= head)},
            t >= 0 && (lane == 63 || ((heads >> ((lane + 1) & 63)) & 1ull) != 0)};
}
// The scatter of a backward along such a list: v[cc], this lane's term for channel cc < cb, is summed over the lane's run
// (channel by channel, the six steps of seg_prefix_sum: fixed bits), and the tail lane of every run calls add(cc, sum) for
// the channels in ascending order -- one atomic per run and channel where 64 lanes on one address would serialise.
template <int CB, class Add>
__device__ __forceinline__ void scatter_runs(float (&v)[CB], int cb, int t, int lane, Add add) {
    const WaveRuns runs = wave_runs(t, lane);
#pragma unroll
    for (int cc = 0; cc < CB; cc++) v[cc] = seg_prefix_sum(v[cc], runs.masks);
    if (runs.tail) {
#pragma unroll
        for (int cc = 0; cc < CB; cc++)
            if (cc < cb) add(cc, v[cc]);
    }
}

// Maximum of a 64-bit key: over the 16 lanes of a row in every lane of the row (the tree of row_reduce16, both halves of
// the key through DPP), and over the wave as a wave-uniform value (the four row results read back with v_readlane).
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
    const unsigned lo = dpp<CTRL, 0xf, true>((unsigned)v), hi = dpp<CTRL, 0xf, true>((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long row_max16_u64(unsigned long long v) {
    v = max_u64(v, dpp_u64<kQuadXor1>(v));
    v = max_u64(v, dpp_u64<kQuadXor2>(v));
    v = max_u64(v, dpp_u64<kRowHalfMirror>(v));
    return max_u64(v, dpp_u64<kRowMirror>(v));
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = row_max16_u64(v);
    return max_u64(max_u64(readlane_u64(v, 0), readlane_u64(v, 16)), max_u64(readlane_u64(v, 32), readlane_u64(v, 48)));
}
}  // namespace pcc
