// Submanifold sparse convolution on the slots of pcc_grid_cluster (pcc_cell_neighbours, pcc_sparse_conv,
// include/pcc_neighbour.h), gfx950, wave64.  Nothing is atomic, every word is written once.
//   * cell_nbr_kernel: the kernel map.  A workgroup owns kMapSlots slots of one cloud.  The cloud's ascending list of kept
//     cells (cell[order[seg[r]]], r < min(U, m): at most 64 KB) goes to LDS; a thread owns a row of taps -- one (slot, di, dj)
//     and the ksize offsets along dk --, decomposes the slot's cell BEFORE it adds the offsets (a tap outside [0, res)^3 is
//     -1, never the cell the flat sum would wrap to), finds the row's first target by bisection over the whole list and every
//     later one by a bisection over the `dilation` entries behind the last bound (the cells are distinct, so at most
//     `dilation` of them lie between two targets: one probe for dilation 1), and stores its ksize words side by side.
//   * sparse_conv_mfma_kernel<NOT, VEC> (c >= 8 and o >= 16): the gather-GEMM on v_mfma_f32_16x16x4_f32, described above it.
//   * sparse_conv_kernel<OB> (narrower layers): the gather-GEMM as a VALU register tile.  A wave owns kRowTile = 64 consecutive
//     slots, a lane one slot and OB output channels in registers.  Per tap the lane reads its neighbour's index; a tap that is
//     empty for the whole wave is skipped (the slots are in cell order, so a wave's slots are neighbours in space); otherwise
//     every channel is one gathered word of x per lane (+0 in a lane whose tap is empty) against OB weights that are the same
//     for the whole wave: the compiler reads them with scalar loads and multiplies with v_pk_fma_f32, so they cost no vector
//     register, no LDS and no vector-memory instruction.  (Scalar loads return out of order, so every channel waits for its own
//     weights: measured at c = o = 64 this kernel reached 3 to 12 % of the f32 peak and lost to the MFMA kernel)
// In both x stays channels-major: consecutive slots are mostly consecutive cells, whose neighbours at one tap are mostly
// consecutive slots again, so the gathers of one channel fall into a few cache lines.  The [b, c, m, t] tensor never exists.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>

#include "pcc_common.hpp"
#include "pcc_neighbour.h"

namespace {

constexpr int kMaxPoints = 16384;  // pcc_voxel_index's limit: a cloud's kept cells fit 64 KB of LDS
constexpr int kMapThreads = 256;   // threads of cell_nbr_kernel
constexpr int kMapSlots = 256;     // slots per workgroup of cell_nbr_kernel
constexpr int kRowTile = 64;       // slots per workgroup (one wave) of sparse_conv_kernel
constexpr int kMaxOb = 64;         // output channels per thread at the most; the instantiations are 8, 16, 32, 64
constexpr int kMaxGridY = 65535;   // blocks of output channels per launch; the kernel strides over the blocks beyond

__global__ __launch_bounds__(kMapThreads) void cell_nbr_kernel(int n, int m, int res, int ksize, int dil, const int32_t *__restrict__ cell,
                                                               const int32_t *__restrict__ order, const int32_t *__restrict__ seg,
                                                               const int32_t *__restrict__ n_cells, int64_t *__restrict__ nbr) {
    extern __shared__ int kept_cell[];  // [kept], ascending
    const size_t smp = blockIdx.y;
    const int tid = threadIdx.x;
    const int kept = min(max(n_cells[smp], 0), m);
    const int32_t *cb = cell + smp * n, *ob = order + smp * n, *sb = seg + smp * ((size_t)m + 1);
    for (int r = tid; r < kept; r += kMapThreads) {  // (an entry that names no point: no cell; never dereferenced)
        const unsigned s = (unsigned)sb[r];
        const unsigned p = s < (unsigned)n ? (unsigned)ob[s] : ~0u;
        kept_cell[r] = p < (unsigned)n ? cb[p] : -1;
    }
    __syncthreads();
    const int h = (ksize - 1) / 2, rows = ksize * ksize, cells = res * res * res;
    const int r0 = blockIdx.x * kMapSlots, slots = min(kMapSlots, m - r0);
    for (int item = tid; item < slots * rows; item += kMapThreads) {
        const int r = r0 + item / rows, row = item % rows;
        int64_t *dst = nbr + ((smp * m + r) * rows + row) * ksize;
        const int v = r < kept ? kept_cell[r] : -1;
        const int i = v / (res * res) + dil * (row / ksize - h), j = v / res % res + dil * (row % ksize - h), k0 = v % res - dil * h;
        if ((unsigned)v >= (unsigned)cells || (unsigned)i >= (unsigned)res || (unsigned)j >= (unsigned)res) {
            for (int u = 0; u < ksize; u++) dst[u] = -1;
            continue;
        }
        const int base = (i * res + j) * res;
        int pos = 0;  // the first entry of the list that is >= the last target looked for
        bool first = true;
        for (int u = 0; u < ksize; u++) {
            const int k = k0 + u * dil;
            int64_t found = -1;
            if ((unsigned)k < (unsigned)res) {
                const int want = base + k;
                int lo = pos, hi = first ? kept : min(pos + dil, kept);  // the lower bound of `want` lies in [lo, hi]
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (kept_cell[mid] < want) lo = mid + 1;
                    else hi = mid;
                }
                pos = lo;
                first = false;
                if (pos < kept && kept_cell[pos] == want) found = pos;
            }
            dst[u] = found;
        }
    }
}

// OB output channels from o0 of one slot per lane.  FULL: the block lies inside a row of the weights (o0 + OB <= o), so the
// OB weights of a channel are one run of words; otherwise the words behind the row's end are never read (the index is
// clamped) and never stored.
template <int OB, bool FULL>
__device__ __forceinline__ void conv_block(int c, int o, int n, int m, int t, int o0, int r, const float *__restrict__ xb,
                                           const int64_t *__restrict__ list, const float *__restrict__ weight,
                                           const float *__restrict__ bias, float *__restrict__ ob) {
    float acc[OB];
#pragma unroll
    for (int j = 0; j < OB; j++) acc[j] = 0.f;
    bool some = false;
    for (int tap = 0; tap < t; tap++) {
        const long long idx = r < m ? list[tap] : -1;
        const bool valid = pcc::in_range(idx, n);
        if (!__any(valid)) continue;  // nobody in the wave has a neighbour here
        some |= valid;
        const float *xr = xb + (valid ? (int)idx : 0);
        const float *w = weight + (size_t)tap * c * o + o0;  // (the same for every lane: scalar loads)
#pragma unroll 4
        for (int ch = 0; ch < c; ch++) {
            const float got = xr[(size_t)ch * n];
            const float xv = valid ? got : 0.f;
            const float *wr = w + (size_t)ch * o;
#pragma unroll
            for (int j = 0; j < OB; j++) acc[j] = __builtin_fmaf(xv, wr[FULL ? j : min(j, o - 1 - o0)], acc[j]);
        }
    }
    if (r >= m) return;
#pragma unroll
    for (int j = 0; j < OB; j++) {
        if (!FULL && o0 + j >= o) continue;
        // a row with no neighbour at all is a padded slot: +0, without the bias
        const float bv = bias ? bias[o0 + j] : 0.f;
        ob[(size_t)j * m] = some ? acc[j] + bv : 0.f;
    }
}

template <int OB>
__global__ __launch_bounds__(kRowTile) void sparse_conv_kernel(int c, int o, int n, int m, int t, const float *__restrict__ x,
                                                               const int64_t *__restrict__ nbr, const float *__restrict__ weight,
                                                               const float *__restrict__ bias, float *__restrict__ out) {
    const size_t smp = blockIdx.z;
    const int r = blockIdx.x * kRowTile + threadIdx.x;
    const float *xb = x + smp * c * n;
    const int64_t *list = nbr + (smp * m + min(r, m - 1)) * t;
    for (int o0 = blockIdx.y * OB; o0 < o; o0 += gridDim.y * OB) {  // (once, unless o > kMaxGridY * OB)
        float *ob = out + (smp * o + o0) * m + r;
        if (o0 + OB <= o) conv_block<OB, true>(c, o, n, m, t, o0, r, xb, list, weight, bias, ob);
        else conv_block<OB, false>(c, o, n, m, t, o0, r, xb, list, weight, bias, ob);
    }
}

// f(std::integral_constant<int, OB>) for the smallest instantiated block that holds o channels, kMaxOb above that
template <class F>
void dispatch_ob(int o, F &&f) {
    if (o <= 8) f(std::integral_constant<int, 8>{});
    else if (o <= 16) f(std::integral_constant<int, 16>{});
    else if (o <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, kMaxOb>{});
}

// ---------------------------------------------------------------------------------------------------
// c >= kMfmaMinC and o >= kMfmaMinO: the same sum on v_mfma_f32_16x16x4_f32 (exact f32: an fmaf chain).  The MFMA computes
// D[oc][slot] += W[oc][ch] * X[ch][slot] for 16 output channels, 16 slots and 4 channels: lane l supplies A = W[oc = l & 15]
// [ch = l >> 4] and B = X[ch = l >> 4][slot = l & 15] and holds D[oc = 4 * (l >> 4) + reg][slot = l & 15] in four registers.
// A wave owns kMfmaNt tiles of 16 consecutive slots and NOT tiles of 16 output channels; row i of channel tile ot is the
// output channel o0 + NOT * i + ot, so that the NOT weights a lane needs for one channel are consecutive words: one load of
// NOT floats (VEC: o is a multiple of NOT and weight itself starts on a 4 * NOT-byte boundary, which launch_mfma checks, so
// the load is aligned and lies inside the row or outside it as a whole; any other weight takes the scalar loads).  Per four
// channels a lane loads NOT weights and one gathered word of x per slot tile for NOT * kMfmaNt MFMAs: the operands a
// VALU tile re-reads per output channel are loaded once per 16.  A tap that is empty for a whole tile of 16 slots is skipped
// for that tile: a quarter of the VALU kernel's wave, so more taps are skipped and fewer lanes are zero-filled.
// ---------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int kMfmaTile = 16;  // slots per MFMA tile: the granularity at which an empty tap is skipped
constexpr int kMfmaNt = 2;     // slot tiles per wave
constexpr int kMfmaSteps = 4;  // k-steps (of 4 channels) whose loads are in flight together
constexpr int kMfmaWaves = 4;  // waves per workgroup (they share nothing but the cache lines of the weights)
constexpr int kMfmaRows = kMfmaTile * kMfmaNt * kMfmaWaves;  // slots per workgroup
constexpr int kMfmaMinC = 8, kMfmaMinO = 16;  // below: the VALU tile (a k-step is 4 channels, a channel tile 16 outputs)

template <int NOT, bool VEC>
__global__ __launch_bounds__(64 * kMfmaWaves) void sparse_conv_mfma_kernel(int c, int o, int n, int m, int t, const float *__restrict__ x,
                                                                            const int64_t *__restrict__ nbr, const float *__restrict__ weight,
                                                                            const float *__restrict__ bias, float *__restrict__ out) {
    const size_t smp = blockIdx.z;
    const int lane = threadIdx.x & 63, j = lane & 15, kk = lane >> 4;
    const int r0 = blockIdx.x * kMfmaRows + (threadIdx.x >> 6) * (kMfmaTile * kMfmaNt);
    if (r0 >= m) return;  // (the whole wave: there is no barrier below)
    const float *xb = x + smp * c * n;
    for (int o0 = blockIdx.y * 16 * NOT; o0 < o; o0 += gridDim.y * 16 * NOT) {  // (once, unless o > kMaxGridY * 16 * NOT)
        f32x4 acc[kMfmaNt][NOT];
        bool some[kMfmaNt];
#pragma unroll
        for (int nt = 0; nt < kMfmaNt; nt++) {
            some[nt] = false;
#pragma unroll
            for (int ot = 0; ot < NOT; ot++) acc[nt][ot] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int oc0 = o0 + NOT * j;  // the first of this lane's NOT output channels as the A operand
        const int64_t *list[kMfmaNt];
        bool inside[kMfmaNt];
        long long next[kMfmaNt];  // the indices of the next tap: their loads fly during this tap's channels
#pragma unroll
        for (int nt = 0; nt < kMfmaNt; nt++) {
            const int r = r0 + nt * kMfmaTile + j;
            inside[nt] = r < m;
            list[nt] = nbr + (smp * m + min(r, m - 1)) * t;  // (a row behind the last slot reads the last slot's and drops it)
            next[nt] = list[nt][0];
        }
        for (int tap = 0; tap < t; tap++) {
            int at[kMfmaNt];
            bool valid[kMfmaNt], any[kMfmaNt];
#pragma unroll
            for (int nt = 0; nt < kMfmaNt; nt++) {
                const long long idx = next[nt];
                next[nt] = list[nt][min(tap + 1, t - 1)];
                valid[nt] = inside[nt] && pcc::in_range(idx, n);
                at[nt] = valid[nt] ? (int)idx : 0;
                any[nt] = __any(valid[nt]);
                some[nt] |= valid[nt];
            }
            const float *wt = weight + (size_t)tap * c * o;
            // The channels of one tap for the slot tiles that have it (T0, T1: wave-uniform), kMfmaSteps k-steps at a time:
            // straight-line code that issues every load of the k-steps before the first MFMA waits for its operands.  (Left
            // to `#pragma unroll` the compiler kept one k-step per iteration: load, wait, four MFMAs.)  The channels behind
            // c are clamped loads whose values are replaced by +0.
            auto channels = [&](auto T0, auto T1) {
                constexpr bool on[kMfmaNt] = {decltype(T0)::value, decltype(T1)::value};
                for (int ch0 = 0; ch0 < c; ch0 += 4 * kMfmaSteps) {
                    float a[kMfmaSteps][NOT], xv[kMfmaSteps][kMfmaNt];
#pragma unroll
                    for (int u = 0; u < kMfmaSteps; u++) {
                        const int ch = min(ch0 + 4 * u + kk, c - 1);
                        const float *wr = wt + (size_t)ch * o;
                        if (VEC) {
                            const float *p = wr + (oc0 < o ? oc0 : 0);
                            if constexpr (NOT == 4) {
                                const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
                                a[u][0] = v.x, a[u][1] = v.y, a[u][2] = v.z, a[u][3] = v.w;
                            } else if constexpr (NOT == 2) {
                                const f32x2 v = *reinterpret_cast<const f32x2 *>(p);
                                a[u][0] = v.x, a[u][1] = v.y;
                            } else {
                                a[u][0] = *p;
                            }
                        } else {
#pragma unroll
                            for (int ot = 0; ot < NOT; ot++) a[u][ot] = wr[min(oc0 + ot, o - 1)];
                        }
#pragma unroll
                        for (int nt = 0; nt < kMfmaNt; nt++)
                            if (on[nt]) xv[u][nt] = xb[(size_t)ch * n + at[nt]];
                    }
                    __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks every load to just before its MFMAs)
#pragma unroll
                    for (int u = 0; u < kMfmaSteps; u++) {
                        const bool chv = ch0 + 4 * u + kk < c;
#pragma unroll
                        for (int ot = 0; ot < NOT; ot++) a[u][ot] = chv && oc0 + (VEC ? 0 : ot) < o ? a[u][ot] : 0.f;
#pragma unroll
                        for (int nt = 0; nt < kMfmaNt; nt++) {
                            if (!on[nt]) continue;
                            const float b = valid[nt] && chv ? xv[u][nt] : 0.f;
#pragma unroll
                            for (int ot = 0; ot < NOT; ot++)
                                acc[nt][ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][ot], b, acc[nt][ot], 0, 0, 0);
                        }
                    }
                }
            };
            static_assert(kMfmaNt == 2, "the three cases below are those of two slot tiles");
            if (any[0] && any[1]) channels(std::true_type{}, std::true_type{});
            else if (any[0]) channels(std::true_type{}, std::false_type{});
            else if (any[1]) channels(std::false_type{}, std::true_type{});  // (neither: no slot of the wave has a neighbour here)
        }
#pragma unroll
        for (int nt = 0; nt < kMfmaNt; nt++) {
            const int r = r0 + nt * kMfmaTile + j;
            if (r >= m) continue;
#pragma unroll
            for (int ot = 0; ot < NOT; ot++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int oc = o0 + NOT * (4 * kk + reg) + ot;
                    if (oc >= o) continue;
                    // a row with no neighbour at all is a padded slot: +0, without the bias
                    const float bv = bias ? bias[oc] : 0.f;
                    out[(smp * o + oc) * m + r] = some[nt] ? acc[nt][ot][reg] + bv : 0.f;
                }
        }
    }
}

template <int NOT>
void launch_mfma(int b, int c, int o, int n, int m, int t, const float *x, const int64_t *nbr, const float *weight, const float *bias,
                 float *out, hipStream_t st) {
    // (the profile tells the variants apart behind one prefix per tile: the tests read either)
    static const char *const names[][5] = {
        {"", "sparse_conv_mfma_kernel<16>", "sparse_conv_mfma_kernel<32>", "", "sparse_conv_mfma_kernel<64>"},
        {"", "sparse_conv_mfma_kernel<16> scalar weights", "sparse_conv_mfma_kernel<32> scalar weights", "",
         "sparse_conv_mfma_kernel<64> scalar weights"}};
    // (weight is the caller's pointer: any 4-byte-aligned address is legal, the wide load is taken only on a 4 * NOT-byte one)
    const bool vec = o % NOT == 0 && (reinterpret_cast<uintptr_t>(weight) & (4 * NOT - 1)) == 0;
    pcc::ProfScope prof(names[vec ? 0 : 1][NOT], st);
    const dim3 grid((unsigned)pcc::ceil_div(m, kMfmaRows), (unsigned)std::min(pcc::ceil_div(o, 16 * NOT), kMaxGridY), (unsigned)b);
    if (vec)
        hipLaunchKernelGGL((sparse_conv_mfma_kernel<NOT, true>), grid, dim3(64 * kMfmaWaves), 0, st, c, o, n, m, t, x, nbr, weight, bias, out);
    else
        hipLaunchKernelGGL((sparse_conv_mfma_kernel<NOT, false>), grid, dim3(64 * kMfmaWaves), 0, st, c, o, n, m, t, x, nbr, weight, bias, out);
}

}  // namespace

extern "C" {

int pcc_cell_neighbours(int b, int n, int m, int res, int ksize, int dilation, const int32_t *cell, const int32_t *order,
                        const int32_t *seg, const int32_t *n_cells, int64_t *nbr, pcc_stream_t stream) {
    const char *name = "cell_neighbours";
    pcc::clear_error();
    if (b < 0) return pcc::invalidf("%s: b must be >= 0", name);
    if (n < 1 || n > kMaxPoints) return pcc::invalidf("%s: n must be in [1, %d]", name, kMaxPoints);
    if (m < 1 || m > n) return pcc::invalidf("%s: m must be in [1, n]", name);
    if (res < 2 || res > 128) return pcc::invalidf("%s: res must be in [2, 128]", name);
    if (ksize != 3 && ksize != 5) return pcc::invalidf("%s: ksize must be 3 or 5", name);
    if (dilation < 1) return pcc::invalidf("%s: dilation must be >= 1", name);
    if (b > 65535) return pcc::invalidf("%s: batch too large (b > 65535)", name);
    if ((long long)b * m * ksize * ksize * ksize > INT_MAX) return pcc::invalidf("%s: map too large (b * m * ksize^3 >= 2^31)", name);
    if (b == 0) return PCC_OK;
    if (!cell || !order || !seg || !n_cells || !nbr) return pcc::invalidf("%s: null pointer", name);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t attr = pcc::allow_lds<cell_nbr_kernel>((size_t)kMaxPoints * sizeof(int));
    if (attr != hipSuccess) {
        pcc::set_error((int)attr, "cell_neighbours: cannot reserve the cell list's LDS");
        return (int)attr;
    }
    // (a dilation of res or more reaches no cell but the centre: min keeps dil * ksize inside an int)
    pcc::ProfScope prof("cell_nbr_kernel", st);
    hipLaunchKernelGGL(cell_nbr_kernel, dim3((unsigned)pcc::ceil_div(m, kMapSlots), (unsigned)b), dim3(kMapThreads), (size_t)m * sizeof(int), st,
                       n, m, res, ksize, std::min(dilation, res), cell, order, seg, n_cells, nbr);
    return pcc::check_launch(name);
}

int pcc_sparse_conv(int b, int c, int o, int n, int m, int t, const float *x, const int64_t *nbr, const float *weight,
                    const float *bias, float *out, pcc_stream_t stream) {
    const char *name = "sparse_conv";
    pcc::clear_error();
    if (int rc = pcc::check_list_sizes(name, b, c, n, m, t)) return rc;
    if (o < 1 || m < 1) return pcc::invalidf("%s: bad size", name);
    if ((long long)c * o * t > INT_MAX) return pcc::invalidf("%s: weight too large (t * c * o >= 2^31)", name);
    if (b == 0) return PCC_OK;
    if (!x || !nbr || !weight || !out) return pcc::invalidf("%s: null pointer", name);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (c >= kMfmaMinC && o >= kMfmaMinO) {
        if (o <= 16) launch_mfma<1>(b, c, o, n, m, t, x, nbr, weight, bias, out, st);
        else if (o <= 32) launch_mfma<2>(b, c, o, n, m, t, x, nbr, weight, bias, out, st);
        else launch_mfma<4>(b, c, o, n, m, t, x, nbr, weight, bias, out, st);
        return pcc::check_launch(name);
    }
    dispatch_ob(o, [&](auto OB) {
        static const char *const names[] = {"sparse_conv_kernel<8>", "sparse_conv_kernel<16>", "sparse_conv_kernel<32>", "sparse_conv_kernel<64>"};
        pcc::ProfScope prof(names[OB == 8 ? 0 : OB == 16 ? 1 : OB == 32 ? 2 : 3], st);
        hipLaunchKernelGGL((sparse_conv_kernel<OB>), dim3((unsigned)pcc::ceil_div(m, kRowTile), (unsigned)std::min(pcc::ceil_div(o, (int)OB), kMaxGridY), (unsigned)b),
                           dim3(kRowTile), 0, st, c, o, n, m, t, x, nbr, weight, bias, out);
    });
    return pcc::check_launch(name);
}

}  // extern "C"
