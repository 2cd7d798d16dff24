// All-pairs Chamfer distances between two banks of clouds for gfx950 (MI355X), wave64: pcc_chamfer_matrix.
//
// The paired entry points (chamfer.hip) score sample b of one batch against sample b of the other; scoring a generated
// SET (minimum matching distance, coverage, 1-NN accuracy) needs every cloud of one bank against every cloud of the
// other.  That matrix needs no argmin and no per-point output, only the two directional sums of minima, so:
//   * ONE distance evaluation serves both directions.  A wave works on a register tile of 64 streamed points x 32 staged
//     points: lane (lq, lc) of an 8 x 8 layout holds 8 streamed points (stride 8 from lq) and reads 4 staged points
//     (one ds_read_b128 per coordinate at lc).  Each of the 32 distances of a lane feeds a running ROW minimum (one per
//     streamed point, in registers for the whole staged chunk, v_min3: 0.5 op per pair) and a COLUMN minimum (one per
//     staged point of the step, v_min3 again).  Written one pair at a time that is 6 + 0.5 + 0.5 = 7 VALU ops per pair
//     for both directions, where nn_fwd_kernel spends 6.9 per pair and direction; the differences, the product and the
//     two fma of TWO staged points go through the packed f32 instructions, 3 + 1 = 4 issued instructions per pair.
//   * the cross-lane part: the column minima of a step are combined over the 8 lq lanes -- the low lane bits, so three
//     DPP v_min_u32 per value -- and folded into the chunk's column minima in LDS with one integer ds_min (distances are
//     non-negative, so their bit patterns order as unsigned integers; a minimum does not depend on the order of its
//     operands).  About 17 instructions per step beside the 128 of its pair work.  The row minima cross lanes once per tile.
//   * a workgroup stages one cloud of the `staged` bank in LDS (SoA, 24 KB per 2048 points) and streams `group` clouds
//     of the other bank past it; consecutive logical workgroup ids share the staged cloud, and pcc::xcd_contiguous puts
//     them on one XCD.
//   * an entry is a fixed-order float32 sum of the minima: per 2048-point block one strided partial per thread, a
//     butterfly inside the wave, the four waves added pairwise; blocks in index order.  Both directions go through this
//     one function on arrays of minima in point order, so an entry depends on the two clouds, n, m and `mean` only --
//     not on which bank was staged, where the clouds sit in their banks, or the grid.
//   * clouds of more than 2048 points: the staged cloud goes through LDS chunk by chunk (the chunk loop of
//     nn_fwd_kernel); the column minima of a chunk are complete when the chunk has met every streamed point, so the
//     two-direction kernel needs the streamed cloud to fit one block.  The host stages whichever bank lets it; when both
//     clouds are larger, each direction runs as a rows-only launch (the cost of the paired composition).
#include "pcc_common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int kT = 256, kWaves = kT / 64;
constexpr int kCH = 2048;           // points per staged chunk and per streamed block
constexpr int kRQ = 8, kRC = 4;     // streamed / staged points per lane and step
constexpr int kTQ = 8 * kRQ;        // streamed points per wave tile
constexpr int kTC = 8 * kRC;        // staged points per step
constexpr unsigned kInfBits = 0x7f800000u;
static_assert(kCH % kTQ == 0 && kCH % kTC == 0, "a chunk holds whole tiles");

struct MatrixArgs {
    const float *q, *c;        // streamed bank [nq][pq][3], staged bank [nc][pc][3]
    int nq, nc, pq, pc;
    int group, groups;         // streamed clouds per workgroup, workgroups per staged cloud
    int swap;                  // 0: streamed = a, staged = bank; 1: the other way round
    int self_mode;             // 0: two banks; 1: one bank, streamed <= staged only, mirrored; 2: one bank, all pairs (rows only)
    int mean, r;               // r: row length of the outputs
    float *d_ab, *d_ba;        // either may be null
};

__device__ __forceinline__ bool non_finite(float v) { return !(__builtin_fabsf(v) < __builtin_inff()); }

// Two point pairs per instruction (v_pk_add / v_pk_mul / v_pk_fma_f32): the same IEEE operations as pcc::sq3, lane by lane.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 sq3x2(f32x2 x, f32x2 y, f32x2 z) {
    return __builtin_elementwise_fma(z, z, __builtin_elementwise_fma(x, x, y * y));
}

// The bits of the minimum of a distance over the 8 lanes that share lane bits 3-5 (quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror).  Distances are >= +0, so their bit patterns order as unsigned integers.
template <int CTRL>
__device__ __forceinline__ unsigned dpp_min(unsigned v) { return min(v, pcc::dpp<CTRL>(v, v)); }
__device__ __forceinline__ unsigned min_over_lq(float d) {
    return dpp_min<pcc::kRowHalfMirror>(dpp_min<pcc::kQuadXor2>(dpp_min<pcc::kQuadXor1>(__builtin_bit_cast(unsigned, d))));
}

// Sum of the floats whose bits are v[0 .. len) (len <= kCH), valid in thread 0: thread t adds v[t], v[t + 256], ... in
// that order, a butterfly adds the 64 partials of a wave, and the four waves are added as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ float block_sum(const unsigned *v, int len, float *part) {
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int k = tid; k < len; k += kT) s += __builtin_bit_cast(float, v[k]);
    s = pcc::wave_sum_xor(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    const float total = (part[0] + part[1]) + (part[2] + part[3]);
    __syncthreads();  // `part` and `v` may be rewritten from here on
    return total;
}

template <bool COL>
__global__ __launch_bounds__(kT) void chamfer_matrix_kernel(MatrixArgs a) {
    __shared__ __attribute__((aligned(16))) float lds_c[3 * kCH];  // x[kCH] | y[kCH] | z[kCH]
    __shared__ unsigned rowmin[kCH];
    __shared__ unsigned colmin[COL ? kCH : 1];
    __shared__ float part[kWaves];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 7, lc = lane >> 3;

    // Workgroups of one staged cloud hold consecutive logical ids: one XCD, one L2 (a pure speed choice).
    const int lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int cj = lid / a.groups;
    const int q_begin = (lid - cj * a.groups) * a.group;
    int q_end = min(q_begin + a.group, a.nq);
    if (a.self_mode == 1) {
        if (q_begin > cj) return;  // (whole workgroup) below the diagonal: mirrored from above it
        q_end = min(q_end, cj + 1);
    }
    const int pq = a.pq, pc = a.pc;
    const float *C = a.c + (size_t)cj * pc * 3;
    const float4 *X4 = reinterpret_cast<const float4 *>(lds_c);
    const float4 *Y4 = X4 + kCH / 4;
    const float4 *Z4 = Y4 + kCH / 4;

    int staged_c0 = -1;
    bool bad_c = false;  // this thread staged a NaN or infinite coordinate (v_min drops NaN: the cloud is flagged instead)

    for (int qi = q_begin; qi < q_end; qi++) {
        const int i = a.swap ? cj : qi, j = a.swap ? qi : cj;  // the entry: cloud i of a, cloud j of bank
        if (a.self_mode == 1 && qi == cj) {
            // a cloud against itself: every minimum is the distance of a point to itself
            bool bad = false;
            for (int e = tid; e < pc * 3; e += kT) bad |= non_finite(C[e]);
            const int any = __syncthreads_or(bad);
            if (tid == 0) {
                const float v = any ? __builtin_nanf("") : 0.f;
                if (a.d_ab) a.d_ab[(size_t)i * a.r + j] = v;
                if (a.d_ba) a.d_ba[(size_t)i * a.r + j] = v;
            }
            continue;
        }
        const float *Q = a.q + (size_t)qi * pq * 3;
        bool bad_q = false;
        float row_total = 0.f, col_total = 0.f;
        for (int q0 = 0; q0 < pq; q0 += kCH) {  // (COL: one block, the host's choice of the staged bank)
            const int qcnt = min(kCH, pq - q0);
            const int tiles = pcc::ceil_div(qcnt, kTQ);
            for (int e = tid; e < tiles * kTQ; e += kT) rowmin[e] = kInfBits;
            for (int c0 = 0; c0 < pc; c0 += kCH) {
                const int cnt = min(kCH, pc - c0);
                const int steps = pcc::ceil_div(cnt, kTC);
                __syncthreads();  // the previous chunk is consumed
                if (staged_c0 != c0) {
                    // AoS global -> SoA LDS; the last step is padded with +inf, which never is a row minimum
                    const float *src = C + (size_t)c0 * 3;
                    for (int e = tid; e < cnt * 3; e += kT) {
                        const float v = src[e];
                        bad_c |= non_finite(v);
                        const int p = e / 3;
                        lds_c[(e - p * 3) * kCH + p] = v;
                    }
                    for (int e = cnt + tid; e < steps * kTC; e += kT) {
                        lds_c[e] = __builtin_inff();
                        lds_c[kCH + e] = __builtin_inff();
                        lds_c[2 * kCH + e] = __builtin_inff();
                    }
                    staged_c0 = c0;
                }
                if (COL)
                    for (int e = tid; e < steps * kTC; e += kT) colmin[e] = kInfBits;
                __syncthreads();

                for (int tile = w; tile < tiles; tile += kWaves) {
                    float qx[kRQ], qy[kRQ], qz[kRQ], racc[kRQ];
#pragma unroll
                    for (int r = 0; r < kRQ; r++) {
                        // a point past the end repeats the last one: no minimum changes
                        const int p = q0 + min(tile * kTQ + r * 8 + lq, qcnt - 1);
                        qx[r] = Q[(size_t)p * 3 + 0];
                        qy[r] = Q[(size_t)p * 3 + 1];
                        qz[r] = Q[(size_t)p * 3 + 2];
                        bad_q |= non_finite(qx[r]) || non_finite(qy[r]) || non_finite(qz[r]);
                        racc[r] = __builtin_inff();
                    }
                    for (int s = 0; s < steps; s++) {
                        const float4 cx = X4[s * 8 + lc], cy = Y4[s * 8 + lc], cz = Z4[s * 8 + lc];
                        const f32x2 cxa = {cx.x, cx.y}, cxb = {cx.z, cx.w}, cya = {cy.x, cy.y}, cyb = {cy.z, cy.w};
                        const f32x2 cza = {cz.x, cz.y}, czb = {cz.z, cz.w};
                        float cm0 = __builtin_inff(), cm1 = cm0, cm2 = cm0, cm3 = cm0;
#pragma unroll
                        for (int r = 0; r < kRQ; r += 2) {
                            const f32x2 d0a = sq3x2(cxa - qx[r], cya - qy[r], cza - qz[r]);
                            const f32x2 d0b = sq3x2(cxb - qx[r], cyb - qy[r], czb - qz[r]);
                            const f32x2 d1a = sq3x2(cxa - qx[r + 1], cya - qy[r + 1], cza - qz[r + 1]);
                            const f32x2 d1b = sq3x2(cxb - qx[r + 1], cyb - qy[r + 1], czb - qz[r + 1]);
                            racc[r] = __builtin_fminf(__builtin_fminf(racc[r], d0a.x), d0a.y);
                            racc[r] = __builtin_fminf(__builtin_fminf(racc[r], d0b.x), d0b.y);
                            racc[r + 1] = __builtin_fminf(__builtin_fminf(racc[r + 1], d1a.x), d1a.y);
                            racc[r + 1] = __builtin_fminf(__builtin_fminf(racc[r + 1], d1b.x), d1b.y);
                            if (COL) {
                                cm0 = __builtin_fminf(__builtin_fminf(cm0, d0a.x), d1a.x);
                                cm1 = __builtin_fminf(__builtin_fminf(cm1, d0a.y), d1a.y);
                                cm2 = __builtin_fminf(__builtin_fminf(cm2, d0b.x), d1b.x);
                                cm3 = __builtin_fminf(__builtin_fminf(cm3, d0b.y), d1b.y);
                            }
                        }
                        if (COL) {
                            // lane lq < 4 folds staged point lc * 4 + lq of the step into the chunk's column minima
                            const unsigned u0 = min_over_lq(cm0), u1 = min_over_lq(cm1), u2 = min_over_lq(cm2), u3 = min_over_lq(cm3);
                            const unsigned mine = lq == 0 ? u0 : lq == 1 ? u1 : lq == 2 ? u2 : u3;
                            if (lq < kRC) atomicMin(&colmin[s * kTC + lc * kRC + lq], mine);
                        }
                    }
                    // row minima over the 8 lc lanes (lane bits 3-5); this wave alone owns the tile's slots
#pragma unroll
                    for (int r = 0; r < kRQ; r++) {
                        float v = racc[r];
                        v = __builtin_fminf(v, __shfl_xor(v, 8));
                        v = __builtin_fminf(v, __shfl_xor(v, 16));
                        v = __builtin_fminf(v, __shfl_xor(v, 32));
                        if (lc == 0) {
                            unsigned *slot = &rowmin[tile * kTQ + r * 8 + lq];
                            *slot = min(*slot, __builtin_bit_cast(unsigned, v));
                        }
                    }
                }
                __syncthreads();
                if (COL) col_total += block_sum(colmin, cnt, part);
            }
            row_total += block_sum(rowmin, qcnt, part);
        }
        const int bad = __syncthreads_or(bad_c | bad_q);
        if (tid == 0) {
            float row = a.mean ? row_total / (float)pq : row_total;
            float col = a.mean ? col_total / (float)pc : col_total;
            if (bad) row = col = __builtin_nanf("");
            float *row_out = a.swap ? a.d_ba : a.d_ab;  // the streamed cloud's points against the staged cloud
            float *col_out = a.swap ? a.d_ab : a.d_ba;
            if (row_out) row_out[(size_t)i * a.r + j] = row;
            if (COL && col_out) col_out[(size_t)i * a.r + j] = col;
            if (a.self_mode) {  // one bank: d_ba[j,i] = d_ab[i,j] (never swapped)
                if (a.d_ba) a.d_ba[(size_t)j * a.r + i] = row;
                if (COL && a.d_ab) a.d_ab[(size_t)j * a.r + i] = col;
            }
        }
    }
}

template <bool COL>
int launch_matrix(MatrixArgs a, hipStream_t st) {
    // Streamed clouds per workgroup: the staged cloud is reused `group` times; about 2048 workgroups keep 256 CUs level.
    const long long pairs = (long long)a.nq * a.nc;
    a.group = (int)std::min<long long>(std::min<long long>(16, a.nq), std::max<long long>(1, pairs / 2048));
    a.groups = pcc::ceil_div(a.nq, a.group);
    const long long grid = (long long)a.nc * a.groups;
    if (grid > 0x7fffffffLL) return pcc::invalid("chamfer_matrix: grid too large");
    {
        pcc::ProfScope prof(COL ? "chamfer_matrix_kernel<both>" : "chamfer_matrix_kernel<rows>", st);
        hipLaunchKernelGGL((chamfer_matrix_kernel<COL>), dim3((unsigned)grid), dim3(kT), 0, st, a);
    }
    return pcc::check_launch("chamfer_matrix");
}

}  // namespace

extern "C" {

int pcc_chamfer_matrix(int s, int n, const float *a, int r, int m, const float *bank, int mean, float *d_ab,
                       float *d_ba, pcc_stream_t stream) {
    pcc::clear_error();
    if (s < 0 || r < 0 || n < 0 || m < 0) return pcc::invalid("chamfer_matrix: negative size");
    if (s == 0 || r == 0) return PCC_OK;
    if (n == 0 || m == 0) return pcc::invalid("chamfer_matrix: a cloud is empty");
    if (n > (1 << 30) || m > (1 << 30)) return pcc::invalid("chamfer_matrix: bad size");
    if (!a || !bank) return pcc::invalid("chamfer_matrix: null pointer");
    if (!d_ab && !d_ba) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);

    MatrixArgs g{};
    g.mean = mean != 0;
    g.r = r;
    g.d_ab = d_ab;
    g.d_ba = d_ba;
    const auto stream_a = [&] { g.q = a; g.nq = s; g.pq = n; g.c = bank; g.nc = r; g.pc = m; g.swap = 0; };
    const auto stream_bank = [&] { g.q = bank; g.nq = r; g.pq = m; g.c = a; g.nc = s; g.pc = n; g.swap = 1; };

    if (a == bank && s == r && n == m) {  // one bank against itself
        stream_a();
        if (n <= kCH) {
            g.self_mode = 1;
            return launch_matrix<true>(g, st);
        }
        g.self_mode = 2;
        return launch_matrix<false>(g, st);
    }
    if (d_ab && d_ba) {
        if (n <= kCH) {
            stream_a();
            return launch_matrix<true>(g, st);
        }
        if (m <= kCH) {
            stream_bank();
            return launch_matrix<true>(g, st);
        }
        stream_a();
        if (int rc = launch_matrix<false>(g, st)) return rc;
        stream_bank();
        return launch_matrix<false>(g, st);
    }
    if (d_ab) stream_a();
    else stream_bank();
    return launch_matrix<false>(g, st);
}

}  // extern "C"
