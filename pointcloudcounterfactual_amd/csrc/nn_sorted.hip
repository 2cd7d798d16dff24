// ---------------------------------------------------------------------------------------------------
// Nearest neighbours on the sorted clouds (the Chamfer half of the reference's ChamferEMD loss, nndistance.cu:2-128, when
// it is computed in the same call as the approximate EMD: pcc_chamfer_emd).  The exhaustive scan of nn_fwd_kernel
// evaluates every pair; here the Hilbert-sorted points, the 16-point boxes and the permutations of THIS call's sort are
// reused, and a group of 16 consecutive sorted queries only visits the candidate blocks that can still hold a nearest
// neighbour:
//   1. the candidate blocks of a window are ordered by the distance between their box and the group's box (a lower
//      bound of every distance between the two boxes) and visited nearest first;
//   2. the group's radius is the largest of its queries' best distances so far; the first block whose box is farther
//      than the radius ends the walk (everything behind it is farther still): exact, nothing that could win -- or tie
//      with a lower index -- is skipped.  On the bench clouds a group visits 11 of 128 blocks on average (43 at most);
//   3. ties go to the lowest ORIGINAL candidate index (the reference's rule; the sorted order is not the original one):
//      the best so far is one 64-bit key (distance bits : original index).  Distances are the oracle's fmaf chain:
//      indices and distances carry the bits of nn_fwd_kernel / the oracle (tests/test_gpu_structural.py).
// Measured: 42 us per half-batch launch at B=32, N=2048 -- on a par with the exhaustive kernel (the 16 x 16 tile steps cost
// ~100 instructions each, 4x the exhaustive kernel's cost per pair, on 9 % of the pairs); what the fused call saves is
// the separate loss-reduction launch (it rides in the finish launch) and the second read of the clouds.
// ---------------------------------------------------------------------------------------------------
#include "approxmatch.hpp"
#include "wave_ops.hpp"
#include "wave_sort.hpp"

namespace {

using pcc::sq3;

struct NNSortedArgs {
    int n_q, n_c, q_n4, c_n4, q_nb, c_nb, groups, batch;
    const float *q_soa;            // [b][3][n4]
    const float4 *c_aos;           // [b][n_c] (x, y, z, original index) per sorted candidate
    const float *q_box, *c_box;    // [b][nb][8]
    const int *q_perm;             // [b][n] sorted position -> original index
    float *out_d;                  // [b][n_q] in the caller's query order
    int *out_i;
};

// A WAVE owns one group of 16 consecutive sorted queries and works alone (no LDS, no barrier: thousands of independent
// waves hide each other's latency): lane = (candidate slot cl of a 16-candidate block, query quad), four queries in
// registers.  128 candidate blocks per window: every lane tests two of them against the group's box, the survivors are
// two 64-bit ballots that the wave walks bit by bit; a lane loads ITS candidate of the block straight from the sorted
// rows (L2-resident), the next block's loads are issued before the current one is consumed.
constexpr int kNNWaves = 4;  // independent waves per workgroup
constexpr int kNNQ = 4;      // queries per lane

__global__ __launch_bounds__(64 * kNNWaves) void nn_sorted_kernel(NNSortedArgs a0, NNSortedArgs a1, int waves0) {
    const int lane = threadIdx.x & 63;
    int gw = (int)blockIdx.x * kNNWaves + (int)(threadIdx.x >> 6);   // global wave = (direction, sample, group)
    const bool second = gw >= waves0;
    const NNSortedArgs &a = second ? a1 : a0;
    if (second) gw -= waves0;
    const int smp = gw / a.groups;
    const int grp = gw - smp * a.groups;
    if (smp >= a.batch) return;  // (whole wave)
    const int cl = lane & (kBox - 1), quad = lane / kBox;
    const float *Q = a.q_soa + (size_t)smp * 3 * a.q_n4;
    const float4 *C = a.c_aos + (size_t)smp * a.n_c;

    // best so far per query as ONE 64-bit key (distance bits : original candidate index): squared distances are
    // non-negative floats, which order like unsigned integers, so a single 64-bit compare is the reference's rule
    // "smaller distance, lowest index on ties"
    float qx[kNNQ], qy[kNNQ], qz[kNNQ];
    unsigned long long bk[kNNQ];
#pragma unroll
    for (int j = 0; j < kNNQ; j++) {
        int q = grp * kBox + quad * kNNQ + j;
        q = q < a.n_q ? q : a.n_q - 1;
        qx[j] = Q[q];
        qy[j] = Q[a.q_n4 + q];
        qz[j] = Q[2 * a.q_n4 + q];
        bk[j] = pcc::kKeyInf;
    }
    const float4 *gb = reinterpret_cast<const float4 *>(a.q_box + ((size_t)smp * a.q_nb + grp) * 8);
    const float4 glo = gb[0], ghi = gb[1];

    struct Cand {
        float x, y, z;
        int o;
    };
    auto load_block = [&](int blk) -> Cand {  // this lane's candidate of block `blk` (+inf / INT_MAX beyond the cloud)
        // unconditional loads of a clamped index (a branch around them would serialise the software pipeline below),
        // then the select
        const int ci = blk * kBox + cl;
        const bool real = ci < a.n_c;
        const unsigned cc = (unsigned)(real ? ci : a.n_c - 1);
        const float4 v = C[cc];  // one 16-byte load per lane and block
        Cand c;
        c.x = real ? v.x : __builtin_inff();
        c.y = v.y;
        c.z = v.z;
        c.o = real ? __float_as_int(v.w) : 0x7fffffff;
        return c;
    };
    auto scan = [&](const Cand &c) {
#pragma unroll
        for (int j = 0; j < kNNQ; j++) {
            const float d = sq3(c.x - qx[j], c.y - qy[j], c.z - qz[j]);
            const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)c.o;
            bk[j] = k < bk[j] ? k : bk[j];
        }
    };
    // the group's radius: every query's best so far over its 16 candidate lanes, the largest over the 16 queries
    auto group_radius = [&]() -> float {
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < kNNQ; j++) {
            const float m = pcc::row_reduce16(__uint_as_float((unsigned)(bk[j] >> 32)), [](float a, float b) { return fminf(a, b); });
            r = fmaxf(r, grp * kBox + quad * kNNQ + j < a.n_q ? m : 0.f);
        }
        // the four rows (query quads) meet through scalar reads
        const int ri = __float_as_int(r);
        const float r0 = __int_as_float(__builtin_amdgcn_readlane(ri, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(ri, 16));
        const float r2 = __int_as_float(__builtin_amdgcn_readlane(ri, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(ri, 48));
        return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
    };

    float r = __builtin_inff();  // the group's radius: the largest of its queries' best distances so far
    for (int b0 = 0; b0 < a.c_nb; b0 += 128) {  // windows of 128 candidate blocks (2048 candidates)
        // every lane: two blocks of the window, keyed by the lower bound of every distance between the group's box and
        // the block's box (the candidates' own chain); nearest boxes first
        unsigned key[2];
        pcc::sort_box_window(key, a.c_box, smp, a.c_nb, b0, glo, ghi, lane, sq3);
        // walk the window nearest-first; a block farther than the radius ends it (everything behind is farther still):
        // nothing that could win, or tie with a lower original index, is skipped.  Two blocks are in flight ahead.
        // (branch-free: a branch around the look-ahead loads makes the compiler drain them before every use)
        const int nwin = min(128, a.c_nb - b0);
        // batches of four blocks: their sixteen loads are issued together, each block is consumed as soon as ITS loads
        // have landed (straight-line code: the compiler counts the outstanding loads exactly), the radius is refreshed
        // after every batch
        bool done = false;
        for (int p = 0; p < nwin && !done; p += 4) {
            unsigned kk[4];
            Cand cc[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                kk[u] = pcc::window_key(key, min(p + u, nwin - 1));  // (past the end: the last block again, never consumed)
                cc[u] = load_block(b0 + (int)(kk[u] & 127u));
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (!done) {
                    if (p + u >= nwin || __uint_as_float(kk[u] & ~127u) > r) done = true;
                    else scan(cc[u]);
                }
            }
            r = fminf(r, group_radius());
        }
    }
    // every query: best over its 16 candidate lanes
#pragma unroll
    for (int j = 0; j < kNNQ; j++) {
#pragma unroll
        for (int off = 1; off < kBox; off <<= 1) {
            const unsigned long long ok = pcc::shfl_xor_u64(bk[j], off);
            bk[j] = ok < bk[j] ? ok : bk[j];
        }
    }
    if (cl == 0) {
#pragma unroll
        for (int j = 0; j < kNNQ; j++) {
            const int qs = grp * kBox + quad * kNNQ + j;
            if (qs < a.n_q) {
                const int orig = a.q_perm[(size_t)smp * a.n_q + qs];
                // A key that still holds kKeyInf's index found no candidate: every distance of the query was NaN (its
                // bits sort above +inf).  It gets what the reference and pcc_nndistance give a NaN query, NaN / index 0:
                // no index outside the other cloud is ever written (the backward gathers through these indices).
                const bool found = (unsigned)(bk[j] & 0xffffffffu) != 0x7fffffffu;
                a.out_d[(size_t)smp * a.n_q + orig] = __uint_as_float(found ? (unsigned)(bk[j] >> 32) : 0x7fc00000u);
                a.out_i[(size_t)smp * a.n_q + orig] = found ? (int)(bk[j] & 0xffffffffu) : 0;
            }
        }
    }
}

}  // namespace

namespace pcc {

// The Chamfer half of a ChamferEMD call for the samples [s0, s0 + bc) (`v`: the workspace view at s0): nearest neighbours
// on the clouds this call has just sorted, both directions in one launch.
int launch_nn_sorted(const AmDims &L, const WsView &v, int s0, int bc, const ChamferOut *chamfer, hipStream_t lst) {
    const size_t o = (size_t)s0;
    const int n = L.n, m = L.m;
    NNSortedArgs q1{}, q2{};
    q1.n_q = n; q1.n_c = m; q1.q_n4 = L.n4; q1.c_n4 = L.m4; q1.q_nb = L.nb1; q1.c_nb = L.nb2;
    q1.groups = L.nb1; q1.batch = bc;
    q1.q_soa = v.soa1; q1.c_aos = v.aos2; q1.q_box = v.box1; q1.c_box = v.box2; q1.q_perm = v.perm1;
    q1.out_d = chamfer->dist1 + o * n; q1.out_i = chamfer->idx1 + o * n;
    q2.n_q = m; q2.n_c = n; q2.q_n4 = L.m4; q2.c_n4 = L.n4; q2.q_nb = L.nb2; q2.c_nb = L.nb1;
    q2.groups = L.nb2; q2.batch = bc;
    q2.q_soa = v.soa2; q2.c_aos = v.aos1; q2.q_box = v.box2; q2.c_box = v.box1; q2.q_perm = v.perm2;
    q2.out_d = chamfer->dist2 + o * m; q2.out_i = chamfer->idx2 + o * m;
    const long long w0 = (long long)bc * q1.groups, w1 = (long long)bc * q2.groups;
    const long long grid = (w0 + w1 + kNNWaves - 1) / kNNWaves;
    if (w0 + w1 > 0x7fffffffLL) return pcc::invalid("chamfer_emd: grid too large");
    {
        pcc::ProfScope prof("nn_sorted_kernel", lst);
        hipLaunchKernelGGL(nn_sorted_kernel, dim3((unsigned)grid), dim3(64 * kNNWaves), 0, lst, q1, q2, (int)w0);
    }
    return pcc::check_launch("chamfer_emd(nearest neighbours)");  // (the loss reduction rides in the finish launch)
}
}  // namespace pcc
