// Auction EMD for gfx950 (MI355X), wave64.
//
// Replaces external/emd/src/emd_cuda.cu (7 kernels x iters launches, all state in global memory, racy GetMax /
// Assign).  One persistent 1024-thread workgroup per sample runs every iteration with the auction state in
// LDS (targets SoA and prices; for n <= 4095, where 40 n + 16 bytes fit the 160 KiB, also the max increments and
// the bidder-side arrays -- from n = 4096 on those six arrays live in global scratch, which leaves 16 n + 16
// bytes of LDS and lets n = 8192 launch): phases are separated by workgroup barriers instead of kernel
// boundaries, compaction/winner selection use integer atomics, and every tie is resolved deterministically
// (lowest bidder index), so two runs agree bit for bit.
// A bidder that no target gives a value above the scan's floor of -1e9 (its own coordinates are NaN or
// infinite, or every target is non-finite or ~1e9 away) makes NO BID in that iteration: best_i stays -1, it
// writes bid -1 and nothing else, GetMax and Assign skip it (the forced last iteration too) and it ends with
// assignment -1 and dist NaN.  A non-finite target needs no rule: its value is NaN or -inf, which wins neither
// `d > best` nor `d > better`, so nobody ever bids on it.
// Bid values follow emd_cuda.cu:145 literally: `3.0 - sqrtf(d2) - price` is DOUBLE arithmetic rounded once
// to float; sqrtf is correctly rounded (-fno-fast-math).
#include "pcc_common.hpp"
#include "pcc_emd.h"
#include "pcc_test_hooks.h"

#include <algorithm>

namespace {

using pcc::sq3;

struct Cand {
    float best, better;
    int best_i;
};

// first-maximum rule (emd_cuda.cu:146-153 / :166-171) as an order-independent merge
__device__ __forceinline__ Cand merge(const Cand &a, const Cand &b) {
    Cand r;
    const bool take_b = (b.best > a.best) || (b.best == a.best && (unsigned)b.best_i < (unsigned)a.best_i);
    r.best = take_b ? b.best : a.best;
    r.best_i = take_b ? b.best_i : a.best_i;
    const float loser = take_b ? a.best : b.best;
    r.better = fmaxf(loser, fmaxf(a.better, b.better));
    return r;
}

__global__ __launch_bounds__(1024) void auction_kernel(int n, const float *__restrict__ xyz1,
                                                        const float *__restrict__ xyz2, float eps, int iters,
                                                        float *__restrict__ dist, int *__restrict__ assignment,
                                                        int *__restrict__ scratch, int state_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *sx = reinterpret_cast<float *>(smem);
    float *sy = sx + n, *sz = sy + n, *price = sz + n;
    int *hot_end = reinterpret_cast<int *>(price + n);
    int *cnt = state_in_lds ? hot_end + n : hot_end;  // [4]
    int *st = state_in_lds ? cnt + 4 : scratch + (size_t)blockIdx.x * 6 * n;
    int *unass = st, *inv = st + n, *bid = st + 2 * n, *win = st + 3 * n;
    float *inc = reinterpret_cast<float *>(st + 4 * n);
    int *max_inc = state_in_lds ? hot_end : st + 5 * n;  // float bits; values written are >= 0 or -1e9

    const int tid = threadIdx.x, T = 1024;
    const int smp = blockIdx.x;
    const float *p1 = xyz1 + (size_t)smp * n * 3, *p2 = xyz2 + (size_t)smp * n * 3;
    int *ass = assignment + (size_t)smp * n;

    for (int k = tid; k < n; k += T) {
        sx[k] = p2[k * 3 + 0];
        sy[k] = p2[k * 3 + 1];
        sz[k] = p2[k * 3 + 2];
        price[k] = 0.f;
        max_inc[k] = 0;  // emd_module.py:41 zeros
        ass[k] = -1;
        inv[k] = -1;
        bid[k] = 0;
        inc[k] = 0.f;
    }
    __syncthreads();

    for (int it = 0; it < iters; it++) {
        const bool last = it == iters - 1;
        if (tid == 0) cnt[0] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += T)
            if (ass[j] == -1) unass[atomicAdd(&cnt[0], 1)] = j;  // order irrelevant to the result
        __syncthreads();
        const int nu = cnt[0];
        if (nu == 0) break;  // everything assigned: the remaining iterations (and the forced one) are no-ops
        // ---- Bid (emd_cuda.cu:94-178): TPB lanes share one bidder and split the targets ----
        int tpb = 1;
        while (tpb < 64 && tpb * 2 * nu <= T) tpb *= 2;
        const int per_round = T / tpb;
        const int sub = tid & (tpb - 1);
        for (int u0 = 0; u0 < nu; u0 += per_round) {
            const int u = u0 + tid / tpb;
            const bool live = u < nu;
            const int j = live ? unass[u] : unass[0];
            const float x1 = p1[j * 3 + 0], y1 = p1[j * 3 + 1], z1 = p1[j * 3 + 2];
            Cand c{-1e9f, -1e9f, -1};
            for (int k = sub; k < n; k += tpb) {
                const float s = __builtin_sqrtf(sq3(sx[k] - x1, sy[k] - y1, sz[k] - z1));
                const float d = (float)(3.0 - (double)s - (double)price[k]);
                if (d > c.best) {
                    c.better = c.best;
                    c.best = d;
                    c.best_i = k;
                } else if (d > c.better) {
                    c.better = d;
                }
            }
            for (int off = 1; off < tpb; off <<= 1) {
                Cand o;
                o.best = __shfl_xor(c.best, off, 64);
                o.better = __shfl_xor(c.better, off, 64);
                o.best_i = __shfl_xor(c.best_i, off, 64);
                c = merge(c, o);
            }
            if (live && sub == 0) {
                bid[j] = c.best_i;  // -1: no bid in this iteration
                if (c.best_i >= 0) {
                    const float bi = c.best - c.better + eps;  // :174
                    inc[j] = bi;
                    atomicMax(&max_inc[c.best_i], __float_as_int(bi));  // :175 (bi >= 0: int order == float order)
                    win[c.best_i] = 0x7fffffff;
                }
            }
        }
        __syncthreads();
        // ---- GetMax (:180-193): lowest qualifying bidder wins ----
        for (int u = tid; u < nu; u += T) {
            const int j = unass[u], t = bid[j];
            if (t < 0) continue;
            const double bi = inc[j], mi = __int_as_float(max_inc[t]);
            if (bi - 1e-6 <= mi && mi <= bi + 1e-6) atomicMin(&win[t], j);
        }
        __syncthreads();
        // ---- Assign (:195-214) ----
        for (int u = tid; u < nu; u += T) {
            const int j = unass[u], t = bid[j];
            if (t < 0) continue;
            if (last || win[t] == j) {
                const int owner = inv[t];
                if (!last && owner != -1) ass[owner] = -1;
                inv[t] = j;
                ass[j] = t;
                if (last) atomicAdd(&price[t], inc[j]);
                else price[t] += inc[j];
                max_inc[t] = __float_as_int(-1e9f);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int j = tid; j < n; j += T) {  // CalcDist :216-225
        const int k = ass[j];
        const bool valid = k >= 0 && k < n;  // -1: a bidder that never had a bid
        const int kk = valid ? k : 0;
        const float d = sq3(p1[j * 3 + 0] - sx[kk], p1[j * 3 + 1] - sy[kk], p1[j * 3 + 2] - sz[kk]);
        dist[(size_t)smp * n + j] = valid ? d : __builtin_nanf("");
    }
}

// ---------------------------------------------------------------------------------------------------
// Cluster schedule: C workgroups per sample instead of one (B=32 samples on one workgroup each use 32 of 256 CUs).
// A workgroup owns a contiguous slice of the BIDDERS (set1 points) and keeps the whole target cloud plus a copy of
// the prices in LDS; the state the workgroups of a sample share -- prices, assignment, inverse assignment, highest
// increment and winner per target -- lives in global memory and is touched only with agent-scope (sc1) accesses /
// atomics (the rule of pcc::coresident_barrier, pcc_common.hpp).  Three sample-local barriers per
// iteration replace the kernel boundaries of the reference (Bid | GetMax | Assign).  Same deterministic rules as the
// one-workgroup kernel, hence the same bits: the best / second-best scan of a bidder does not depend on who runs
// it, atomicMax / atomicMin are order-free, and every target has at most one winner per iteration.
// All workgroups of a launch must be co-resident (the host sizes C and the launch for that, behind a
// pcc::CoresidentGate); spins are bounded and raise an error word that poisons the outputs instead of hanging.
// ---------------------------------------------------------------------------------------------------
using pcc::agent_ld, pcc::agent_st;

__global__ __launch_bounds__(1024) void auction_cluster_kernel(int n, int C, const float *__restrict__ xyz1,
                                                                const float *__restrict__ xyz2, float eps, int iters,
                                                                float *__restrict__ dist, int *__restrict__ assignment,
                                                                int *__restrict__ scratch, unsigned *__restrict__ sync,
                                                                int smp0, unsigned *__restrict__ host_err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, T = 1024;
    // the C workgroups of a sample exchange prices, bids and barrier arrivals through the L2: give them block ids of one
    // XCD (pcc::xcd_contiguous; a speed choice only -- every shared word is an agent-scope access)
    const int lid = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int smp = smp0 + lid / C, c = lid % C;
    const int j0 = (int)((long long)n * c / C), j1 = (int)((long long)n * (c + 1) / C);
    const int njmax = (n + C - 1) / C + 1;
    float *sx = reinterpret_cast<float *>(smem);
    float *sy = sx + n, *sz = sy + n, *pr = sz + n;       // targets + this iteration's prices
    int *unass = reinterpret_cast<int *>(pr + n);          // [njmax] own unassigned bidders
    int *bidl = unass + njmax;                             // [njmax] their targets   (indexed like unass)
    float *incl = reinterpret_cast<float *>(bidl + njmax);  // [njmax] their increments
    int *cnt = reinterpret_cast<int *>(incl + njmax);      // [4]

    const float *p1 = xyz1 + (size_t)smp * n * 3, *p2 = xyz2 + (size_t)smp * n * 3;
    int *ass = assignment + (size_t)smp * n;
    int *sc = scratch + (size_t)smp * 4 * n;
    float *price = reinterpret_cast<float *>(sc);
    int *inv = sc + n, *max_inc = sc + 2 * n, *win = sc + 3 * n;
    unsigned *err = sync;                                  // one error word, then the per-sample records:
    unsigned *sy_ctr = sync + 1 + (size_t)smp * (2 + iters);  // [0] barrier counter, [1] unused, [2 + it] bidders of iteration it
    unsigned barriers = 0;
    auto barrier = [&] {  // the error word is launch-wide; the sticky host word is raised once, at the end of the kernel
        return pcc::coresident_barrier<2, (1u << 24)>(sy_ctr, C * ++barriers, err, nullptr, [] { return 1u; });
    };

    for (int k = tid; k < n; k += T) {
        sx[k] = p2[k * 3 + 0];
        sy[k] = p2[k * 3 + 1];
        sz[k] = p2[k * 3 + 2];
    }
    for (int k = j0 + tid; k < j1; k += T) {  // this workgroup initialises its share of the shared state
        agent_st(&price[k], 0.f);
        agent_st(&inv[k], -1);
        agent_st(&max_inc[k], 0);  // emd_module.py:41 zeros
        agent_st(&ass[k], -1);
    }
    bool ok = barrier();

    for (int it = 0; ok && it < iters; it++) {
        const bool last = it == iters - 1;
        if (tid == 0) cnt[0] = 0;
        for (int k = tid; k < n; k += T) pr[k] = agent_ld(&price[k]);
        __syncthreads();
        for (int j = j0 + tid; j < j1; j += T)
            if (agent_ld(&ass[j]) == -1) unass[atomicAdd(&cnt[0], 1)] = j;  // order irrelevant to the result
        __syncthreads();
        const int nu = cnt[0];
        if (tid == 0 && nu) __hip_atomic_fetch_add(&sy_ctr[2 + it], (unsigned)nu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ---- Bid (emd_cuda.cu:94-178): TPB lanes share one bidder and split the targets ----
        int tpb = 1;
        while (tpb < 64 && tpb * 2 * nu <= T) tpb *= 2;
        const int per_round = T / tpb;
        const int sub = tid & (tpb - 1);
        for (int u0 = 0; u0 < nu; u0 += per_round) {
            const int u = u0 + tid / tpb;
            const bool live = u < nu;
            const int j = live ? unass[u] : unass[0];
            const float x1 = p1[j * 3 + 0], y1 = p1[j * 3 + 1], z1 = p1[j * 3 + 2];
            Cand cd{-1e9f, -1e9f, -1};
            for (int k = sub; k < n; k += tpb) {
                const float s = __builtin_sqrtf(sq3(sx[k] - x1, sy[k] - y1, sz[k] - z1));
                const float d = (float)(3.0 - (double)s - (double)pr[k]);
                if (d > cd.best) {
                    cd.better = cd.best;
                    cd.best = d;
                    cd.best_i = k;
                } else if (d > cd.better) {
                    cd.better = d;
                }
            }
            for (int off = 1; off < tpb; off <<= 1) {
                Cand o;
                o.best = __shfl_xor(cd.best, off, 64);
                o.better = __shfl_xor(cd.better, off, 64);
                o.best_i = __shfl_xor(cd.best_i, off, 64);
                cd = merge(cd, o);
            }
            if (live && sub == 0) {
                bidl[u] = cd.best_i;  // -1: no bid in this iteration
                if (cd.best_i >= 0) {
                    const float bi = cd.best - cd.better + eps;  // :174
                    incl[u] = bi;
                    // :175 (bi >= 0: int order == float order)
                    __hip_atomic_fetch_max(&max_inc[cd.best_i], __float_as_int(bi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    agent_st(&win[cd.best_i], 0x7fffffff);
                }
            }
        }
        ok = barrier();
        if (!ok) break;
        // everything assigned: the remaining iterations (and the forced one) are no-ops; every workgroup of the
        // sample reads the same total, so the exit is uniform
        if (agent_ld(&sy_ctr[2 + it]) == 0) break;
        // ---- GetMax (:180-193): lowest qualifying bidder wins ----
        for (int u = tid; u < nu; u += T) {
            const int j = unass[u], t = bidl[u];
            if (t < 0) continue;
            const double bi = incl[u], mi = __int_as_float(agent_ld(&max_inc[t]));
            if (bi - 1e-6 <= mi && mi <= bi + 1e-6) __hip_atomic_fetch_min(&win[t], j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        ok = barrier();
        if (!ok) break;
        // ---- Assign (:195-214) ----
        for (int u = tid; u < nu; u += T) {
            const int j = unass[u], t = bidl[u];
            if (t < 0) continue;
            if (last || agent_ld(&win[t]) == j) {
                const int owner = agent_ld(&inv[t]);
                if (!last && owner != -1) agent_st(&ass[owner], -1);
                agent_st(&inv[t], j);
                agent_st(&ass[j], t);
                if (last) __hip_atomic_fetch_add(&price[t], incl[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else agent_st(&price[t], pr[t] + incl[u]);  // the only writer of price[t] in this iteration
                agent_st(&max_inc[t], __float_as_int(-1e9f));
            }
        }
        ok = barrier();
    }
    __syncthreads();
    const bool bad = agent_ld(err) != 0;
    // the failure also goes to a sticky word in host memory: the next pcc_auction_* call on this device reports it
    if (bad && tid == 0 && host_err) __hip_atomic_store(host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int j = j0 + tid; j < j1; j += T) {  // CalcDist :216-225
        const int k = agent_ld(&ass[j]);
        const bool valid = !bad && k >= 0 && k < n;
        const int kk = valid ? k : 0;
        const float d = sq3(p1[j * 3 + 0] - sx[kk], p1[j * 3 + 1] - sy[kk], p1[j * 3 + 2] - sz[kk]);
        dist[(size_t)smp * n + j] = valid ? d : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(256) void auction_bwd_kernel(size_t total, int n, const float *__restrict__ xyz1,
                                                           const float *__restrict__ xyz2,
                                                           const float *__restrict__ grad_dist,
                                                           const int *__restrict__ idx, float *__restrict__ grad1) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const size_t smp = t / n;
    const int j2 = idx[t];
    // an assignment outside [0, n) (a point a failed forward left unassigned, -1) has no partner: zero gradient,
    // never an out-of-range read
    const bool valid = (unsigned)j2 < (unsigned)n;
    const float g = valid ? grad_dist[t] * 2 : 0.f;
    const size_t q = smp * n + (valid ? j2 : 0);
#pragma unroll
    for (int c = 0; c < 3; c++) grad1[t * 3 + c] = valid ? g * (xyz1[t * 3 + c] - xyz2[q * 3 + c]) : 0.f;
}

}  // namespace

extern "C" {

int pcc_auction_forward(int b, int n, const float *xyz1, const float *xyz2, float eps, int iters, float *dist,
                        int *assignment, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 1 || iters < 1) return pcc::invalid("auction: bad size (n >= 1, iters >= 1)");
    if (n > 8192) return pcc::invalid("auction: n > 8192 does not fit the LDS-resident state");
    // the highest increment per target is an integer atomicMax on the float's bits: right for increments >= 0 only
    if (!(eps >= 0.f)) return pcc::invalid("auction: eps must be >= 0 (and not NaN)");
    if (b == 0) return PCC_OK;
    if (!xyz1 || !xyz2 || !dist || !assignment) return pcc::invalid("auction: null pointer");
    if (pcc::take_coresident_failure(pcc::kAuctionCluster))
        return pcc::invalid("auction: an earlier launch on this device did not complete (a sample barrier timed out: its "
                            "outputs were poisoned with NaN / -1); this call was not started");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // ---- cluster schedule: C workgroups per sample when they can all be resident at once ----
    {
        // measurement switch (pcc_test_hooks.h): 1 forces one workgroup per sample, 2..16 forces C
        const int cl_override = pcc::tuning(PCC_TUNE_AUCTION_CLUSTER);
        const int cus = pcc::device_cus();
        int C = 1;
        if (cl_override != 1 && n >= 512 && cus > 0) {
            C = cl_override > 1 ? cl_override : 8;
            while (C > 1 && (n / C < 128)) C /= 2;          // a slice of at least 128 bidders
            while (C > 1 && C > cus) C /= 2;                 // one workgroup per CU: residency by construction
        }
        const int njmax = (n + C - 1) / C + 1;
        const size_t lds = (size_t)4 * n * 4 + (size_t)3 * njmax * 4 + 16;
        if (C > 1 && lds <= 160 * 1024 - 256) {
            pcc::CoresidentGate gate(pcc::kAuctionCluster, st);  // declines while capturing: auction_kernel below, same bits
            if (gate.ok) {
                // (the kernel also has a few bytes of static LDS: barrier flag)
                (void)pcc::allow_lds<auction_cluster_kernel>(160 * 1024 - 256);
                const int group = std::max(1, cus / C);          // samples per launch
                const size_t sync_words = 1 + (size_t)b * (2 + iters);
                const size_t bytes = (size_t)b * 4 * n * 4 + sync_words * 4;
                pcc::WsBlock ws(st);
                if (int rc = ws.alloc(bytes, "auction: workspace allocation failed")) return rc;
                int *scratch = static_cast<int *>(ws.p);
                unsigned *sync = reinterpret_cast<unsigned *>(static_cast<char *>(ws.p) + (size_t)b * 4 * n * 4);
                (void)hipMemsetAsync(sync, 0, sync_words * 4, st);
                if (gate.inject) (void)hipMemsetAsync(sync, 1, 1, st);  // test hook: start with the error word raised
                for (int s0 = 0; s0 < b; s0 += group) {
                    const int gb = std::min(group, b - s0);
                    pcc::ProfScope prof("auction_cluster_kernel", st);
                    hipLaunchKernelGGL(auction_cluster_kernel, dim3((unsigned)(gb * C)), dim3(1024), lds, st, n, C, xyz1, xyz2, eps,
                                       iters, dist, assignment, scratch, sync, s0, gate.sticky);
                }
                return pcc::check_launch("auction_forward(cluster)");
            }
        }
    }
    // targets, prices and the counters always; max increments + the five bidder-side arrays while all of it fits
    // (40 n + 16 <= 160 KiB: n <= 4095), in global scratch otherwise (16 n + 16 bytes of LDS: 128 KiB + 16 at n = 8192)
    const size_t hot = (size_t)4 * n * 4 + 16, state = (size_t)6 * n * 4;
    const int in_lds = hot + state <= 160 * 1024;
    const size_t lds = in_lds ? hot + state : hot;
    (void)pcc::allow_lds<auction_kernel>(160 * 1024);
    pcc::WsBlock scratch(st);
    if (!in_lds) {
        if (int rc = scratch.alloc((size_t)b * state, "auction: workspace allocation failed")) return rc;
    }
    {
        pcc::ProfScope prof("auction_kernel", st);
        hipLaunchKernelGGL(auction_kernel, dim3(b), dim3(1024), lds, st, n, xyz1, xyz2, eps, iters, dist, assignment,
                           static_cast<int *>(scratch.p), in_lds);
    }
    return pcc::check_launch("auction_forward");
}

int pcc_auction_status(void) {
    return pcc::take_coresident_failure(pcc::kAuctionCluster) ? 1 : 0;
}

int pcc_auction_backward(int b, int n, const float *xyz1, const float *xyz2, const float *grad_dist,
                         const int *assignment, float *grad_xyz1, pcc_stream_t stream) {
    pcc::clear_error();
    if (pcc::take_coresident_failure(pcc::kAuctionCluster))
        return pcc::invalid("auction_backward: the forward launch on this device did not complete (a sample barrier timed "
                            "out: dist was poisoned with NaN, unassigned points are -1)");
    if (b < 0 || n < 0) return pcc::invalid("auction_backward: bad size");
    if (b == 0 || n == 0) return PCC_OK;
    if (!xyz1 || !xyz2 || !grad_dist || !assignment || !grad_xyz1) return pcc::invalid("auction_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t total = (size_t)b * n;
    hipLaunchKernelGGL(auction_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, n, xyz1, xyz2,
                       grad_dist, assignment, grad_xyz1);
    return pcc::check_launch("auction_backward");
}

}  // extern "C"
