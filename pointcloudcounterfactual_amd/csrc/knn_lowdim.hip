// k-NN graph, c <= 3 and k <= 32, for gfx950 (MI355X), wave64: exact difference-form distances on the f32 VALU.
//   * knn_sorted_kernel (n <= 16384): search on the Hilbert-sorted cloud (see the kernel);
//   * knn_small_kernel (larger clouds): the same distances, exhaustive.
// The overview of the k-NN kernels is at the top of knn.hip.
#include "knn.hpp"
#include "pcc_neighbour.h"
#include "topk.hpp"
#include "wave_sort.hpp"

namespace {

constexpr int kCH = 2048;    // candidates staged per chunk (small-c kernel)

template <int K, int S>
struct SmallLayout {
    static constexpr int T = 64 * S;
    static constexpr int cand_bytes = 3 * kCH * 4;
    static constexpr int buf_bytes = 2 * kCap * T * 4;
    static constexpr int merge_bytes = 2 * S * K * 64 * 4;
    static constexpr int bytes = (cand_bytes + buf_bytes) > merge_bytes ? (cand_bytes + buf_bytes) : merge_bytes;
};

// Merge S sorted K-lists per lane (LDS layout [s][slot][lane]) and write the first k indices as int64.  Equal distances
// go to the lower candidate index: a wave's list is in (distance, index) order, but the waves' candidate ranges
// interleave (wave w takes the w-th quarter of EVERY 2048-candidate chunk), so from the second chunk on "the earlier
// wave" is not "the lower index".
// -> the slots that took a list entry; the others are padded with n - 1.
template <int K, int S>
__device__ __forceinline__ int merge_and_store(const float *md, const int *mi, int lane, int k, int64_t *dst, int n) {
    // heads as 64-bit keys (distance bits : index): the distances are non-negative and never NaN, so they order like
    // unsigned integers and one compare is "smaller distance, then lower index"; a list that has run out heads kKeyInf
    const auto entry = [&](int s, int pos) -> unsigned long long {
        return ((unsigned long long)__float_as_uint(md[(s * K + pos) * 64 + lane]) << 32) | (unsigned)mi[(s * K + pos) * 64 + lane];
    };
    int p[S];
    unsigned long long h[S];
    int filled = 0;
#pragma unroll
    for (int s = 0; s < S; s++) {
        p[s] = 0;
        h[s] = entry(s, 0);
    }
    for (int o = 0; o < k; o++) {
        int best = 0;
        unsigned long long bv = h[0];
#pragma unroll
        for (int s = 1; s < S; s++) {
            const bool lt = h[s] < bv;
            bv = lt ? h[s] : bv;
            best = lt ? s : best;
        }
        int pos = 0;
#pragma unroll
        for (int s = 0; s < S; s++) pos = (best == s) ? p[s] : pos;
        // (the lists run out when fewer than k distances are finite: never emit an index outside the cloud)
        dst[o] = (int64_t)min((int)(bv & 0xffffffffull), n - 1);
        filled += (unsigned)bv != 0x7fffffffu ? 1 : 0;
        const int np = pos + 1;
        const unsigned long long nh = np < K ? entry(best, np) : pcc::kKeyInf;
#pragma unroll
        for (int s = 0; s < S; s++) {
            const bool sel = best == s;
            p[s] = sel ? np : p[s];
            h[s] = sel ? nh : h[s];
        }
    }
    return filled;
}

template <int K, int S>
__global__ __launch_bounds__(64 * S) void knn_small_kernel(int c, int n, int k, const float *__restrict__ x,
                                                            int64_t *__restrict__ indices) {
    using L = SmallLayout<K, S>;
    constexpr int T = L::T;
    __shared__ __attribute__((aligned(16))) unsigned char smem[L::bytes];
    float *lds_c = reinterpret_cast<float *>(smem);
    float *buf_d = reinterpret_cast<float *>(smem + L::cand_bytes);
    int *buf_i = reinterpret_cast<int *>(smem + L::cand_bytes + kCap * T * 4);
    float *mrg_d = reinterpret_cast<float *>(smem);
    int *mrg_i = reinterpret_cast<int *>(smem + S * K * 64 * 4);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int smp = blockIdx.y;
    const float *xb = x + (size_t)smp * c * n;
    int q = blockIdx.x * 64 + lane;
    const bool q_ok = q < n;
    q = q_ok ? q : n - 1;
    const float qx = xb[q];
    const float qy = c > 1 ? xb[(size_t)n + q] : 0.f;
    const float qz = c > 2 ? xb[(size_t)2 * n + q] : 0.f;

    pcc::BufferedTopK<K, kCap, T> tk;
    tk.init(buf_d, buf_i, tid);

    const float4 *X4 = reinterpret_cast<const float4 *>(lds_c);
    const float4 *Y4 = X4 + kCH / 4;
    const float4 *Z4 = Y4 + kCH / 4;

    for (int c0 = 0; c0 < n; c0 += kCH) {
        const int cnt = min(kCH, n - c0);
        const int ngroups = (cnt + 7) / 8;
        if (c0) __syncthreads();
        for (int ch = 0; ch < 3; ch++) {
            for (int i = tid; i < ngroups * 8; i += T)
                lds_c[ch * kCH + i] = (i < cnt) ? (ch < c ? xb[(size_t)ch * n + c0 + i] : 0.f) : __builtin_inff();
        }
        __syncthreads();
        const int gs = (ngroups + S - 1) / S;
        const int g_begin = w * gs;
        const int g_end = min(g_begin + gs, ngroups);
        for (int g = g_begin; g < g_end; g++) {
            const float4 xa = X4[2 * g], xb4 = X4[2 * g + 1];
            const float4 ya = Y4[2 * g], yb4 = Y4[2 * g + 1];
            const float4 za = Z4[2 * g], zb4 = Z4[2 * g + 1];
            const float cx[8] = {xa.x, xa.y, xa.z, xa.w, xb4.x, xb4.y, xb4.z, xb4.w};
            const float cy[8] = {ya.x, ya.y, ya.z, ya.w, yb4.x, yb4.y, yb4.z, yb4.w};
            const float cz[8] = {za.x, za.y, za.z, za.w, zb4.x, zb4.y, zb4.z, zb4.w};
            if (tk.must_flush(8)) tk.flush();
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float dx = cx[j] - qx, dy = cy[j] - qy, dz = cz[j] - qz;
                // sum over channels in channel order: ((dx^2 + dy^2) + dz^2) as an fma chain
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                tk.offer(d, c0 + g * 8 + j);
            }
        }
    }
    tk.flush();
    __syncthreads();  // every wave is done with the candidate / FIFO regions: reuse them for the merge
#pragma unroll
    for (int s = 0; s < K; s++) {
        mrg_d[(w * K + s) * 64 + lane] = tk.top.d[s];
        mrg_i[(w * K + s) * 64 + lane] = tk.top.i[s];
    }
    __syncthreads();
    if (w == 0 && q_ok) {
        int64_t *dst = indices + ((size_t)smp * n + q) * k;
        const int filled = merge_and_store<K, S>(mrg_d, mrg_i, lane, k, dst, n);
        // the lists hold finite distances only: a short row continues with its +inf distances (see fill_inf_tail)
        if (filled < k)
            fill_inf_tail(
                filled, k, n,
                [&](int j) {
                    const float dx = xb[j] - qx, dy = (c > 1 ? xb[(size_t)n + j] : 0.f) - qy, dz = (c > 2 ? xb[(size_t)2 * n + j] : 0.f) - qz;
                    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                },
                [&](int slot, int j) { dst[slot] = (int64_t)j; });
    }
}

// ---------------------------------------------------------------------------------------------------
// c <= 3, n <= 16384: search on the Hilbert-sorted cloud.
// The exhaustive kernel above spends > 90 % of its time in the top-K insertion chains: candidates arrive in index
// order, so a lane's K-th distance keeps improving all through the scan (K(1 + ln(N/K)) insertions per list, four lists
// per query).  Here the cloud is first put in Hilbert order with one bounding box per 16 consecutive points (the sort
// kernel of the approximate EMD, cloud_sort.hip).  A WAVE owns one box of 16 consecutive sorted queries and works
// alone: lane = (query, candidate slice), the four slices of a query take four candidates each of every 16-candidate
// block and keep their own sorted K-list.
//   * the candidate blocks of a window are ordered by the distance between their box and the queries' box and visited
//     nearest first, so the lists fill with near points at once;
//   * a query's bound: if each of its four slice lists holds at least ceil(k/4) entries <= t, at least k candidates are
//     <= t, so its k-th distance is <= the largest of the four slices' ceil(k/4)-th entries.  Candidates beyond the bound
//     are not even buffered; the first block whose box is farther than the largest bound of the 16 queries ends the
//     walk (exact: nothing that could enter a list, or tie with a lower index, is skipped);
//   * list entries are 64-bit keys (distance bits : ORIGINAL index): squared distances are non-negative floats, which
//     order like unsigned integers, so one 64-bit compare is "ascending distance, ties ascending index" although
//     candidates no longer arrive in index order;
//   * the four slice lists of a query are merged at the end (LDS, one lane per query).
// ---------------------------------------------------------------------------------------------------
constexpr int kSW = 4;     // independent waves per workgroup (no barrier; the workgroup only shares the LDS allocation)
constexpr int kSQ = 16;    // queries per wave = one box of the sort
constexpr int kSlices = 4; // candidate slices per query
using pcc::kKeyInf;

// One step of the insertion chain: (slot, carry) <- (min, max) of the two 64-bit keys.  Keys are unique, so once the
// carry displaces an entry everything behind shifts.  One v_cmp_lt_u64 and four v_cndmask_b32 on ITS mask (written as
// asm: the compiler turns the two selects into separate unsigned min / max, i.e. two of the slow 64-bit compares).
__device__ __forceinline__ void ce_step(unsigned long long &slot, unsigned long long &carry) {
    const unsigned long long m = __ballot(carry < slot);
    const unsigned sl = (unsigned)slot, sh = (unsigned)(slot >> 32), cl = (unsigned)carry, ch = (unsigned)(carry >> 32);
    unsigned nsl, nsh, ncl, nch;
    // (s_nop: a VALU-written SGPR pair needs two wait states before a VALU reads it as a mask)
    asm("s_nop 1\n\tv_cndmask_b32_e64 %0, %4, %6, %8\n\tv_cndmask_b32_e64 %1, %5, %7, %8\n\t"
        "v_cndmask_b32_e64 %2, %6, %4, %8\n\tv_cndmask_b32_e64 %3, %7, %5, %8"
        : "=&v"(nsl), "=&v"(nsh), "=&v"(ncl), "=&v"(nch)
        : "v"(sl), "v"(sh), "v"(cl), "v"(ch), "s"(m));
    slot = ((unsigned long long)nsh << 32) | nsl;
    carry = ((unsigned long long)nch << 32) | ncl;
}

struct KnnSortedArgs {
    int n, nb, batch, k;
    const float4 *aos;   // [b][n] (x, y, z, original index) per sorted point (+ padding, see pcc::knn_sorted)
    const float *box;    // [b][nb][8]
    const int *perm;     // [b][n]
    int64_t *out;        // [b][n][k] in the caller's point order
};

// K = list slots (>= k), KPREV = the next smaller instantiation (k > KPREV)
template <int K, int KPREV>
__global__ __launch_bounds__(64 * kSW, (K == 16 ? 3 : K <= 25 ? 4 : 1)) void knn_sorted_kernel(KnnSortedArgs a) {  // (<= 128 VGPRs up to K = 25: four waves per SIMD; the carried chain of K = 16 needs 3 to stay out of scratch)
    // per wave: FIFO [kCap][64] x (distance, index), reused as the merge area [slice][K][16] x (distance 4 B | index 2 B:
    // n <= 16384) -- 6 bytes per entry keep K = 25 under 10 KB per wave, i.e. four waves per SIMD
    constexpr int kEntries = kSlices * K * kSQ;
    constexpr int kMergeWords = kEntries + (kEntries + 1) / 2;
    constexpr int kWaveWords = (2 * kCap * 64) > kMergeWords ? (2 * kCap * 64) : kMergeWords;
    __shared__ __attribute__((aligned(8))) unsigned smem[kSW * kWaveWords];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gw = (int)blockIdx.x * kSW + w;  // global wave = (sample, box)
    const int smp = gw / a.nb, grp = gw - smp * a.nb;
    if (smp >= a.batch) return;  // (whole wave; the kernel has no barrier)
    unsigned *wbase = smem + w * kWaveWords;
    float *buf_d = reinterpret_cast<float *>(wbase);
    int *buf_i = reinterpret_cast<int *>(wbase + kCap * 64);
    const int n = a.n, k = a.k;
    const int ql = lane & (kSQ - 1), cs = lane >> 4;
    const float4 *C = a.aos + (size_t)smp * n;
    const int qs = min(grp * kSQ + ql, n - 1);
    const float4 me = C[qs];
    const float4 *gb = reinterpret_cast<const float4 *>(a.box + ((size_t)smp * a.nb + grp) * 8);
    const float4 glo = gb[0], ghi = gb[1];

    // ascending; the list lives in the LAST k slots (the first K - k hold key 0, which nothing displaces), so that the
    // k-th entry is the static register pair key[K - 1]
    unsigned long long key[K];
#pragma unroll
    for (int s = 0; s < K; s++) key[s] = s < K - k ? 0ull : kKeyInf;
    // the slot whose entry bounds the query's k-th distance (see above): rank ceil(k/4) of the slice when k == K,
    // otherwise a static slot that has at least that rank for every k in (KPREV, K]
    // The insertion pass in its carry-free form (every slot from the old list) needs ~30 fewer VGPRs than the chain that
    // carries the displaced key from slot to slot, which decides the occupancy at K = 20 and 25 (four waves per SIMD
    // together with the 6-byte merge entries; surface clouds: 118 -> 104 us and 139 -> 133 us, Gaussian 231 -> 197 us at
    // K = 25) and is worth a few per cent at K <= 8; at K = 16 and 32 the carried chain measured faster (90 / 164 us
    // against 100 / 193) -- there the launch bound alone (128 VGPRs up to K = 25) is what helps (K = 16: 101 -> 90 us).
    constexpr bool kCarryFree = K <= 8 || K == 20 || K == 25;
    constexpr int kTight = K - 1 - (3 * K) / 4, kLoose = K - 1 - (3 * (KPREV + 1)) / 4;
    unsigned long long thr = kKeyInf;  // buffering threshold: min(own k-th key, the query's bound) at the last flush
    int cnt = 0;
    float r = __builtin_inff();        // the largest bound of the 16 queries

    auto flush = [&]() {
        for (int t = 0; t < kCap; t++) {
            if (!__any(t < cnt)) break;
            unsigned long long x = kKeyInf;
            if (t < cnt) x = ((unsigned long long)__float_as_uint(buf_d[t * 64 + lane]) << 32) | (unsigned)buf_i[t * 64 + lane];
            if (x < key[K - 1]) {
                if (kCarryFree) {
                    // every slot from the OLD list: key'[s] = x < key[s-1] ? key[s-1] : x < key[s] ? x : key[s]
                    bool lt[K];
#pragma unroll
                    for (int s = 0; s < K; s++) lt[s] = x < key[s];
#pragma unroll
                    for (int s = K - 1; s > 0; s--) key[s] = lt[s - 1] ? key[s - 1] : (lt[s] ? x : key[s]);
                    key[0] = lt[0] ? x : key[0];
                } else {
#pragma unroll
                    for (int s = 0; s < K; s++) ce_step(key[s], x);
                }
            }
        }
        cnt = 0;
        // the query's bound over its four slices, then the largest over the 16 queries (distance bits order like ints)
        int qb = (int)((k == K ? key[kTight] : key[kLoose]) >> 32);
        qb = max(qb, __shfl_xor(qb, 16, 64));
        qb = max(qb, __shfl_xor(qb, 32, 64));
        const unsigned long long bound = ((unsigned long long)(unsigned)qb << 32) | 0x7fffffffull;
        thr = key[K - 1] < bound ? key[K - 1] : bound;
        int m = grp * kSQ + ql < n ? qb : 0;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
        r = __int_as_float(__builtin_amdgcn_readfirstlane(m));
    };

    for (int b0 = 0; b0 < a.nb; b0 += 128) {  // windows of 128 candidate blocks
        unsigned bkey[2];
        // the candidates' own fma chain on the box gaps
        pcc::sort_box_window(bkey, a.box, smp, a.nb, b0, glo, ghi, lane, [](float dx, float dy, float dz) {
            return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        });
        const int nwin = min(128, a.nb - b0);
        // a lane's four candidates of a block are 64 contiguous bytes; the next block's are in flight while this one is
        // consumed.  Rows past the cloud's end are loaded (the workspace is padded) and never offered.
        auto load4 = [&](float4 (&v)[4], int c0) {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = C[c0 + cs * 4 + j];
        };
        unsigned bk = pcc::window_key(bkey, 0);
        float4 cur[4], nxt[4];
        load4(cur, (b0 + (int)(bk & 127u)) * pcc::kBox);
        for (int p = 0; p < nwin; p++) {
            if (__uint_as_float(bk & ~127u) > r) break;  // everything behind is farther still
            const int c0 = (b0 + (int)(bk & 127u)) * pcc::kBox;
            const unsigned bk_next = pcc::window_key(bkey, min(p + 1, nwin - 1));
            load4(nxt, (b0 + (int)(bk_next & 127u)) * pcc::kBox);
            if (__any(cnt > kCap - 4)) flush();
            const int left = n - c0 - cs * 4;  // real candidates from cur[0] on
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float dx = cur[j].x - me.x, dy = cur[j].y - me.y, dz = cur[j].z - me.z;
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                const unsigned long long x = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(cur[j].w);
                if (j < left && x < thr) {  // (false for NaN distances: their bits sort above +inf)
                    buf_d[cnt * 64 + lane] = d;
                    buf_i[cnt * 64 + lane] = __float_as_int(cur[j].w);
                    cnt++;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) cur[j] = nxt[j];
            if (__any(cnt > 0) && ((p & 7) == 7 || p < 8)) flush();  // fresh bounds: every block at first, then every 8th (measured)
            bk = bk_next;
        }
    }
    flush();

    // merge the four slice lists of every query: [slice][slot][query] keys in the wave's LDS region (the FIFO is drained)
    unsigned *md = wbase;                                                        // distance bits
    unsigned short *mi = reinterpret_cast<unsigned short *>(wbase + kEntries);  // original index (0xffff: the empty-slot sentinel)
    auto merged_key = [&](int e) -> unsigned long long {
        const unsigned i16 = mi[e];
        return ((unsigned long long)md[e] << 32) | (i16 == 0xffffu ? 0x7fffffffu : i16);
    };
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s = 0; s < K; s++) {
        const unsigned lo = (unsigned)key[s];
        md[(cs * K + s) * kSQ + ql] = (unsigned)(key[s] >> 32);
        mi[(cs * K + s) * kSQ + ql] = (unsigned short)(lo == 0x7fffffffu ? 0xffffu : lo);
    }
    __builtin_amdgcn_wave_barrier();
    if (cs == 0 && grp * kSQ + ql < n) {
        int64_t *dst = a.out + ((size_t)smp * n + a.perm[(size_t)smp * n + qs]) * k;
        int pos[kSlices];
        unsigned long long h[kSlices];
#pragma unroll
        for (int s = 0; s < kSlices; s++) {
            pos[s] = K - k;
            h[s] = merged_key((s * K + (K - k)) * kSQ + ql);
        }
        for (int o = 0; o < k; o++) {
            int best = 0;
            unsigned long long bv = h[0];
#pragma unroll
            for (int s = 1; s < kSlices; s++) {
                const bool lt = h[s] < bv;
                bv = lt ? h[s] : bv;
                best = lt ? s : best;
            }
            // (the lists run short only when fewer than k distances are not NaN -- a +inf distance has a key below
            // kKeyInf and enters like any other: never emit an index outside the cloud)
            dst[o] = (int64_t)min((int)(bv & 0xffffffffull), n - 1);
            int np = 0;
#pragma unroll
            for (int s = 0; s < kSlices; s++) np = best == s ? pos[s] + 1 : np;
            const unsigned long long nh = np < K ? merged_key((best * K + np) * kSQ + ql) : kKeyInf;
#pragma unroll
            for (int s = 0; s < kSlices; s++) {
                const bool sel = best == s;
                pos[s] = sel ? np : pos[s];
                h[s] = sel ? nh : h[s];
            }
        }
    }
}

template <int K>
int launch_small(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st) {
    static const char *const kNames[] = {"knn_small_kernel<4,4>", "knn_small_kernel<8,4>", "knn_small_kernel<16,4>",
                                         "knn_small_kernel<20,4>", "knn_small_kernel<25,4>", "knn_small_kernel<32,4>"};  // <K,S>
    pcc::ProfScope prof(kNames[slot_index(K)], st);
    hipLaunchKernelGGL((knn_small_kernel<K, 4>), dim3(pcc::ceil_div(n, 64), b), dim3(256), 0, st, c, n, k, x, indices);
    return PCC_OK;
}

template <int K>
int launch_sorted(const KnnSortedArgs &a, hipStream_t st) {
    static const char *const kNames[] = {"knn_sorted_kernel<4>", "knn_sorted_kernel<8>", "knn_sorted_kernel<16>",
                                         "knn_sorted_kernel<20>", "knn_sorted_kernel<25>", "knn_sorted_kernel<32>"};
    pcc::ProfScope prof(kNames[slot_index(K)], st);
    const int waves = a.batch * a.nb;
    hipLaunchKernelGGL((knn_sorted_kernel<K, prev_slots(K)>), dim3(pcc::ceil_div(waves, kSW)), dim3(64 * kSW), 0, st, a);
    return PCC_OK;
}

}  // namespace

int pcc::knn_sorted(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st) {
    // sorted search: workspace = packed sorted rows | boxes | permutation
    const int nb = pcc::ceil_div(n, pcc::kBox);
    // (+256: the search loads whole 16-row blocks; the last block of the last sample may run past the cloud)
    const size_t aos_b = (size_t)b * n * 16 + 256, box_b = (size_t)b * nb * 32;
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc(aos_b + box_b + (size_t)b * n * 4, "knn: workspace allocation failed")) return rc;
    char *base = static_cast<char *>(ws.p);
    float4 *aos = reinterpret_cast<float4 *>(base);
    float *box = reinterpret_cast<float *>(base + aos_b);
    int *perm = reinterpret_cast<int *>(base + aos_b + box_b);
    if (int rc = pcc::sort_cloud_cmajor(b, c, n, x, aos, box, perm, st)) return rc;
    const KnnSortedArgs a{n, nb, b, k, aos, box, perm, indices};
    with_slots(k, [&](auto K) { return launch_sorted<K>(a, st); });
    return pcc::check_launch("knn(sorted)");
}

int pcc::knn_small(int b, int c, int n, int k, const float *x, int64_t *indices, hipStream_t st) {
    with_slots(k, [&](auto K) { return launch_small<K>(b, c, n, k, x, indices, st); });
    return pcc::check_launch("knn(small)");
}
