// Searches over packed (ragged) batches (pcc_knn_ragged, pcc_ball_query_ragged: include/pcc_neighbour.h), gfx950, wave64.
//
// A packed batch is xyz[n, 3] with offset[b], the cumulative ends of its clouds; the queries are packed the same way.  The
// offsets stay on the device: a query finds its cloud by bisection over the clipped query offsets (<= 16 steps, b <= 65535)
// and reads the clipped point range [lo, hi) of that cloud.  A workgroup owns consecutive query rows, so its clouds are
// consecutive too, and it scans the union [lowest lo, highest hi) of their ranges in LDS chunks copied as they lie in
// memory (x, y, z interleaved).  A query takes only the candidates of its own [lo, hi): one unsigned compare per candidate
// in the k-NN kernel, a clamp of the wave's loop bounds in the ball kernel.
//   * knn_ragged_kernel<K>: 64 queries per workgroup, a lane per query (knn_small_kernel's shape, knn_lowdim.hip): the four
//     waves split every staged chunk, each lane keeps a buffered top-K (topk.hpp), and the four lists of a query are merged
//     at the end by (distance, index) keys.  The lists take a candidate with a strict `<` against a threshold that starts
//     at +inf, so +inf distances are appended afterwards (fill_inf_tail, knn.hpp); what is still missing is (-1, +inf).
//   * ball_ragged_kernel: a wave per centre, 16 centres per workgroup over shared tiles (ball_lds_kernel's shape,
//     ball_query.hip): ballot, pcc::lanes_below, and the workgroup stops as soon as none of its centres has candidates left
//     (__syncthreads_or).
// Every loop is bounded by n, k or nsample (the bisection by 16); no atomics, no workspace, and the workgroups share
// nothing.  Nothing is read outside xyz[0, n), offset[0, b) and the m query rows, whatever the offsets hold.
#include "knn.hpp"
#include "pcc_neighbour.h"
#include "topk.hpp"
#include "wave_ops.hpp"

namespace {

typedef unsigned long long u64;

// The clipped range of cloud c in a packed array of `total` rows (the header's rule).
__device__ __forceinline__ void cloud_range(const int32_t *__restrict__ off, int c, int total, int &lo, int &hi) {
    lo = min(max(c > 0 ? off[c - 1] : 0, 0), total);
    hi = min(max(off[c], lo), total);
}

// The cloud whose clipped range holds row i of a packed array of `total` rows, -1 when there is none: the first cloud
// whose clipped end lies behind i (bisection: b <= 65535 halves to nothing in 16 steps), if its range holds i.  On offsets
// that do not ascend the bisection ends somewhere, and the check keeps the answer a cloud that holds i, or none.
__device__ __forceinline__ int find_cloud(const int32_t *__restrict__ off, int b, int total, int i) {
    int a = 0, e = b;
    for (int s = 0; s < 16 && a < e; s++) {
        const int mid = (a + e) >> 1;
        if (min(max(off[mid], 0), total) > i) e = mid;
        else a = mid + 1;
    }
    if (a >= b) return -1;
    int lo, hi;
    cloud_range(off, a, total, lo, hi);
    return i >= lo && i < hi ? a : -1;
}

// ---- k-NN -----------------------------------------------------------------------------------------------------------------

constexpr int kCH = 2048;  // candidates staged per chunk
constexpr int kS = 4;      // waves per workgroup: each takes a quarter of every chunk

template <int K>
struct RaggedLayout {
    static constexpr int T = 64 * kS;
    static constexpr int cand_bytes = 3 * kCH * 4;
    static constexpr int buf_bytes = 2 * kCap * T * 4;
    static constexpr int merge_bytes = 2 * kS * K * 64 * 4;
    static constexpr int bytes = (cand_bytes + buf_bytes) > merge_bytes ? (cand_bytes + buf_bytes) : merge_bytes;
};

// Merge the kS sorted K-lists of a lane (LDS layout [wave][slot][lane]) by 64-bit keys (distance bits : index), as
// merge_and_store of knn_lowdim.hip does: the distances are non-negative and never NaN, so one unsigned compare is "smaller
// distance, then lower index".  Writes k slots; a slot behind the last entry is (-1, +inf).  -> the slots that took an entry.
template <int K>
__device__ __forceinline__ int merge_ragged(const float *md, const int *mi, int lane, int k, int64_t *di, float *dd) {
    const auto entry = [&](int s, int pos) -> u64 {
        return ((u64)__float_as_uint(md[(s * K + pos) * 64 + lane]) << 32) | (unsigned)mi[(s * K + pos) * 64 + lane];
    };
    constexpr u64 kNone = ((u64)0x7f800000u << 32) | 0x7fffffffull;  // an empty slot of TopK: (+inf, 0x7fffffff)
    int p[kS];
    u64 h[kS];
    int filled = 0;
#pragma unroll
    for (int s = 0; s < kS; s++) {
        p[s] = 0;
        h[s] = entry(s, 0);
    }
    for (int o = 0; o < k; o++) {
        int best = 0;
        u64 bv = h[0];
#pragma unroll
        for (int s = 1; s < kS; s++) {
            const bool lt = h[s] < bv;
            bv = lt ? h[s] : bv;
            best = lt ? s : best;
        }
        int pos = 0;
#pragma unroll
        for (int s = 0; s < kS; s++) pos = (best == s) ? p[s] : pos;
        const bool real = (unsigned)bv != 0x7fffffffu;  // (no point has that index: n < 2^31)
        di[o] = real ? (int64_t)(int)(unsigned)bv : (int64_t)-1;
        if (dd) dd[o] = real ? __uint_as_float((unsigned)(bv >> 32)) : __builtin_inff();
        filled += real ? 1 : 0;
        const int np = pos + 1;
        const u64 nh = np < K ? entry(best, np) : kNone;
#pragma unroll
        for (int s = 0; s < kS; s++) {
            const bool sel = best == s;
            p[s] = sel ? np : p[s];
            h[s] = sel ? nh : h[s];
        }
    }
    return filled;
}

template <int K>
__global__ __launch_bounds__(64 * kS) void knn_ragged_kernel(int b, int n, int m, int k, const float *__restrict__ xyz,
                                                              const int32_t *__restrict__ offset, const float *__restrict__ query,
                                                              const int32_t *__restrict__ query_offset, int64_t *__restrict__ idx,
                                                              float *__restrict__ dist) {
    using L = RaggedLayout<K>;
    constexpr int T = L::T;
    __shared__ __attribute__((aligned(16))) unsigned char smem[L::bytes];
    float *lds_c = reinterpret_cast<float *>(smem);
    float *buf_d = reinterpret_cast<float *>(smem + L::cand_bytes);
    int *buf_i = reinterpret_cast<int *>(smem + L::cand_bytes + kCap * T * 4);
    float *mrg_d = reinterpret_cast<float *>(smem);
    int *mrg_i = reinterpret_cast<int *>(smem + kS * K * 64 * 4);

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // every wave holds the same 64 queries, a lane each
    const long long row = (long long)blockIdx.x * 64 + lane;
    const bool row_ok = row < m;
    int lo = 0, hi = 0;  // the candidates of this query: none for a row of no cloud
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (row_ok) {
        const int cloud = find_cloud(query_offset, b, m, (int)row);
        if (cloud >= 0) cloud_range(offset, cloud, n, lo, hi);
        qx = query[(size_t)row * 3], qy = query[(size_t)row * 3 + 1], qz = query[(size_t)row * 3 + 2];
    }
    // the union of the ranges of the 64 queries (the same in every wave, so the barriers below are uniform)
    int ulo = hi > lo ? lo : 0x7fffffff, uhi = hi > lo ? hi : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ulo = min(ulo, __shfl_xor(ulo, o, 64));
        uhi = max(uhi, __shfl_xor(uhi, o, 64));
    }
    ulo = __builtin_amdgcn_readfirstlane(ulo), uhi = __builtin_amdgcn_readfirstlane(uhi);
    const unsigned span = (unsigned)(hi - lo);

    pcc::BufferedTopK<K, kCap, T> tk;
    tk.init(buf_d, buf_i, tid);
    const float4 *C4 = reinterpret_cast<const float4 *>(lds_c);

    for (int c0 = ulo; c0 < uhi; c0 += kCH) {
        const int cnt = min(kCH, uhi - c0);
        const int ngroups = (cnt + 7) / 8;
        if (c0 != ulo) __syncthreads();
        const float *src = xyz + (size_t)c0 * 3;  // (c0 + cnt <= uhi <= n)
        for (int e = tid; e < ngroups * 24; e += T) lds_c[e] = e < cnt * 3 ? src[e] : __builtin_inff();
        __syncthreads();
        const int gs = (ngroups + kS - 1) / kS;
        const int g_begin = w * gs;
        const int g_end = min(g_begin + gs, ngroups);
        for (int g = g_begin; g < g_end; g++) {
            // eight candidates, 24 words: x0 y0 z0 x1 | y1 z1 x2 y2 | z2 x3 y3 z3 | ... (every lane the same address)
            const float4 v0 = C4[6 * g], v1 = C4[6 * g + 1], v2 = C4[6 * g + 2];
            const float4 v3 = C4[6 * g + 3], v4 = C4[6 * g + 4], v5 = C4[6 * g + 5];
            const float cx[8] = {v0.x, v0.w, v1.z, v2.y, v3.x, v3.w, v4.z, v5.y};
            const float cy[8] = {v0.y, v1.x, v1.w, v2.z, v3.y, v4.x, v4.w, v5.z};
            const float cz[8] = {v0.z, v1.y, v2.x, v2.w, v3.z, v4.y, v5.x, v5.w};
            if (tk.must_flush(8)) tk.flush();
            const unsigned j0 = (unsigned)c0 + (unsigned)g * 8u;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float d = pcc::sqdist(cx[j], cy[j], cz[j], qx, qy, qz);
                // a candidate of the query's own cloud (one unsigned compare: lo <= j0 + j < hi); the slots behind the
                // chunk's end lie behind every hi, and their words are +inf
                if (j0 + j - (unsigned)lo < span) tk.offer(d, (int)(j0 + j));
            }
        }
        if (uhi - c0 <= kCH) break;  // (c0 never passes n, so it cannot overflow)
    }
    tk.flush();
    __syncthreads();  // every wave is done with the candidate / FIFO regions: reuse them for the merge
#pragma unroll
    for (int s = 0; s < K; s++) {
        mrg_d[(w * K + s) * 64 + lane] = tk.top.d[s];
        mrg_i[(w * K + s) * 64 + lane] = tk.top.i[s];
    }
    __syncthreads();
    if (w == 0 && row_ok) {
        int64_t *di = idx + (size_t)row * k;
        float *dd = dist ? dist + (size_t)row * k : nullptr;
        const int filled = merge_ragged<K>(mrg_d, mrg_i, lane, k, di, dd);
        // the lists hold finite distances only: a short row continues with its +inf distances (fill_inf_tail), whose
        // dist words merge_ragged has written already.  A NaN query has none.
        if (filled < k && hi > lo && qx == qx && qy == qy && qz == qz) {
            const float *xb = xyz + (size_t)lo * 3;
            fill_inf_tail(
                filled, k, hi - lo,
                [&](int j) { return pcc::sqdist(xb[(size_t)j * 3], xb[(size_t)j * 3 + 1], xb[(size_t)j * 3 + 2], qx, qy, qz); },
                [&](int slot, int j) { di[slot] = (int64_t)lo + j; });
        }
    }
}

// ---- ball query -----------------------------------------------------------------------------------------------------------

constexpr int kBallWaves = 16;   // centres per workgroup
constexpr int kBallTile = 4096;  // candidates per LDS tile (ball_lds_kernel's product shape)
constexpr int kUnroll = 4;       // blocks of 64 candidates per step

__global__ __launch_bounds__(kBallWaves * 64) void ball_ragged_kernel(int b, int n, int m, int nsample, float r2, int pad,
                                                                     const float *__restrict__ xyz, const int32_t *__restrict__ offset,
                                                                     const float *__restrict__ centres,
                                                                     const int32_t *__restrict__ centre_offset, int64_t *__restrict__ idx,
                                                                     int32_t *__restrict__ cnt) {
    __shared__ float tile[kBallTile * 3];
    __shared__ int range[2 * kBallWaves];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kBallWaves + wave;  // the centre of this wave
    const bool active = row < m;
    int lo = 0, hi = 0;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (active) {
        const int cloud = find_cloud(centre_offset, b, m, (int)row);
        if (cloud >= 0) cloud_range(offset, cloud, n, lo, hi);
        lo = __builtin_amdgcn_readfirstlane(lo), hi = __builtin_amdgcn_readfirstlane(hi);
        cx = centres[(size_t)row * 3], cy = centres[(size_t)row * 3 + 1], cz = centres[(size_t)row * 3 + 2];
    }
    const bool has = active && hi > lo;  // (wave-uniform, like everything below but `lane`)
    if (lane == 0) range[wave] = has ? lo : 0x7fffffff, range[kBallWaves + wave] = has ? hi : 0;
    __syncthreads();
    int ulo = 0x7fffffff, uhi = 0;  // the union of the workgroup's ranges
#pragma unroll
    for (int s = 0; s < kBallWaves; s++) ulo = min(ulo, range[s]), uhi = max(uhi, range[kBallWaves + s]);

    // the list of this wave: pcc_ball_query's rule (Ball of ball_query.hip) with global indices
    int64_t *out = idx + (size_t)(active ? row : 0) * nsample;
    int count = 0, first = lo;
    for (int t0 = ulo; t0 < uhi; t0 += kBallTile) {
        const int len = min(uhi - t0, kBallTile);  // points of this tile: t0 + len <= uhi <= n
        const float *src = xyz + (size_t)t0 * 3;
        for (int e = threadIdx.x; e < len * 3; e += kBallWaves * 64) tile[e] = src[e];
        __syncthreads();
        if (has && count < nsample) {
            // the part of the tile that belongs to this wave's cloud (empty when the cloud lies before or behind it)
            const int begin = max(lo, t0) - t0, end = min(hi, t0 + len) - t0;
            for (int base = begin; base < end && count < nsample; base += 64 * kUnroll) {
#pragma unroll
                for (int u = 0; u < kUnroll; u++) {
                    if (count >= nsample) continue;
                    const int off = base + u * 64 + lane;
                    const bool valid = off < end;  // (< len <= kBallTile)
                    const int wd = valid ? off * 3 : 0;
                    const bool inside = valid && pcc::sqdist(tile[wd], tile[wd + 1], tile[wd + 2], cx, cy, cz) < r2;  // (false for NaN)
                    const u64 mask = __ballot(inside);
                    if (mask == 0) continue;
                    if (count == 0) first = t0 + base + u * 64 + (int)__builtin_ctzll(mask);
                    const int slot = count + pcc::lanes_below(mask);
                    if (inside && slot < nsample) out[slot] = (int64_t)(t0 + off);
                    count += (int)__popcll(mask);
                }
            }
        }
        const int more = has && count < nsample && hi > t0 + len;
        if (!__syncthreads_or(more) || uhi - t0 <= kBallTile) break;  // (that barrier also keeps the next copy behind these reads)
    }
    if (active) {
        const int c = count < nsample ? count : nsample;
        // a row of no cloud, or of a cloud without points, has nothing a FIRST padding could name
        const int64_t fill = has && pad == PCC_BALL_PAD_FIRST ? (int64_t)first : (int64_t)-1;
        for (int s = c + lane; s < nsample; s += 64) out[s] = fill;
        if (cnt && lane == 0) cnt[row] = c;
    }
}

}  // namespace

extern "C" int pcc_knn_ragged(int b, int n, int m, int k, const float *xyz, const int32_t *offset, const float *query,
                              const int32_t *query_offset, int64_t *idx, float *dist, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 0 || m < 0 || k < 1) return pcc::invalid("knn_ragged: bad size");
    if (k > 32) return pcc::invalid("knn_ragged: k > 32 is not supported in this version");
    if (b > 65535) return pcc::invalid("knn_ragged: batch too large");
    if (b == 0 || m == 0) return PCC_OK;
    if ((!xyz && n > 0) || !offset || !query || !query_offset || !idx) return pcc::invalid("knn_ragged: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_slots(k, [&](auto K) {
        pcc::ProfScope prof("knn_ragged_kernel", st);
        hipLaunchKernelGGL((knn_ragged_kernel<decltype(K)::value>), dim3((unsigned)(((long long)m + 63) / 64)), dim3(64 * kS), 0, st, b, n, m, k, xyz,
                           offset, query, query_offset, idx, dist);
        return PCC_OK;
    });
    return pcc::check_launch("knn_ragged");
}

extern "C" int pcc_ball_query_ragged(int b, int n, int m, int nsample, float radius, int pad, const float *xyz,
                                     const int32_t *offset, const float *centres, const int32_t *centre_offset, int64_t *idx,
                                     int32_t *cnt, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || m < 0 || n < 1 || nsample < 1) return pcc::invalid("ball_query_ragged: bad size");
    if (!(radius > 0.f)) return pcc::invalid("ball_query_ragged: radius must be > 0");
    if (pad != PCC_BALL_PAD_FIRST && pad != PCC_BALL_PAD_NONE) return pcc::invalid("ball_query_ragged: pad must be 0 (first) or 1 (none)");
    if (b > 65535) return pcc::invalid("ball_query_ragged: batch too large");
    if (b == 0 || m == 0) return PCC_OK;
    if (!xyz || !offset || !centres || !centre_offset || !idx) return pcc::invalid("ball_query_ragged: null pointer");
    const float r2 = radius * radius;  // one float32 multiplication (-ffp-contract=off)
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        pcc::ProfScope prof("ball_ragged_kernel", st);
        hipLaunchKernelGGL(ball_ragged_kernel, dim3((unsigned)(((long long)m + kBallWaves - 1) / kBallWaves)), dim3(kBallWaves * 64), 0,
                           st, b, n, m, nsample, r2, pad, xyz, offset, centres, centre_offset, idx, cnt);
    }
    return pcc::check_launch("ball_query_ragged");
}
