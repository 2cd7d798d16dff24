// The grid index of a packed (ragged) batch (pcc_grid_cluster_ragged, include/pcc_neighbour.h), gfx950, wave64: every point
// of xyz[n, 3] / offset[b] gets the 64-bit key (cloud : q0 : q1 : q2) of its grid cell, the (key, point) pairs are sorted by a
// device-wide stable radix sort, and the runs of equal keys become the slots of the pooled level.  Clouds of any size, up to
// 2^16 cells per axis.  Integers only behind the key kernel; no float atomics; every output word is written once.
// The launches of one call, all on the caller's stream, their grids a function of (b, n, m, axis_bits) alone:
//   * rg_key_kernel: a thread per row.  The cloud by bisection over the clipped offsets (ragged_search.hip's rule, restated),
//     the cell per axis as floorf((x - start) / size) with a correctly rounded division, the key and the point index.
//   * per 8-bit digit, ceil((cloud_bits + 3 axis_bits) / 8) times, least significant digit first:
//       rg_hist_kernel     a workgroup per tile of kTile keys counts its digits in LDS (integer atomics: a sum of integers)
//                          and writes column `tile` of the table[256][tiles];
//       the scan (below)   over the table as it lies in memory, digit-major: the first output position of every
//                          (digit, tile);
//       rg_scatter_kernel  the same tiles.  A wave owns kTile / 4 consecutive keys of the tile and walks them 64 at a time:
//                          eight ballots find the lanes that hold the same digit, the first of them takes the wave's running
//                          count of that digit from LDS and adds the group, so a key's rank among its digit's keys is its
//                          rank in tile order -- the sort is stable by construction, and equal keys stay in point order.
//                          The keys are then laid out in LDS in sorted order and stored from there: the stores of one
//                          digit are contiguous.
//   * rg_heads_kernel: flag[pos] = the key at sorted position pos is valid and differs from the one before; the scan turns
//     the flags into the number of runs that start before every position.
//   * rg_bounds_kernel: a thread per cloud bisects the sorted keys for the first key of a later cloud: new_offset, n_cells,
//     and for the next launch the number of distinct and of valid keys.
//   * rg_emit_kernel: a thread per sorted position writes order, cluster (through the point index, range-checked), and at
//     the head of a kept run seg and the decoded coord; the threads behind the last run fill the tails of seg and coord.
// The scan is three launches -- rg_scan_reduce_kernel (a sum per block of kScanBlock words), rg_scan_partials_kernel (ONE
// workgroup walks the block sums kScanThreads at a time with a carry) and rg_scan_down_kernel (every block scans its words
// from its offset) --: no workgroup waits on another anywhere in this file.  Every loop is bounded by a size.
#include <cmath>
#include <cstdint>

#include "pcc_common.hpp"
#include "pcc_neighbour.h"
#include "wave_ops.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;                       // threads of the sort's workgroups: four waves
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;                           // keys per thread
constexpr int kTile = kThreads * kItems;            // keys per tile (PCC_GRID_RAGGED_TILE)
constexpr int kWaveKeys = kTile / kWaves;           // consecutive keys of a tile that one wave ranks
constexpr int kDigits = 256;                        // 8-bit digits
constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;                       // consecutive words per thread of the scan
constexpr int kScanBlock = kScanThreads * kScanItems;
static_assert(kTile == PCC_GRID_RAGGED_TILE, "the header documents the tile");
static_assert(kDigits == kThreads, "a thread per digit in the tile kernels");

// The clipped range of cloud c in a packed array of `total` rows, and the cloud that holds row i (-1: none): pcc_knn_ragged's
// rule, as in ragged_search.hip.
__device__ __forceinline__ void cloud_range(const int32_t *__restrict__ off, int c, int total, int &lo, int &hi) {
    lo = min(max(c > 0 ? off[c - 1] : 0, 0), total);
    hi = min(max(off[c], lo), total);
}
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

// One axis of the cell rule: t = (x - s) / size, every operation rounded; valid iff t >= 0 (false for NaN) and
// floorf(t) < 2^axis_bits.
__device__ __forceinline__ bool axis_cell_ragged(float x, float s, float size, float cells, unsigned &q) {
    const float t = (x - s) / size;
    const float f = floorf(t);
    const bool ok = t >= 0.f && f < cells;
    q = ok ? (unsigned)(int)f : 0u;
    return ok;
}

__global__ __launch_bounds__(kThreads) void rg_key_kernel(int b, int n, int axis_bits, const float *__restrict__ xyz,
                                                          const int32_t *__restrict__ offset, const float *__restrict__ start, float size,
                                                          u64 *__restrict__ keys, int32_t *__restrict__ idx) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = find_cloud(offset, b, n, (int)i);
    const float cells = (float)(1 << axis_bits);  // (exact: axis_bits <= 16)
    u64 key = (u64)(unsigned)b << (3 * axis_bits);  // the dropped key
    if (c >= 0) {
        const float *p = xyz + (size_t)i * 3, *s = start + (size_t)c * 3;
        unsigned q0, q1, q2;
        const bool ok0 = axis_cell_ragged(p[0], s[0], size, cells, q0);
        const bool ok1 = axis_cell_ragged(p[1], s[1], size, cells, q1);
        const bool ok2 = axis_cell_ragged(p[2], s[2], size, cells, q2);
        if (ok0 && ok1 && ok2)
            key = ((u64)(unsigned)c << (3 * axis_bits)) | ((u64)q0 << (2 * axis_bits)) | ((u64)q1 << axis_bits) | (u64)q2;
    }
    keys[i] = key;
    idx[i] = (int32_t)i;
}

// ---- the sort -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void rg_hist_kernel(int n, int tiles, int shift, const u64 *__restrict__ keys, int32_t *__restrict__ table) {
    __shared__ int hist[kDigits];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * kTile;
    hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kItems; j++) {
        const long long g = base + j * kThreads + tid;
        if (g < n) atomicAdd(&hist[(int)((keys[g] >> shift) & 255u)], 1);
    }
    __syncthreads();
    table[(size_t)tid * tiles + blockIdx.x] = hist[tid];
}

// The exclusive prefix sum of `v` over the workgroup's kScanThreads (or kThreads: both 256) threads, and their total.
__device__ __forceinline__ int block_exclusive_scan(int v, int *wave_tot, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, 64);
        incl += lane >= off ? u : 0;
    }
    __syncthreads();  // (wave_tot may still be read from the call before)
    if (lane == 63) wave_tot[w] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) {
        const int t = wave_tot[i];
        before += i < w ? t : 0;
        total += t;
    }
    return before + incl - v;
}

__global__ __launch_bounds__(kThreads) void rg_scatter_kernel(int n, int tiles, int shift, const u64 *__restrict__ keys_in,
                                                              const int32_t *__restrict__ idx_in, const int32_t *__restrict__ table,
                                                              u64 *__restrict__ keys_out, int32_t *__restrict__ idx_out) {
    __shared__ u64 skey[kTile];
    __shared__ int sidx[kTile];
    __shared__ int whist[kWaves][kDigits];  // per wave: the running count of every digit, then the count of the waves before
    __shared__ int dstart[kDigits];         // the first tile-sorted position of every digit
    __shared__ int goff[kDigits];           // global position of a digit's key = goff + its tile-sorted position
    __shared__ int wave_tot[kWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long base = (long long)blockIdx.x * kTile;
    const int count = (int)min((long long)kTile, (long long)n - base);  // keys of this tile (>= 1)
#pragma unroll
    for (int i = 0; i < kWaves; i++) whist[i][tid] = 0;
    __syncthreads();

    u64 key[kItems];
    int pt[kItems], dig[kItems], local[kItems];
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const int pos = w * kWaveKeys + r * 64 + lane;  // tile order: the wave's keys are consecutive
        const bool ok = pos < count;
        key[r] = ok ? keys_in[base + pos] : 0ull;
        pt[r] = ok ? idx_in[base + pos] : 0;
        const int d = (int)((key[r] >> shift) & 255u);
        dig[r] = d;
        // the lanes of the wave that hold a key with this digit
        u64 peers = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const u64 has = __ballot((d >> bit) & 1);
            peers &= ((d >> bit) & 1) ? has : ~has;
        }
        peers = ok ? peers : 0ull;
        const int first = peers ? (int)__builtin_ctzll(peers) : lane;
        int seen = 0;
        if (ok && lane == first) {  // one lane per digit: the addresses differ, and the table is this wave's own
            seen = whist[w][d];
            whist[w][d] = seen + (int)__popcll(peers);
        }
        seen = __shfl(seen, first, 64);
        local[r] = seen + pcc::lanes_below(peers);  // the rank among the wave's keys of this digit, in tile order
    }
    __syncthreads();
    {
        // thread = digit: the waves' counts become the counts of the waves before, the tile's digit counts its digit starts
        int run = 0;
#pragma unroll
        for (int i = 0; i < kWaves; i++) {
            const int t = whist[i][tid];
            whist[i][tid] = run;
            run += t;
        }
        int total;
        const int first = block_exclusive_scan(run, wave_tot, total);
        dstart[tid] = first;
        goff[tid] = table[(size_t)tid * tiles + blockIdx.x] - first;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; r++) {
        const int pos = w * kWaveKeys + r * 64 + lane;
        const int p = dstart[dig[r]] + whist[w][dig[r]] + local[r];
        if (pos < count && (unsigned)p < (unsigned)kTile) {
            skey[p] = key[r];
            sidx[p] = pt[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kItems; j++) {
        const int p = j * kThreads + tid;
        if (p < count) {
            const u64 k = skey[p];
            const long long g = (long long)goff[(int)((k >> shift) & 255u)] + p;
            if ((u64)g < (u64)n) {  // (the table is scratch: never an address without a check)
                keys_out[g] = k;
                idx_out[g] = sidx[p];
            }
        }
    }
}

// ---- the device-wide exclusive scan of int32 words, in place ------------------------------------------------------------------

__global__ __launch_bounds__(kScanThreads) void rg_scan_reduce_kernel(long long len, const int32_t *__restrict__ data, int32_t *__restrict__ partial) {
    __shared__ int wave_tot[kWaves];
    const long long at = ((long long)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    int v = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) v += at + j < len ? data[at + j] : 0;
    int total;
    (void)block_exclusive_scan(v, wave_tot, total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// One workgroup: partial[0, count) becomes its exclusive scan, partial[count] the total.
__global__ __launch_bounds__(kScanThreads) void rg_scan_partials_kernel(int count, int32_t *__restrict__ partial) {
    __shared__ int wave_tot[kWaves];
    int carry = 0;
    for (int c0 = 0; c0 < count; c0 += kScanThreads) {
        const int at = c0 + threadIdx.x;
        const int v = at < count ? partial[at] : 0;
        int total;
        const int before = block_exclusive_scan(v, wave_tot, total);
        if (at < count) partial[at] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) partial[count] = carry;
}

__global__ __launch_bounds__(kScanThreads) void rg_scan_down_kernel(long long len, int32_t *__restrict__ data, const int32_t *__restrict__ partial) {
    __shared__ int wave_tot[kWaves];
    const long long at = ((long long)blockIdx.x * kScanThreads + threadIdx.x) * kScanItems;
    int v[kScanItems], sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        v[j] = at + j < len ? data[at + j] : 0;
        sum += v[j];
    }
    int total;
    int run = partial[blockIdx.x] + block_exclusive_scan(sum, wave_tot, total);
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        if (at + j < len) data[at + j] = run;
        run += v[j];
    }
}

// ---- runs -------------------------------------------------------------------------------------------------------------------------

// The key at sorted position pos opens a run of a valid key.
__device__ __forceinline__ bool is_head(const u64 *__restrict__ keys, long long pos, u64 dropped) {
    const u64 k = keys[pos];
    return k < dropped && (pos == 0 || keys[pos - 1] != k);
}

__global__ __launch_bounds__(kThreads) void rg_heads_kernel(int n, u64 dropped, const u64 *__restrict__ keys, int32_t *__restrict__ flag) {
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (pos < n) flag[pos] = is_head(keys, pos, dropped) ? 1 : 0;
}

// The first sorted position whose key is >= bound (n: none).  n < 2^31: 31 halvings at the most.
__device__ __forceinline__ int first_at_least(const u64 *__restrict__ keys, int n, u64 bound) {
    int a = 0, e = n;
    for (int s = 0; s < 32 && a < e; s++) {
        const int mid = a + ((e - a) >> 1);
        if (keys[mid] >= bound) e = mid;
        else a = mid + 1;
    }
    return a;
}

// before[pos]: the runs that start before sorted position pos.  Thread c < b: cloud c; thread b: the counts.
__global__ __launch_bounds__(kThreads) void rg_bounds_kernel(int b, int n, int m, int axis_bits, const u64 *__restrict__ keys,
                                                             const int32_t *__restrict__ before, int32_t *__restrict__ new_offset,
                                                             int32_t *__restrict__ n_cells, int32_t *__restrict__ meta) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c > b) return;
    const u64 dropped = (u64)(unsigned)b << (3 * axis_bits);
    const int u = before[n - 1] + (is_head(keys, n - 1, dropped) ? 1 : 0);  // the distinct valid keys
    if (c == b) {
        n_cells[0] = u;
        meta[0] = u;
        meta[1] = first_at_least(keys, n, dropped);  // the valid points
        return;
    }
    const int at = first_at_least(keys, n, (u64)(unsigned)(c + 1) << (3 * axis_bits));  // the first key of a later cloud
    new_offset[c] = min(m, at < n ? before[at] : u);
}

__global__ __launch_bounds__(kThreads) void rg_emit_kernel(int b, int n, int m, int axis_bits, const u64 *__restrict__ keys,
                                                           const int32_t *__restrict__ idx, const int32_t *__restrict__ before,
                                                           const int32_t *__restrict__ meta, int32_t *__restrict__ cluster,
                                                           int32_t *__restrict__ order, int32_t *__restrict__ seg, int32_t *__restrict__ coord) {
    const long long pos = (long long)blockIdx.x * kThreads + threadIdx.x;  // [0, n]
    if (pos > n) return;
    const u64 dropped = (u64)(unsigned)b << (3 * axis_bits);
    if (pos < n) {
        const u64 k = keys[pos];
        const bool head = is_head(keys, pos, dropped);
        const int rank = before[pos] + (head ? 1 : 0) - 1;  // of this position's key among the distinct valid ones
        const int p = idx[pos];
        order[pos] = p;
        if ((unsigned)p < (unsigned)n) cluster[p] = k < dropped && rank >= 0 && rank < m ? rank : -1;
        if (head && rank >= 0 && rank <= m) {
            seg[rank] = (int32_t)pos;  // (rank m: the end of the last kept run)
            if (rank < m) {
                const unsigned mask = (1u << axis_bits) - 1u;
                int32_t *cr = coord + (size_t)rank * 4;
                cr[0] = (int32_t)(k >> (3 * axis_bits));
                cr[1] = (int32_t)((unsigned)(k >> (2 * axis_bits)) & mask);
                cr[2] = (int32_t)((unsigned)(k >> axis_bits) & mask);
                cr[3] = (int32_t)((unsigned)k & mask);
            }
        }
    }
    // the slots behind the last run: empty runs at the end of the valid points
    const int u = meta[0];
    if (pos <= m && pos >= u) {
        seg[pos] = meta[1];
        if (pos < m) {
            int32_t *cr = coord + (size_t)pos * 4;
            cr[0] = cr[1] = cr[2] = cr[3] = -1;
        }
    }
}

int bit_width(unsigned v) {
    int w = 0;
    for (; v; v >>= 1) w++;
    return w;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// In place; `partial` holds ceil(len / kScanBlock) + 1 words.
void exclusive_scan(long long len, int32_t *data, int32_t *partial, hipStream_t st) {
    const int blocks = (int)((len + kScanBlock - 1) / kScanBlock);
    {
        pcc::ProfScope prof("rg_scan_reduce_kernel", st);
        hipLaunchKernelGGL(rg_scan_reduce_kernel, dim3((unsigned)blocks), dim3(kScanThreads), 0, st, len, data, partial);
    }
    {
        pcc::ProfScope prof("rg_scan_partials_kernel", st);
        hipLaunchKernelGGL(rg_scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, st, blocks, partial);
    }
    {
        pcc::ProfScope prof("rg_scan_down_kernel", st);
        hipLaunchKernelGGL(rg_scan_down_kernel, dim3((unsigned)blocks), dim3(kScanThreads), 0, st, len, data, partial);
    }
}

}  // namespace

extern "C" int pcc_grid_cluster_ragged(int b, int n, int m, int axis_bits, const float *xyz, const int32_t *offset, const float *start,
                                       float size, int32_t *cluster, int32_t *order, int32_t *seg, int32_t *coord, int32_t *new_offset,
                                       int32_t *n_cells, pcc_stream_t stream) {
    pcc::clear_error();
    if (n < 1 || m < 1 || m > n || b < 1) return pcc::invalid("grid_cluster_ragged: bad size");
    if (b > 65535) return pcc::invalid("grid_cluster_ragged: batch too large");
    if ((long long)n + 1 >= (1ll << 31)) return pcc::invalid("grid_cluster_ragged: too many points (n + 1 >= 2^31)");
    if (axis_bits < 1 || axis_bits > 16) return pcc::invalid("grid_cluster_ragged: axis_bits must be in [1, 16]");
    const int key_bits = bit_width((unsigned)b) + 3 * axis_bits;
    if (key_bits > 63) return pcc::invalid("grid_cluster_ragged: the key is wider than 63 bits");
    if (!std::isfinite(size) || !(size > 0.f)) return pcc::invalid("grid_cluster_ragged: size must be finite and > 0");
    if (!xyz || !offset || !start || !cluster || !order || !seg || !coord || !new_offset || !n_cells)
        return pcc::invalid("grid_cluster_ragged: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);

    const int tiles = (int)(((long long)n + kTile - 1) / kTile);
    const long long table_len = (long long)kDigits * tiles;
    const long long scan_len = table_len > n ? table_len : n;
    const size_t key_bytes = align16((size_t)n * sizeof(u64)), idx_bytes = align16((size_t)n * sizeof(int32_t));
    const size_t table_bytes = align16((size_t)table_len * sizeof(int32_t));
    const size_t partial_bytes = align16((size_t)((scan_len + kScanBlock - 1) / kScanBlock + 1) * sizeof(int32_t));
    pcc::WsBlock ws(st);
    if (int rc = ws.alloc(2 * key_bytes + 3 * idx_bytes + table_bytes + partial_bytes + 16, "grid_cluster_ragged: workspace allocation failed")) return rc;
    unsigned char *at = static_cast<unsigned char *>(ws.p);
    const auto carve = [&](size_t bytes) {
        unsigned char *p = at;
        at += bytes;
        return p;
    };
    u64 *keys[2] = {reinterpret_cast<u64 *>(carve(key_bytes)), reinterpret_cast<u64 *>(carve(key_bytes))};
    int32_t *idx[2] = {reinterpret_cast<int32_t *>(carve(idx_bytes)), reinterpret_cast<int32_t *>(carve(idx_bytes))};
    int32_t *before = reinterpret_cast<int32_t *>(carve(idx_bytes));
    int32_t *table = reinterpret_cast<int32_t *>(carve(table_bytes));
    int32_t *partial = reinterpret_cast<int32_t *>(carve(partial_bytes));
    int32_t *meta = reinterpret_cast<int32_t *>(carve(16));

    const unsigned row_blocks = (unsigned)(((long long)n + kThreads - 1) / kThreads);
    {
        pcc::ProfScope prof("rg_key_kernel", st);
        hipLaunchKernelGGL(rg_key_kernel, dim3(row_blocks), dim3(kThreads), 0, st, b, n, axis_bits, xyz, offset, start, size, keys[0], idx[0]);
    }
    int cur = 0;
    for (int shift = 0; shift < key_bits; shift += 8, cur ^= 1) {
        {
            pcc::ProfScope prof("rg_hist_kernel", st);
            hipLaunchKernelGGL(rg_hist_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, n, tiles, shift, keys[cur], table);
        }
        exclusive_scan(table_len, table, partial, st);
        pcc::ProfScope prof("rg_scatter_kernel", st);
        hipLaunchKernelGGL(rg_scatter_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, n, tiles, shift, keys[cur], idx[cur], table,
                           keys[cur ^ 1], idx[cur ^ 1]);
    }
    const u64 dropped = (u64)(unsigned)b << (3 * axis_bits);
    {
        pcc::ProfScope prof("rg_heads_kernel", st);
        hipLaunchKernelGGL(rg_heads_kernel, dim3(row_blocks), dim3(kThreads), 0, st, n, dropped, keys[cur], before);
    }
    exclusive_scan(n, before, partial, st);
    {
        pcc::ProfScope prof("rg_bounds_kernel", st);
        hipLaunchKernelGGL(rg_bounds_kernel, dim3((unsigned)(b / kThreads + 1)), dim3(kThreads), 0, st, b, n, m, axis_bits, keys[cur], before,
                           new_offset, n_cells, meta);
    }
    {
        pcc::ProfScope prof("rg_emit_kernel", st);
        hipLaunchKernelGGL(rg_emit_kernel, dim3((unsigned)(((long long)n + 1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, b, n, m,
                           axis_bits, keys[cur], idx[cur], before, meta, cluster, order, seg, coord);
    }
    return pcc::check_launch("grid_cluster_ragged");
}
