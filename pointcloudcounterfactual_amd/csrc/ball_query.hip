// Ball query (pcc_ball_query, include/pcc_neighbour.h), gfx950, wave64.
//
// One wave answers one query.  Lane l tests candidate base + l; one ballot gives the 64-bit mask of the candidates inside
// the ball; a lane's output slot is count + (inside lanes below it) (pcc::lanes_below), so the list comes out in ascending
// index order with no sort and no atomic, and the stores of a step are contiguous.  count += popcount(mask) is
// wave-uniform, so the loop ends for the whole wave as soon as the list is full or the cloud is exhausted; the same wave
// then writes the padding.  A step takes kUnroll blocks of 64 candidates: the direct kernel issues their loads together;
// each block is tested and appended in index order, and a block behind a full list is skipped.  (Testing all the blocks
// of a step before appending any was measured and is slower: DESIGN.md section 4f.)
//   * ball_direct_kernel<WAVES>: every wave reads the candidates straight from global memory (a 2048-point cloud is 24 KB:
//     the WAVES queries of a workgroup and its neighbours read it from L1 / L2);
//   * ball_lds_kernel<WAVES, TILE>: the workgroup copies TILE candidates into LDS as they lie in memory (x, y, z
//     interleaved: lane l reads words 3 l + c, and 3 is odd, so the 32 lanes of a group fall on 32 different banks), every
//     wave scans the tile, and the workgroup goes on to the next tile while any of its queries is unfinished
//     (__syncthreads_or: that barrier also keeps the next copy behind the last read of this one).
// Every loop is bounded by n (the padding loop by nsample); the workgroups share nothing.
#include "pcc_common.hpp"
#include "pcc_neighbour.h"
#include "pcc_test_hooks.h"
#include "wave_ops.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kUnroll = 4;  // blocks of 64 candidates per step

// One query's list while its wave scans the cloud.  Everything but `lane` is wave-uniform.
struct Ball {
    float cx, cy, cz, r2;
    int nsample, count, first, lane;
    int64_t *out;

    __device__ __forceinline__ bool full() const { return count >= nsample; }

    // candidate j = base + lane at (x, y, z); `valid`: j is a point of the cloud
    __device__ __forceinline__ void take(int base, bool valid, float x, float y, float z) {
        const bool inside = valid && pcc::sqdist(x, y, z, cx, cy, cz) < r2;  // (false for a NaN distance)
        const u64 mask = __ballot(inside);
        if (mask == 0) return;
        if (count == 0) first = base + (int)__builtin_ctzll(mask);
        const int slot = count + pcc::lanes_below(mask);
        if (inside && slot < nsample) out[slot] = (int64_t)(base + lane);
        count += (int)__popcll(mask);
    }

    // slots cnt .. nsample - 1, and the count
    __device__ __forceinline__ void finish(int pad, int32_t *cnt) {
        const int c = count < nsample ? count : nsample;
        const int64_t fill = pad == PCC_BALL_PAD_FIRST ? (int64_t)first : (int64_t)-1;
        for (int s = c + lane; s < nsample; s += 64) out[s] = fill;
        if (cnt && lane == 0) *cnt = c;
    }
};

// The query of this wave: q = blockIdx.x * WAVES + wave of cloud blockIdx.y; false for a wave past the last query.
template <int WAVES>
__device__ __forceinline__ bool open_ball(Ball &ball, int m, int nsample, float r2, const float *__restrict__ centres,
                                          int64_t *__restrict__ idx, int32_t *__restrict__ &cnt) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long q = (long long)blockIdx.x * WAVES + wave;
    ball.lane = threadIdx.x & 63;
    ball.nsample = nsample, ball.r2 = r2, ball.count = 0, ball.first = 0;
    if (q >= m) return false;
    const size_t row = (size_t)blockIdx.y * m + (size_t)q;
    ball.cx = centres[row * 3], ball.cy = centres[row * 3 + 1], ball.cz = centres[row * 3 + 2];
    ball.out = idx + row * nsample;
    if (cnt) cnt += row;
    return true;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void ball_direct_kernel(int n, int m, int nsample, float r2, int pad,
                                                                 const float *__restrict__ xyz, const float *__restrict__ centres,
                                                                 int64_t *__restrict__ idx, int32_t *__restrict__ cnt) {
    Ball ball;
    if (!open_ball<WAVES>(ball, m, nsample, r2, centres, idx, cnt)) return;
    const float *xb = xyz + (size_t)blockIdx.y * n * 3;
    for (int base = 0; !ball.full(); base += 64 * kUnroll) {
        float x[kUnroll], y[kUnroll], z[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int off = u * 64 + ball.lane;
            valid[u] = off < n - base;
            const size_t j = (size_t)base + (size_t)off;
            x[u] = y[u] = z[u] = 0.f;
            if (valid[u]) x[u] = xb[j * 3], y[u] = xb[j * 3 + 1], z[u] = xb[j * 3 + 2];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            if (!ball.full()) ball.take(base + u * 64, valid[u], x[u], y[u], z[u]);
        if (n - base <= 64 * kUnroll) break;  // (the cloud is exhausted; base never passes n, so it cannot overflow)
    }
    ball.finish(pad, cnt);
}

template <int WAVES, int TILE>
__global__ __launch_bounds__(WAVES * 64) void ball_lds_kernel(int n, int m, int nsample, float r2, int pad,
                                                              const float *__restrict__ xyz, const float *__restrict__ centres,
                                                              int64_t *__restrict__ idx, int32_t *__restrict__ cnt) {
    static_assert(TILE % (64 * kUnroll) == 0, "ball_query: a tile is whole steps");
    __shared__ float tile[TILE * 3];
    Ball ball;
    const bool active = open_ball<WAVES>(ball, m, nsample, r2, centres, idx, cnt);
    const float *xb = xyz + (size_t)blockIdx.y * n * 3;
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int len = n - t0 < TILE ? n - t0 : TILE;  // points of this tile
        const float *src = xb + (size_t)t0 * 3;
        for (int e = threadIdx.x; e < len * 3; e += WAVES * 64) tile[e] = src[e];
        __syncthreads();
        if (active) {
            for (int base = 0; base < len && !ball.full(); base += 64 * kUnroll) {
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int off = base + u * 64 + ball.lane;  // (< TILE)
                    const bool valid = off < len;
                    const int w = valid ? off * 3 : 0;
                    if (!ball.full()) ball.take(t0 + base + u * 64, valid, tile[w], tile[w + 1], tile[w + 2]);
                }
            }
        }
        const int more = active && !ball.full();
        if (!__syncthreads_or(more) || n - t0 <= TILE) break;
    }
    if (active) ball.finish(pad, cnt);
}

template <int WAVES>
void launch_direct(const char *name, int b, int n, int m, int nsample, float r2, int pad, const float *xyz, const float *centres, int64_t *idx,
                   int32_t *cnt, hipStream_t st) {
    pcc::ProfScope prof(name, st);
    hipLaunchKernelGGL((ball_direct_kernel<WAVES>), dim3((m - 1) / WAVES + 1, b), dim3(WAVES * 64), 0, st, n, m, nsample, r2,
                       pad, xyz, centres, idx, cnt);
}
template <int WAVES, int TILE>
void launch_lds(const char *name, int b, int n, int m, int nsample, float r2, int pad, const float *xyz, const float *centres, int64_t *idx,
                int32_t *cnt, hipStream_t st) {
    pcc::ProfScope prof(name, st);
    hipLaunchKernelGGL((ball_lds_kernel<WAVES, TILE>), dim3((m - 1) / WAVES + 1, b), dim3(WAVES * 64), 0, st, n, m, nsample,
                       r2, pad, xyz, centres, idx, cnt);
}

// The variants: value v of the ball_path switch forces kPaths[v - 1]; kProduct is what a call takes without it
// (DESIGN.md section 4f has the measurements behind the choice).
typedef void (*Launch)(const char *, int, int, int, int, float, int, const float *, const float *, int64_t *, int32_t *, hipStream_t);
const Launch kPaths[] = {launch_direct<4>, launch_direct<16>, launch_lds<4, 1024>, launch_lds<16, 4096>};
// ... under these names in the launch profile: the instantiation, <WAVES> and <WAVES,TILE>
const char *const kNames[] = {"ball_direct_kernel<4>", "ball_direct_kernel<16>", "ball_lds_kernel<4,1024>", "ball_lds_kernel<16,4096>"};
constexpr int kNumPaths = (int)(sizeof kPaths / sizeof kPaths[0]);
static_assert(sizeof kNames / sizeof kNames[0] == kNumPaths, "ball_query: one profile name per variant");
constexpr int kProduct = 3;  // 16 queries per workgroup over LDS tiles of 4096 candidates: the fastest at every shape measured

}  // namespace

extern "C" int pcc_ball_query(int b, int n, int m, int nsample, float radius, int pad, const float *xyz, const float *centres,
                              int64_t *idx, int32_t *cnt, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || m < 0 || n < 1 || nsample < 1) return pcc::invalid("ball_query: bad size");
    if (!(radius > 0.f)) return pcc::invalid("ball_query: radius must be > 0");
    if (pad != PCC_BALL_PAD_FIRST && pad != PCC_BALL_PAD_NONE) return pcc::invalid("ball_query: pad must be 0 (first) or 1 (none)");
    if (b > 65535) return pcc::invalid("ball_query: batch too large");
    if ((long long)b * m > 0x7fffffffLL) return pcc::invalid("ball_query: too many queries (b * m >= 2^31)");
    if (b == 0 || m == 0) return PCC_OK;
    if (!xyz || !centres || !idx) return pcc::invalid("ball_query: null pointer");
    const float r2 = radius * radius;  // one float32 multiplication (-ffp-contract=off)
    const int forced = pcc::tuning(PCC_TUNE_BALL_PATH);  // measurement switch: 1 .. 4 forces a variant
    const int path = forced >= 1 && forced <= kNumPaths ? forced - 1 : kProduct;
    kPaths[path](kNames[path], b, n, m, nsample, r2, pad, xyz, centres, idx, cnt, static_cast<hipStream_t>(stream));
    return pcc::check_launch("ball_query");
}
