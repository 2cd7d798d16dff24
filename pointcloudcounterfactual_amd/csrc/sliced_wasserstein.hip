// Sliced Wasserstein distance between paired clouds (pcc_sliced_wasserstein, include/pcc_structural.h), gfx950, wave64:
// per (cloud, direction) slice, project both clouds on the direction, sort the projections, and sum the squared
// differences of equal ranks; the gradient sends every difference back to the point that holds the rank.
//
// One workgroup per (cloud, chunk of PCC_SW_CHUNK consecutive directions), T threads with E elements each, T E >= n a
// power of two (kVariants below).  Thread t owns the points t E .. t E + E - 1 (the element layout of
// lane_major_bitonic), keeps their coordinates of both clouds in registers across the chunk (the 8192-element variant
// re-reads them from global memory: 1024 threads have 128 registers each) and accumulates their gradients there.  Per
// slice:
//   * sort   64-bit keys (order-preserving image of the projection : point index), pads above every real key.  Every wave
//            sorts its run of 64 E keys in registers (lane_major_bitonic); runs are merged by the flip form of the bitonic
//            network -- first step of a merge of runs of kk / 2: element i against i ^ (kk - 1), then i against i ^ j for
//            j = kk / 4 .. 1, the lower element always keeping the smaller key -- whose steps between waves go through LDS
//            (write all, barrier, read the partner; element i sits at word (i % E) T + i / E, so that the lanes of a wave
//            touch consecutive words) and whose steps j < 64 E are lane_major_bitonic_steps.
//   * cost   both clouds sort into the same layout, so the thread that holds rank r of x holds rank r of y: d_r, e_r, and
//            the contract's halving tree over e in LDS (its last six levels are wave_sum_down: the same tree).  A tree
//            over more than the contract's L elements gives the same words: the levels above L add +0 to values >= +0.
//   * grad   the holder of rank r stores d_r at pi_x(r) and -d_r at pi_y(r) of an LDS scratch (plain stores: a
//            permutation cannot collide); after a barrier the owner of point j adds d * theta_c to its three registers.
// The sort buffer, the scratch and the tree share one LDS array of 8 T E bytes.  With more than one chunk the workgroups
// write partial gradient slabs [b, chunks, n, 3] and sw_finish_kernel sums them in ascending chunk order, scales by
// 2 inv and forms cost[b] from cost_p; with one chunk the slice kernel writes the gradients and cost[b] itself.
#include "pcc_common.hpp"
#include "wave_ops.hpp"
#include "wave_sort.hpp"

#include <cstdint>

#include "pcc_test_hooks.h"

namespace {

typedef unsigned long long u64;

constexpr int kChunk = PCC_SW_CHUNK;
constexpr unsigned kNanImage = 0xff800001u;  // one above the image of +inf
constexpr unsigned kPadImage = 0xffffffffu;  // above every real key

// Order-preserving image of a projection: unsigned order of the images = the contract's order of the values.
__device__ __forceinline__ unsigned image_of(float t) {
    const unsigned u = __float_as_uint(t);
    if (t != t) return kNanImage;
    if (u == 0x80000000u) return 0x80000000u;  // -0 counts as +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned img) {
    return __uint_as_float((img & 0x80000000u) ? (img & 0x7fffffffu) : ~img);  // (kNanImage gives a NaN)
}

struct Args {
    int n, p, nchunks;
    const float *x, *y, *theta;
    float *cost, *cost_p;  // cost: written here only when nchunks == 1; cost_p: the caller's, workspace, or null
    float *gx, *gy;        // nchunks == 1: the gradients; otherwise the slabs [b, nchunks, n, 3] (null: not asked for)
    float inv, two_inv;
};

// One compare-exchange step of the merge between waves: element i = i0 + h against i ^ mask; the one whose `bit` is
// clear keeps the smaller key.
template <int T, int E>
__device__ __forceinline__ void lds_step(u64 (&v)[E], u64 *buf, int tid, int mask, int bit) {
    __syncthreads();  // (whoever read buf before is done)
#pragma unroll
    for (int h = 0; h < E; h++) buf[h * T + tid] = v[h];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < E; h++) {
        const int i = tid * E + h, ip = i ^ mask;
        const u64 o = buf[(ip % E) * T + ip / E];
        const bool lower = (i & bit) == 0;
        v[h] = lower == (o < v[h]) ? o : v[h];
    }
}

template <int T, int E, bool GRAD, bool REGS>
__global__ __launch_bounds__(T) void sw_slice_kernel(Args a) {
    constexpr int L = T * E;
    __shared__ __attribute__((aligned(16))) u64 buf[L];
    const int tid = threadIdx.x, lane = tid & 63, i0 = tid * E;
    const int smp = blockIdx.y, chunk = blockIdx.x, n = a.n;
    const float *xb = a.x + (size_t)smp * n * 3, *yb = a.y + (size_t)smp * n * 3;
    const bool want_cost = a.cost_p != nullptr || a.cost != nullptr;

    float px[REGS ? E : 1][3], py[REGS ? E : 1][3];
    if constexpr (REGS) {
#pragma unroll
        for (int h = 0; h < E; h++) {
            const int j = i0 + h;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                px[h][c] = j < n ? xb[(size_t)j * 3 + c] : 0.f;
                py[h][c] = j < n ? yb[(size_t)j * 3 + c] : 0.f;
            }
        }
    }
    float gx[GRAD ? E : 1][3], gy[GRAD ? E : 1][3];
    if constexpr (GRAD) {
#pragma unroll
        for (int h = 0; h < E; h++)
#pragma unroll
            for (int c = 0; c < 3; c++) gx[h][c] = gy[h][c] = 0.f;
    }

    (void)px, (void)py, (void)gx, (void)gy;

    const int p0 = chunk * kChunk, p1 = min(a.p, p0 + kChunk);
    float chain = 0.f;  // (thread 0) the cost chain, nchunks == 1
    for (int pi = p0; pi < p1; pi++) {
        const float th0 = a.theta[(size_t)pi * 3], th1 = a.theta[(size_t)pi * 3 + 1], th2 = a.theta[(size_t)pi * 3 + 2];
        u64 ka[E], v[E];
        for (int cloud = 0; cloud < 2; cloud++) {
            if (cloud) {
#pragma unroll
                for (int h = 0; h < E; h++) ka[h] = v[h];
            }
#pragma unroll
            for (int h = 0; h < E; h++) {
                const int j = i0 + h;
                unsigned img = kPadImage;
                if (j < n) {
                    float v0, v1, v2;
                    if constexpr (REGS) {
                        v0 = cloud ? py[h][0] : px[h][0];
                        v1 = cloud ? py[h][1] : px[h][1];
                        v2 = cloud ? py[h][2] : px[h][2];
                    } else {
                        const float *q = (cloud ? yb : xb) + (size_t)j * 3;
                        v0 = q[0], v1 = q[1], v2 = q[2];
                    }
                    img = image_of((v0 * th0 + v1 * th1) + v2 * th2);
                }
                v[h] = ((u64)img << 32) | (unsigned)j;
            }
            pcc::lane_major_bitonic(v, lane);
            if constexpr (T > 64) {
#pragma unroll 1
                for (int kk = 128 * E; kk <= L; kk <<= 1) {
                    lds_step<T>(v, buf, tid, kk - 1, kk >> 1);
#pragma unroll 1
                    for (int j = kk >> 2; j >= 64 * E; j >>= 1) lds_step<T>(v, buf, tid, j, j);
                    pcc::lane_major_bitonic_steps(v, lane, 0, 32 * E);
                }
            }
        }
        // rank r = i0 + h: ka[h] = (a_r, pi_x(r)), v[h] = (b_r, pi_y(r))
        float d[E];
#pragma unroll
        for (int h = 0; h < E; h++) d[h] = value_of((unsigned)(ka[h] >> 32)) - value_of((unsigned)(v[h] >> 32));
        if constexpr (GRAD) {
            float *sx = reinterpret_cast<float *>(buf), *sy = sx + L;
            __syncthreads();  // (the sort's last reads of buf)
#pragma unroll
            for (int h = 0; h < E; h++) {
                if (i0 + h < n) {
                    sx[(unsigned)ka[h]] = d[h];
                    sy[(unsigned)v[h]] = -d[h];
                }
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < E; h++) {
                const int j = i0 + h;
                if (j < n) {
                    const float dx = sx[j], dy = sy[j];
                    gx[h][0] = gx[h][0] + dx * th0, gx[h][1] = gx[h][1] + dx * th1, gx[h][2] = gx[h][2] + dx * th2;
                    gy[h][0] = gy[h][0] + dy * th0, gy[h][1] = gy[h][1] + dy * th1, gy[h][2] = gy[h][2] + dy * th2;
                }
            }
        }
        if (want_cost) {
            float *e = reinterpret_cast<float *>(buf);
            __syncthreads();  // (the sort's, or the scratch's, last reads of buf)
            // (volatile: word by word.  hipcc 7.2 merges the E selected values into one wide LDS store and then dies in
            // instruction selection, SIInstrInfo::legalizeOperandsVOP3.)
#pragma unroll
            for (int h = 0; h < E; h++) *(volatile float *)&e[i0 + h] = i0 + h < n ? d[h] * d[h] : 0.f;
#pragma unroll 1
            for (int hh = L / 2; hh >= 64; hh >>= 1) {
                __syncthreads();
                for (int i = tid; i < hh; i += T) e[i] = e[i] + e[i + hh];
            }
            __syncthreads();
            if (tid < 64) {
                const float c = pcc::wave_sum_down(e[tid]);  // levels 32 .. 1 of the same tree, e_0 in lane 0
                if (tid == 0) {
                    if (a.cost_p) a.cost_p[(size_t)smp * a.p + pi] = c;
                    chain = pi == p0 ? c : chain + c;
                }
            }
        }
    }
    if (a.nchunks == 1 && a.cost && tid == 0) a.cost[smp] = chain * a.inv;
    if constexpr (GRAD) {
        const bool direct = a.nchunks == 1;
        const size_t base = direct ? (size_t)smp * n * 3 : ((size_t)smp * a.nchunks + chunk) * n * 3;
        const float s = direct ? a.two_inv : 1.f;
#pragma unroll
        for (int h = 0; h < E; h++) {
            const int j = i0 + h;
            if (j < n) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (a.gx) a.gx[base + (size_t)j * 3 + c] = direct ? gx[h][c] * s : gx[h][c];
                    if (a.gy) a.gy[base + (size_t)j * 3 + c] = direct ? gy[h][c] * s : gy[h][c];
                }
            }
        }
    }
}

// nchunks > 1.  Block (x, smp): words x 256 .. of the cloud's 3 n gradient words, each the slabs' sum in ascending chunk
// order times 2 inv; thread 0 of block (0, smp) forms cost[smp] from cost_p[smp, :] in ascending p.
__global__ __launch_bounds__(256) void sw_finish_kernel(int n, int p, int nchunks, const float *__restrict__ slab_x,
                                                        const float *__restrict__ slab_y, const float *__restrict__ cost_p,
                                                        float *__restrict__ grad_x, float *__restrict__ grad_y,
                                                        float *__restrict__ cost, float inv, float two_inv) {
    const int smp = blockIdx.y;
    const size_t words = (size_t)n * 3;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w < words) {
        if (grad_x) {
            const float *s = slab_x + (size_t)smp * nchunks * words + w;
            float acc = s[0];
            for (int k = 1; k < nchunks; k++) acc = acc + s[(size_t)k * words];
            grad_x[(size_t)smp * words + w] = acc * two_inv;
        }
        if (grad_y) {
            const float *s = slab_y + (size_t)smp * nchunks * words + w;
            float acc = s[0];
            for (int k = 1; k < nchunks; k++) acc = acc + s[(size_t)k * words];
            grad_y[(size_t)smp * words + w] = acc * two_inv;
        }
    }
    if (cost && blockIdx.x == 0 && threadIdx.x == 0) {
        const float *c = cost_p + (size_t)smp * p;
        float acc = c[0];
        for (int k = 1; k < p; k++) acc = acc + c[k];
        cost[smp] = acc * inv;
    }
}

template <int T, int E, bool REGS>
void launch_slices(const char *name, int b, bool grad, const Args &a, hipStream_t st) {
    pcc::ProfScope prof(name, st);
    const dim3 grid((unsigned)a.nchunks, (unsigned)b), block(T);
    if (grad) hipLaunchKernelGGL((sw_slice_kernel<T, E, true, REGS>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((sw_slice_kernel<T, E, false, REGS>), grid, block, 0, st, a);
}

// The variants (threads, elements per thread): value v of the sw_path switch forces kVariants[v - 1] where it holds n.  The
// product takes the first one that holds the cloud.  All of them return the same words.
struct Variant {
    int capacity;
    void (*launch)(const char *, int, bool, const Args &, hipStream_t);
    const char *name;  // the launch profile's: the instantiation, <threads,elements per thread>
};
const Variant kVariants[] = {{64, launch_slices<64, 1, true>, "sw_slice_kernel<64,1>"},
                             {128, launch_slices<64, 2, true>, "sw_slice_kernel<64,2>"},
                             {256, launch_slices<64, 4, true>, "sw_slice_kernel<64,4>"},
                             {512, launch_slices<128, 4, true>, "sw_slice_kernel<128,4>"},
                             {1024, launch_slices<256, 4, true>, "sw_slice_kernel<256,4>"},
                             {2048, launch_slices<512, 4, true>, "sw_slice_kernel<512,4>"},
                             {4096, launch_slices<1024, 4, true>, "sw_slice_kernel<1024,4>"},
                             {8192, launch_slices<1024, 8, false>, "sw_slice_kernel<1024,8>"},
                             {2048, launch_slices<256, 8, true>, "sw_slice_kernel<256,8>"},
                             {4096, launch_slices<512, 8, true>, "sw_slice_kernel<512,8>"}};
constexpr int kNumVariants = (int)(sizeof kVariants / sizeof kVariants[0]);
static_assert(PCC_SW_MAX_N == 8192, "the largest variant holds PCC_SW_MAX_N elements");

}  // namespace

extern "C" int pcc_sliced_wasserstein(int b, int n, int p, const float *x, const float *y, const float *theta, float *cost,
                                      float *cost_p, float *grad_x, float *grad_y, pcc_stream_t stream) {
    pcc::clear_error();
    if (b < 0 || n < 1 || p < 1) return pcc::invalid("sliced_wasserstein: bad size");
    if (n > PCC_SW_MAX_N) return pcc::invalid("sliced_wasserstein: cloud too large (n > PCC_SW_MAX_N)");
    if (b > 65535) return pcc::invalid("sliced_wasserstein: batch too large");
    if ((long long)b * p > 0x7fffffffLL) return pcc::invalid("sliced_wasserstein: too many slices (b * p >= 2^31)");
    if (b == 0) return PCC_OK;
    if (!x || !y || !theta) return pcc::invalid("sliced_wasserstein: null pointer");
    if (!cost && !cost_p && !grad_x && !grad_y) return PCC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool grad = grad_x || grad_y;
    const float inv = (float)(1.0 / ((double)n * (double)p));
    Args a{n, p, pcc::ceil_div(p, kChunk), x, y, theta, cost, cost_p, grad_x, grad_y, inv, 2.f * inv};
    const bool finish = a.nchunks > 1 && (grad || cost);
    const size_t slab = (size_t)b * a.nchunks * n * 3;  // words of one cloud's partial gradients
    pcc::WsBlock ws(st);
    if (finish) {
        const size_t words = (grad_x ? slab : 0) + (grad_y ? slab : 0) + (cost && !cost_p ? (size_t)b * p : 0);
        float *w = nullptr;
        if (words) {
            if (int rc = ws.alloc(words * sizeof(float), "sliced_wasserstein: workspace allocation failed")) return rc;
            w = static_cast<float *>(ws.p);
        }
        if (grad_x) a.gx = w, w += slab;
        if (grad_y) a.gy = w, w += slab;
        if (cost && !cost_p) a.cost_p = w;
        a.cost = nullptr;  // (sw_finish_kernel's)
    }
    const int forced = pcc::tuning(PCC_TUNE_SW_PATH);  // measurement switch: 1 .. kNumVariants forces a variant that holds n
    int path = 0;
    while (kVariants[path].capacity < n) ++path;
    if (forced >= 1 && forced <= kNumVariants && kVariants[forced - 1].capacity >= n) path = forced - 1;
    kVariants[path].launch(kVariants[path].name, b, grad, a, st);
    if (int rc = pcc::check_launch("sliced_wasserstein")) return rc;
    if (finish) {
        pcc::ProfScope prof("sw_finish_kernel", st);
        const unsigned gx = grad ? (unsigned)pcc::ceil_div(n * 3, 256) : 1u;
        hipLaunchKernelGGL(sw_finish_kernel, dim3(gx, (unsigned)b), dim3(256), 0, st, n, p, a.nchunks, grad_x ? a.gx : nullptr,
                           grad_y ? a.gy : nullptr, a.cost_p, grad_x, grad_y, cost, inv, a.two_inv);
        return pcc::check_launch("sliced_wasserstein(finish)");
    }
    return PCC_OK;
}
