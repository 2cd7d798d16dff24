// Local surface geometry along an index list (pcc_local_geometry / pcc_local_covariance_bwd, include/pcc_neighbour.h),
// gfx950, wave64: per row of idx[b,m,k] the mean of the points it names, their scatter matrix, its eigen-decomposition and
// the surface variation -- what get_local_covariance and a batched torch.linalg.eigh compute in a gather, 65 536 small
// matmuls, a cat and a LAPACK-style solve.
//
// The contract fixes the summation order over the slots of a row, so a row is one thread walking its k slots with one set
// of accumulators: the parallelism is across rows.  The index list is nearly all of the traffic (8 k bytes in, at most 100
// bytes out per row), so it is not read row-wise from global memory (one lane: 8 bytes at a stride of 8 k): a workgroup
// stages the contiguous tile of its kRows rows through LDS -- 16-byte loads, range-checked and narrowed to 32 bits on the
// way -- with an odd row stride, so the 64 lanes of a wave, each reading its own row, hit distinct banks.  A row longer than
// kChunk slots is staged kChunk slots at a time.  The cloud is gathered in place (12 n bytes per sample: L2-resident); the
// 3x3 accumulation and the eigen stage (sym3_eigen.hpp) stay in registers.
// The backward is the same walk: per valid slot three float atomics, into LDS bins of the sample where 3 n floats fit
// beside the tile (flushed to the zero-filled grad_xyz with global atomics, so that several workgroups can share a sample),
// straight into global memory otherwise; a lane first sums the run of equal consecutive indices of its row (the padding of
// a PCC_BALL_PAD_FIRST list) in registers.  DESIGN.md section 4i.
#include "chan_block.hpp"
#include "pcc_common.hpp"
#include "sym3_eigen.hpp"

#include <cstdint>

#include "pcc_neighbour.h"

namespace {

using pcc::canonical_nan;
using pcc::v2l;

constexpr int kRows = 256;               // rows of the list per tile = threads per workgroup
constexpr int kChunk = 32;               // slots of a row held in LDS at a time
constexpr int kStride = kChunk + 1;      // words between the rows of a tile: odd
constexpr size_t kBinBytes = 96 * 1024;  // the backward's LDS bins of one sample at the most (12 n bytes: n <= 8192)

// An index outside [0, n) is no point (the -1 of PCC_BALL_PAD_NONE): -1 in the tile.
__device__ __forceinline__ int slot_of(long long raw, int n) { return pcc::in_range(raw, n) ? (int)raw : -1; }

// tile[row][j] = slot c0 + j of row `row`, for the kc slots from c0 of the `nrows` rows at ib (k slots each).  Whole rows
// (kc == k) are one contiguous piece of the list: 16 bytes per lane where the piece is aligned.
__device__ __forceinline__ void stage(int *tile, const int64_t *ib, int nrows, int k, int c0, int kc, int n) {
    const unsigned tid = threadIdx.x, uk = (unsigned)k, ukc = (unsigned)kc;
    if (kc == k && (reinterpret_cast<uintptr_t>(ib) & 15) == 0) {
        const unsigned total = (unsigned)nrows * uk;
        for (unsigned e = tid * 2; e + 1 < total; e += kRows * 2) {
            const v2l two = *reinterpret_cast<const v2l *>(ib + e);
            const unsigned row = e / uk, j = e - row * uk;
            const bool wraps = j + 1 == uk;
            tile[row * kStride + j] = slot_of(two.x, n);
            tile[(wraps ? row + 1 : row) * kStride + (wraps ? 0 : j + 1)] = slot_of(two.y, n);
        }
        if ((total & 1) != 0 && tid == 0) tile[(nrows - 1) * kStride + k - 1] = slot_of(ib[total - 1], n);
    } else {
        const unsigned total = (unsigned)nrows * ukc;
        for (unsigned e = tid; e < total; e += kRows) {
            const unsigned row = e / ukc, j = e - row * ukc;
            tile[row * kStride + j] = slot_of(ib[(size_t)row * uk + c0 + j], n);
        }
    }
}

// f(t) for every valid slot of this thread's row of the tile, in slot order.  Every thread of the workgroup calls it
// (barriers inside).  `resident`: the rows' only chunk is in the tile already (k <= kChunk, after an earlier walk).
template <class F>
__device__ __forceinline__ void walk(int *tile, const int64_t *ib, int nrows, int k, int n, bool resident, F &&f) {
    const int row = threadIdx.x;
    for (int c0 = 0; c0 < k; c0 += kChunk) {
        const int kc = min(kChunk, k - c0);
        if (!resident) {
            __syncthreads();  // (the chunk before has been read)
            stage(tile, ib, nrows, k, c0, kc, n);
            __syncthreads();
        }
        if (row < nrows) {
            for (int j = 0; j < kc; j++) {
                const int t = tile[row * kStride + j];
                if (t >= 0) f(t);
            }
        }
    }
}

// Forward: a tile is kRows consecutive rows of the flattened list [b * m][k]; a thread's sample is its row's.
__global__ __launch_bounds__(kRows) void local_geometry_kernel(int n, int m, int k, long long rows, long long tiles,
                                                               const float *__restrict__ xyz, const int64_t *__restrict__ idx,
                                                               float *__restrict__ mean, float *__restrict__ cov,
                                                               float *__restrict__ eval, float *__restrict__ evec,
                                                               float *__restrict__ curv) {
    __shared__ int tile[kRows * kStride];
    const bool want_eigen = eval || evec || curv, want_cov = cov || want_eigen;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < tiles; u += gridDim.x) {
        const long long r0 = u * kRows, r = r0 + threadIdx.x;
        const int nrows = (int)(rows - r0 < kRows ? rows - r0 : kRows);
        const bool live = (int)threadIdx.x < nrows;
        const int64_t *ib = idx + (size_t)r0 * k;
        const float *cloud = xyz + (size_t)(live ? r / m : 0) * n * 3;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int cnt = 0;
        walk(tile, ib, nrows, k, n, false, [&](int t) {
            const float *p = cloud + (size_t)t * 3;
            sx = sx + p[0];
            sy = sy + p[1];
            sz = sz + p[2];
            cnt++;
        });
        float mx = 0.f, my = 0.f, mz = 0.f;
        if (cnt > 0) {
            const float fc = (float)cnt;
            mx = sx / fc, my = sy / fc, mz = sz / fc;
        }
        if (live && mean) {
            float *o = mean + (size_t)r * 3;
            o[0] = canonical_nan(mx), o[1] = canonical_nan(my), o[2] = canonical_nan(mz);
        }
        if (!want_cov) continue;  // (uniform)
        float c00 = 0.f, c01 = 0.f, c02 = 0.f, c11 = 0.f, c12 = 0.f, c22 = 0.f;
        walk(tile, ib, nrows, k, n, k <= kChunk, [&](int t) {
            const float *p = cloud + (size_t)t * 3;
            const float d0 = p[0] - mx, d1 = p[1] - my, d2 = p[2] - mz;
            c00 = c00 + d0 * d0;
            c01 = c01 + d0 * d1;
            c02 = c02 + d0 * d2;
            c11 = c11 + d1 * d1;
            c12 = c12 + d1 * d2;
            c22 = c22 + d2 * d2;
        });
        if (!live) continue;  // (no barrier is left in this pass)
        if (cov) {
            float *o = cov + (size_t)r * 9;
            const float s00 = canonical_nan(c00), s01 = canonical_nan(c01), s02 = canonical_nan(c02), s11 = canonical_nan(c11),
                        s12 = canonical_nan(c12), s22 = canonical_nan(c22);
            o[0] = s00, o[1] = s01, o[2] = s02;
            o[3] = s01, o[4] = s11, o[5] = s12;
            o[6] = s02, o[7] = s12, o[8] = s22;
        }
        if (want_eigen) {
            const pcc::Eigen3 g = pcc::sym3_eigen(c00, c01, c02, c11, c12, c22);
            if (eval) {
                float *o = eval + (size_t)r * 3;
                o[0] = g.l0, o[1] = g.l1, o[2] = g.l2;
            }
            if (evec) {
                float *o = evec + (size_t)r * 9;
                o[0] = g.x0, o[1] = g.y0, o[2] = g.z0;
                o[3] = g.x1, o[4] = g.y1, o[5] = g.z1;
                o[6] = g.x2, o[7] = g.y2, o[8] = g.z2;
            }
            if (curv) curv[r] = g.curv;
        }
    }
}

// Backward.  Unit u of b * nsplit: rows i0 .. i1 - 1 of sample u / nsplit, tile by tile.  LDS: bins[n][3] of the sample,
// zeroed, added to with ds_add_f32 and flushed into the zero-filled grad_xyz with global atomics (a bin nothing touched adds
// nothing); otherwise every term goes to grad_xyz directly.
template <bool LDS>
__global__ __launch_bounds__(kRows) void local_covariance_bwd_kernel(int n, int m, int k, long long units, int nsplit, unsigned chunk,
                                                                     const float *__restrict__ xyz,
                                                                     const int64_t *__restrict__ idx,
                                                                     const float *__restrict__ mean,
                                                                     const float *__restrict__ grad_cov,
                                                                     const float *__restrict__ grad_mean,
                                                                     float *__restrict__ grad_xyz) {
    __shared__ int tile[kRows * kStride];
    extern __shared__ __attribute__((aligned(16))) float bins[];  // [n][3] (LDS path)
    const int tid = threadIdx.x;
    for (long long u = pcc::xcd_contiguous((int)blockIdx.x, (int)gridDim.x); u < units; u += gridDim.x) {
        const long long smp = u / nsplit;
        const unsigned i0 = (unsigned)(u - smp * nsplit) * chunk, i1 = min((unsigned)m, i0 + chunk);  // (i0 < m: no overflow, m < 2^31)
        const float *cloud = xyz + (size_t)smp * n * 3;
        float *gx = grad_xyz + (size_t)smp * n * 3;
        if (LDS) {
            __syncthreads();  // (the unit before has flushed its bins)
            for (int i = tid; i < 3 * n; i += kRows) bins[i] = 0.f;
            __syncthreads();
        }
        for (unsigned i = i0; i < i1; i += kRows) {
            const int nrows = (int)min((unsigned)kRows, i1 - i);
            const bool live = tid < nrows;
            const size_t r = (size_t)smp * m + i + (live ? tid : 0);
            const int64_t *ib = idx + ((size_t)smp * m + i) * k;
            int cnt = 0;
            if (grad_mean) walk(tile, ib, nrows, k, n, false, [&](int) { cnt++; });
            float mx = 0.f, my = 0.f, mz = 0.f, g00 = 0.f, g01 = 0.f, g02 = 0.f, g11 = 0.f, g12 = 0.f, g22 = 0.f;
            float gm0 = 0.f, gm1 = 0.f, gm2 = 0.f;
            if (live) {
                const float *mp = mean + r * 3, *gc = grad_cov + r * 9;
                mx = mp[0], my = mp[1], mz = mp[2];
                g00 = gc[0] + gc[0], g01 = gc[1] + gc[3], g02 = gc[2] + gc[6];
                g11 = gc[4] + gc[4], g12 = gc[5] + gc[7], g22 = gc[8] + gc[8];
                if (grad_mean && cnt > 0) {
                    const float fc = (float)cnt, *gp = grad_mean + r * 3;
                    gm0 = gp[0] / fc, gm1 = gp[1] / fc, gm2 = gp[2] / fc;
                }
            }
            // the run of equal consecutive indices this lane is in, and the sum of its terms
            int run = -1;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            auto flush = [&]() {
                if (run < 0) return;
                float *dst = gx + (size_t)run * 3;
                if constexpr (LDS) dst = bins + run * 3;
                atomicAdd(dst, a0);
                atomicAdd(dst + 1, a1);
                atomicAdd(dst + 2, a2);
            };
            walk(tile, ib, nrows, k, n, grad_mean != nullptr && k <= kChunk, [&](int t) {
                const float *p = cloud + (size_t)t * 3;
                const float d0 = p[0] - mx, d1 = p[1] - my, d2 = p[2] - mz;
                const float t0 = ((g00 * d0 + g01 * d1) + g02 * d2) + gm0;
                const float t1 = ((g01 * d0 + g11 * d1) + g12 * d2) + gm1;
                const float t2 = ((g02 * d0 + g12 * d1) + g22 * d2) + gm2;
                if (t == run) {
                    a0 += t0, a1 += t1, a2 += t2;
                } else {
                    flush();
                    run = t, a0 = t0, a1 = t1, a2 = t2;
                }
            });
            flush();
        }
        if (LDS) {
            __syncthreads();
            for (int i = tid; i < 3 * n; i += kRows) {
                const float v = bins[i];
                if (v != 0.f) atomicAdd(gx + i, v);
            }
        }
    }
}

int check_sizes(const char *name, int b, int n, int m, int k) {
    pcc::clear_error();
    return pcc::check_list_sizes(name, b, 1, n, m, k);  // (no channels)
}

}  // namespace

extern "C" {

int pcc_local_geometry(int b, int n, int m, int k, const float *xyz, const int64_t *idx, float *mean, float *cov,
                       float *eval, float *evec, float *curv, pcc_stream_t stream) {
    if (int rc = check_sizes("local_geometry", b, n, m, k)) return rc;
    if (b == 0 || m == 0 || (!mean && !cov && !eval && !evec && !curv)) return PCC_OK;
    if (!xyz || !idx) return pcc::invalid("local_geometry: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long rows = (long long)b * m, tiles = (rows + kRows - 1) / kRows;
    pcc::ProfScope prof("local_geometry_kernel", st);
    hipLaunchKernelGGL(local_geometry_kernel, dim3(pcc::grid_for(tiles)), dim3(kRows), 0, st, n, m, k, rows, tiles, xyz, idx, mean, cov,
                       eval, evec, curv);
    return pcc::check_launch("local_geometry");
}

int pcc_local_covariance_bwd(int b, int n, int m, int k, const float *xyz, const int64_t *idx, const float *mean,
                             const float *grad_cov, const float *grad_mean, float *grad_xyz, pcc_stream_t stream) {
    if (int rc = check_sizes("local_covariance_bwd", b, n, m, k)) return rc;
    if (b == 0 || !grad_xyz) return PCC_OK;
    if (m > 0 && (!xyz || !idx || !mean || !grad_cov)) return pcc::invalid("local_covariance_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = pcc::zero_async(grad_xyz, (size_t)b * n * 3 * sizeof(float), st, "local_covariance_bwd: cannot zero grad_xyz")) return rc;
    if (m == 0) return PCC_OK;  // an empty list: nothing points anywhere
    // the rows of a sample go to several workgroups while the call would leave compute units idle: two per unit
    const size_t bin_bytes = (size_t)n * 3 * sizeof(float);
    const long long most = (m + kRows - 1) / kRows;
    long long want = (2LL * pcc::device_cus_or(256) + b - 1) / b;
    want = want < most ? want : most;
    const unsigned chunk = (unsigned)(((m + want - 1) / want + kRows - 1) / kRows * kRows);  // (whole tiles)
    const int nsplit = (int)(((unsigned)m + chunk - 1) / chunk);
    const long long units = (long long)b * nsplit;
    const dim3 grid(pcc::grid_for(units));
    if (bin_bytes <= kBinBytes) {
        pcc::ProfScope prof("local_covariance_bwd_kernel<lds>", st);
        (void)pcc::allow_lds<local_covariance_bwd_kernel<true>>(kBinBytes);
        hipLaunchKernelGGL(local_covariance_bwd_kernel<true>, grid, dim3(kRows), bin_bytes, st, n, m, k, units, nsplit, chunk, xyz, idx,
                           mean, grad_cov, grad_mean, grad_xyz);
    } else {
        pcc::ProfScope prof("local_covariance_bwd_kernel<direct>", st);
        hipLaunchKernelGGL(local_covariance_bwd_kernel<false>, grid, dim3(kRows), 0, st, n, m, k, units, nsplit, chunk, xyz, idx, mean,
                           grad_cov, grad_mean, grad_xyz);
    }
    return pcc::check_launch("local_covariance_bwd");
}

}  // extern "C"
