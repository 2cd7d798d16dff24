// Voxel occupancy counts of a bank of clouds (pcc_occupancy_grid, include/pcc_structural.h), gfx950, wave64.
//
// A histogram with integer atomics: every finite point adds 1 to the bin of its cell, so the counts are the same for
// every schedule, grid size and path (integer adds commute).  The cell rule is the header's; cell_of() is its one copy.
//   * occ_lds_kernel<PER_CLOUD>: res^3 * 4 bytes fit the workgroup's LDS (res <= 32).  A workgroup zeroes a private
//     histogram in LDS, walks its slab of points with coalesced loads and adds with ds_add_u32.  Set mode: the slabs are
//     sized so that at most one workgroup per CU runs and each has kSlabPoints points or more; the non-zero bins are
//     flushed with one global atomic each.  Per-cloud mode: one workgroup owns one cloud and stores its whole row.
//   * occ_global_kernel: any res; one global atomic per point into zeroed counts.
//   * occ_fallback_kernel (in_sphere only): the points whose separable cell lies outside the inscribed sphere were
//     appended to a compact list by the kernels above (one counter add per wave, defer()); one wave per listed point scans
//     the res^2 columns (i, j) -- lane l takes columns l, l + 64, ... -- with the in-sphere interval of every column in
//     LDS, and the wave's minimum of (distance bits, flat index) is the cell.  Its adds are global atomics on the same
//     counts, behind the main kernel in stream order.
#include <algorithm>
#include <climits>
#include <cmath>

#include "pcc_common.hpp"
#include "pcc_test_hooks.h"
#include "wave_ops.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kLdsBlock = 1024;          // threads of occ_lds_kernel: one workgroup per CU, every wave slot of it
constexpr int kGlobalBlock = 256;        // threads of occ_global_kernel
constexpr int kFallbackBlock = 256;      // threads of occ_fallback_kernel: 4 points in flight per workgroup
constexpr int kLdsBudget = 128 * 1024;   // histogram bytes of the LDS path: res <= 32
constexpr int kSlabPoints = 4096;        // set mode, LDS path: fewest points per workgroup (zeroing and flushing res^3 bins
                                         // must stay small beside the slab)
constexpr int kEmptyColumn = 255;        // klo of a column without an in-sphere grid point (res <= 128: klo <= 64)

struct Grid {
    int res, in_sphere;
    float lo, inv, step, top;  // inv = (res - 1) / extent, step = extent / (res - 1), top = res - 1
};

// nearest grid index on one axis: the rule pcc_voxel_index shares
__device__ __forceinline__ int axis_cell(float x, const Grid &g) { return pcc::axis_cell(x, g.lo, g.inv, g.top); }

__device__ __forceinline__ bool in_sphere(int i, int j, int k, int r1) {
    const int a = 2 * i - r1, b = 2 * j - r1, c = 2 * k - r1;
    return a * a + b * b + c * c <= r1 * r1;
}

// Flat cell of point p, or -1 for a point that is counted nowhere here: past the end, non-finite, or `deferred` to the
// fallback pass.
__device__ __forceinline__ int cell_of(const float *__restrict__ xyz, unsigned p, bool active, const Grid &g, bool &deferred) {
    deferred = false;
    if (!active) return -1;
    const float x = xyz[(size_t)p * 3], y = xyz[(size_t)p * 3 + 1], z = xyz[(size_t)p * 3 + 2];
    if (!pcc::finite3(x, y, z)) return -1;
    const int i = axis_cell(x, g), j = axis_cell(y, g), k = axis_cell(z, g);
    if (g.in_sphere && !in_sphere(i, j, k, g.res - 1)) {
        deferred = true;
        return -1;
    }
    return (i * g.res + j) * g.res + k;
}

// Appends p of every lane that wants it to the list: one counter add per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void defer(bool want, unsigned p, int *__restrict__ list, unsigned *__restrict__ list_n) {
    const u64 mask = __ballot(want);
    if (!mask) return;
    const int lane = threadIdx.x & 63, leader = __ffsll(mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(list_n, (unsigned)__popcll(mask));
    base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
    if (want) list[base + (unsigned)pcc::lanes_below(mask)] = (int)p;
}

template <bool PER_CLOUD>
__global__ __launch_bounds__(kLdsBlock) void occ_lds_kernel(int n, int total, int slab, const float *__restrict__ xyz, Grid g,
                                                            int32_t *__restrict__ counts, int *__restrict__ list,
                                                            unsigned *__restrict__ list_n) {
    extern __shared__ __attribute__((aligned(16))) int hist[];
    const unsigned tid = threadIdx.x;
    const int bins = g.res * g.res * g.res;
    for (int b = tid; b < bins; b += kLdsBlock) hist[b] = 0;
    __syncthreads();
    // this workgroup's points [first, last): one cloud, or one slab of the bank (total <= INT_MAX: no wrap in 32 bits)
    const unsigned first = blockIdx.x * (unsigned)(PER_CLOUD ? n : slab);
    const unsigned last = PER_CLOUD ? first + (unsigned)n : min((unsigned)total, first + (unsigned)slab);
    for (unsigned base = first; base < last; base += kLdsBlock) {
        const unsigned p = base + tid;
        bool deferred;
        const int flat = cell_of(xyz, p, p < last, g, deferred);
        if (flat >= 0) atomicAdd(&hist[flat], 1);
        if (g.in_sphere) defer(deferred, p, list, list_n);
    }
    __syncthreads();
    if (PER_CLOUD) {
        int32_t *row = counts + (size_t)blockIdx.x * bins;
        for (int b = tid; b < bins; b += kLdsBlock) row[b] = hist[b];
    } else {
        for (int b = tid; b < bins; b += kLdsBlock)
            if (const int v = hist[b]) atomicAdd(&counts[b], v);
    }
}

__global__ __launch_bounds__(kGlobalBlock) void occ_global_kernel(int n, int total, int per_cloud, const float *__restrict__ xyz,
                                                                  Grid g, int32_t *__restrict__ counts, int *__restrict__ list,
                                                                  unsigned *__restrict__ list_n) {
    const int bins = g.res * g.res * g.res;
    const unsigned stride = gridDim.x * kGlobalBlock;
    for (unsigned base = blockIdx.x * kGlobalBlock; base < (unsigned)total; base += stride) {
        const unsigned p = base + threadIdx.x;
        bool deferred;
        const int flat = cell_of(xyz, p, p < (unsigned)total, g, deferred);
        if (flat >= 0) atomicAdd(&counts[(per_cloud ? (size_t)(p / (unsigned)n) * bins : 0) + flat], 1);
        if (g.in_sphere) defer(deferred, p, list, list_n);
    }
}

__global__ __launch_bounds__(kFallbackBlock) void occ_fallback_kernel(int n, int per_cloud, const float *__restrict__ xyz, Grid g,
                                                                      int32_t *__restrict__ counts, const int *__restrict__ list,
                                                                      const unsigned *__restrict__ list_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char klo[];  // [res][res]; the interval is [klo, res - 1 - klo]
    const int res = g.res, r1 = res - 1, cols = res * res;
    for (int c = threadIdx.x; c < cols; c += kFallbackBlock) {
        const int i = c / res, j = c - i * res;
        const int a = 2 * i - r1, b = 2 * j - r1, rem = r1 * r1 - a * a - b * b;  // (2k - r1)^2 <= rem
        int l = kEmptyColumn;
        if (rem >= 0) {
            int m = (int)sqrtf((float)rem);  // floor(sqrt(rem)), settled in integers
            while (m * m > rem) --m;
            while ((m + 1) * (m + 1) <= rem) ++m;
            const int first = (res - m) >> 1;  // ceil((r1 - m) / 2)
            if (first <= r1 - first) l = first;
        }
        klo[c] = (unsigned char)l;
    }
    __syncthreads();
    const unsigned count = *list_n;
    const int lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * (kFallbackBlock / 64);
    const int bins = cols * res;
    for (unsigned e = blockIdx.x * (kFallbackBlock / 64) + (threadIdx.x >> 6); e < count; e += waves) {
        const unsigned p = (unsigned)list[e];
        const float px = xyz[(size_t)p * 3], py = xyz[(size_t)p * 3 + 1], pz = xyz[(size_t)p * 3 + 2];
        const int ks = axis_cell(pz, g);
        u64 best = 0;  // the maximum of ~(distance bits, flat index): lowest distance, then lowest index
        for (int c = lane; c < cols; c += 64) {
            const int l = klo[c];
            if (l == kEmptyColumn) continue;
            const int i = c / res, j = c - i * res;
            const int k = min(max(ks, l), r1 - l);  // the distance is convex in k: the clamp is the column's best
            const float gx = (float)i * g.step + g.lo, gy = (float)j * g.step + g.lo, gz = (float)k * g.step + g.lo;
            const float d = pcc::sq3(px - gx, py - gy, pz - gz);  // >= +0, so its bits order as an unsigned integer
            best = pcc::max_u64(best, ~(((u64)__float_as_uint(d) << 32) | (unsigned)(c * res + k)));
        }
        best = pcc::wave_max_u64(best);
        if (lane == 0 && best) atomicAdd(&counts[(per_cloud ? (size_t)(p / (unsigned)n) * bins : 0) + (unsigned)~best], 1);
    }
}

template <bool PER_CLOUD>
int launch_lds(int blocks, int n, int total, int slab, const float *xyz, const Grid &g, int32_t *counts, int *list, unsigned *list_n,
               hipStream_t st) {
    if (const hipError_t attr = pcc::allow_lds<occ_lds_kernel<PER_CLOUD>>(kLdsBudget)) {
        pcc::set_error((int)attr, "occupancy_grid: cannot reserve the histogram's LDS");
        return (int)attr;
    }
    const size_t lds = (size_t)g.res * g.res * g.res * sizeof(int);
    pcc::ProfScope prof(PER_CLOUD ? "occ_lds_kernel(per cloud)" : "occ_lds_kernel(set)", st);
    hipLaunchKernelGGL((occ_lds_kernel<PER_CLOUD>), dim3((unsigned)blocks), dim3(kLdsBlock), lds, st, n, total, slab, xyz, g, counts,
                       list, list_n);
    return pcc::check_launch("occupancy_grid(LDS path)");
}

}  // namespace

extern "C" int pcc_occupancy_grid(int s, int n, const float *xyz, int res, float lo, float extent, int in_sphere, int per_cloud,
                                  int32_t *counts, pcc_stream_t stream) {
    pcc::clear_error();
    if (s < 0) return pcc::invalid("occupancy_grid: s must be >= 0");
    if (n < 1) return pcc::invalid("occupancy_grid: n must be >= 1");
    if (res < 2 || res > 128) return pcc::invalid("occupancy_grid: res must be in [2, 128]");
    if (in_sphere && res < 3) return pcc::invalid("occupancy_grid: in_sphere needs res >= 3");
    Grid g;
    g.res = res, g.in_sphere = in_sphere != 0;
    g.lo = lo, g.top = (float)(res - 1);
    g.inv = g.top / extent, g.step = extent / g.top;
    // (an extent so small or so large that 1 / step or step itself is not a positive finite float is refused with it)
    if (!(extent > 0.f) || !std::isfinite(extent) || !std::isfinite(g.inv) || !(g.step > 0.f) || !(g.inv > 0.f))
        return pcc::invalid("occupancy_grid: extent must be finite and > 0");
    if (!std::isfinite(lo)) return pcc::invalid("occupancy_grid: lo must be finite");
    if (s == 0) return PCC_OK;
    if ((long long)s * n > INT_MAX) return pcc::invalid("occupancy_grid: too many points (s * n > INT_MAX)");
    const int bins = res * res * res;
    if (per_cloud && (long long)s * bins > INT_MAX)
        return pcc::invalid("occupancy_grid: per-cloud output too large (s * res^3 > INT_MAX)");
    if (!xyz || !counts) return pcc::invalid("occupancy_grid: null pointer");

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int total = s * n;
    const int forced = pcc::tuning(PCC_TUNE_OCCUPANCY_PATH);  // measurement switch: 1 = global path, 2 = LDS path where it fits
    const bool lds_path = (size_t)bins * sizeof(int) <= (size_t)kLdsBudget && forced != 1;
    const int cus = pcc::device_cus_or(256);

    // in_sphere: [0] the length of the list of deferred points, [4 ..] the list (every point may be on it)
    pcc::WsBlock ws(st);
    int *list = nullptr;
    unsigned *list_n = nullptr;
    if (g.in_sphere) {
        if (int rc = ws.alloc(((size_t)total + 4) * sizeof(int), "occupancy_grid: workspace allocation failed")) return rc;
        list_n = static_cast<unsigned *>(ws.p);
        list = static_cast<int *>(ws.p) + 4;
        if (int rc = pcc::zero_async(list_n, sizeof(unsigned), st, "occupancy_grid: cannot zero the list counter")) return rc;
    }
    // the per-cloud LDS kernel stores every bin of every row; everything else adds into zeroed counts
    if (!(lds_path && per_cloud))
        if (int rc = pcc::zero_async(counts, (size_t)(per_cloud ? s : 1) * bins * sizeof(int32_t), st, "occupancy_grid: cannot zero counts"))
            return rc;

    if (lds_path && per_cloud) {
        if (int rc = launch_lds<true>(s, n, total, 0, xyz, g, counts, list, list_n, st)) return rc;
    } else if (lds_path) {
        int blocks = std::max(1, std::min(cus, pcc::ceil_div(total, kSlabPoints)));
        const int slab = pcc::ceil_div(pcc::ceil_div(total, blocks), kLdsBlock) * kLdsBlock;  // (<= total + 1023 * 2: no wrap, see `first`)
        blocks = pcc::ceil_div(total, slab);
        if (int rc = launch_lds<false>(blocks, n, total, slab, xyz, g, counts, list, list_n, st)) return rc;
    } else {
        const int blocks = std::max(1, std::min(cus * 8, pcc::ceil_div(total, kGlobalBlock)));
        pcc::ProfScope prof("occ_global_kernel", st);
        hipLaunchKernelGGL(occ_global_kernel, dim3((unsigned)blocks), dim3(kGlobalBlock), 0, st, n, total, per_cloud, xyz, g, counts, list,
                           list_n);
        if (int rc = pcc::check_launch("occupancy_grid(global path)")) return rc;
    }
    if (g.in_sphere) {
        const int blocks = std::max(1, std::min(cus * 8, pcc::ceil_div(total, kFallbackBlock / 64)));
        const size_t lds = ((size_t)res * res + 15) / 16 * 16;
        pcc::ProfScope prof("occ_fallback_kernel", st);
        hipLaunchKernelGGL(occ_fallback_kernel, dim3((unsigned)blocks), dim3(kFallbackBlock), lds, st, n, per_cloud, xyz, g, counts, list,
                           list_n);
        if (int rc = pcc::check_launch("occupancy_grid(fallback pass)")) return rc;
    }
    return PCC_OK;
}
