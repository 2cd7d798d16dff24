// The kernel map of a submanifold sparse convolution over a ragged grid level (pcc_cell_neighbours_ragged,
// include/pcc_neighbour.h), gfx950, wave64: for every slot of coord[m, 4] = (cloud, i, j, k) -- pcc_grid_cluster_ragged's,
// ascending by (cloud, i, j, k) -- the rank of the slot at each of the ksize^3 offsets, -1 where there is none.  Integers only,
// nothing is atomic, every word is written once, one launch, no workspace.
//   * cell_map_ragged<KSIZE> (the function cell_map_ragged_kernel): sparse_conv.hip's map kernel, restated for a list that
//     does not fit LDS.  A thread owns a row of taps -- one (slot, di, dj) and the KSIZE offsets along dk -- and stores its
//     KSIZE words side by side, so consecutive threads store consecutive 24- or 40-byte pieces; a workgroup owns kMapThreads
//     consecutive rows (a scene level has too few slots to fill the device with 256 of them per workgroup, and a thread that
//     walks several rows one after the other only waits longer: DESIGN.md 4x has both measured).  The sorted list is coord
//     itself, in global memory (16 bytes per slot: a scene level is a few MB and stays in L2), compared as the 64-bit key
//     (c << 48 | i << 32 | j << 16 | k) formed on the fly from masked components.  A row is one 16-byte load where coord lies
//     on a 16-byte boundary and four dword loads otherwise (one uniform branch).
//     The slot's row is decomposed and range-tested in 32-bit integers BEFORE anything is packed: a source component outside
//     [0, 65536) gives a row of -1, a target component outside it a -1, so no carry crosses a field of the key.
//     The first target of a row is found by bisection over [0, kept).  Its first kTreeLevels levels probe positions that
//     depend on kept alone, so every workgroup first copies those keys to LDS (thread = node of the tree in heap order) and
//     the search walks them there; the levels below read global memory.  On the centre row (di = dj = 0) the first target
//     lies no further than h * dilation entries before r, because the cells are distinct and ascending: that window is
//     searched instead.  Every later target lies at most `dilation` entries behind the last bound.  <= 32 halvings each; every
//     position read is in [0, kept), whatever coord holds.
#include <climits>
#include <cstdint>

#include "pcc_common.hpp"
#include "pcc_neighbour.h"

namespace {

typedef unsigned long long u64;

constexpr int kMapThreads = 256;   // threads, and rows of taps, of a workgroup: four waves
constexpr int kAxisCells = 65536;  // cells per axis, and clouds, a field of the key holds (pcc_grid_cluster_ragged: axis_bits <= 16)
constexpr int kTreeLevels = 8;     // levels of the bisection over [0, kept) a workgroup keeps in LDS (10 and 11 measured slower)
constexpr int kTreeNodes = 1 << kTreeLevels;  // heap order: node 1 is the root, node 0 is unused; one node per thread

// The key of the slot at `pos` (the caller keeps pos inside [0, kept)).  The components of the library's coord are inside
// their fields already; the masks keep anything else from spilling into a neighbouring field.
__device__ __forceinline__ u64 slot_key(const int32_t *__restrict__ coord, int pos, bool wide) {
    int c, i, j, k;
    if (wide) {
        const int4 v = *reinterpret_cast<const int4 *>(coord + (size_t)pos * 4);
        c = v.x, i = v.y, j = v.z, k = v.w;
    } else {
        const int32_t *p = coord + (size_t)pos * 4;
        c = p[0], i = p[1], j = p[2], k = p[3];
    }
    return ((u64)(c & 0xffff) << 48) | ((u64)(i & 0xffff) << 32) | ((u64)(j & 0xffff) << 16) | (u64)(k & 0xffff);
}

// The first position of [lo, hi) whose key is >= want (hi: none).  0 <= lo <= hi <= kept < 2^31: 31 halvings at the most.
__device__ __forceinline__ int lower_bound(const int32_t *__restrict__ coord, bool wide, int lo, int hi, u64 want) {
    for (int s = 0; s < 32 && lo < hi; s++) {
        const int mid = lo + ((hi - lo) >> 1);
        if (slot_key(coord, mid, wide) < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int KSIZE>
__global__ __launch_bounds__(kMapThreads) void cell_map_ragged_kernel(int m, int dil, const int32_t *__restrict__ coord,
                                                                      const int32_t *__restrict__ n_cells, int64_t *__restrict__ nbr) {
    constexpr int h = (KSIZE - 1) / 2, rows = KSIZE * KSIZE;
    __shared__ u64 tree[kTreeNodes];
    const int kept = min(max(n_cells[0], 0), m);
    const bool wide = (reinterpret_cast<uintptr_t>(coord) & 15u) == 0;  // (the same in every thread)
    // thread = node: the interval lower_bound(0, kept) has when it arrives at the node (the bits of the node below its leading
    // one are the turns taken from the root: 1 = right), and the key it probes there
    for (int node = threadIdx.x; node < kTreeNodes; node += kMapThreads) {
        int lo = 0, hi = kept, depth = 0;
        for (int v = node; v > 1; v >>= 1) depth++;
        for (int s = depth - 1; s >= 0 && lo < hi; s--) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((node >> s) & 1) lo = mid + 1;
            else hi = mid;
        }
        tree[node] = node >= 1 && lo < hi ? slot_key(coord, lo + ((hi - lo) >> 1), wide) : 0ull;
    }
    __syncthreads();
    const long long item = (long long)blockIdx.x * kMapThreads + threadIdx.x;  // (slot, di, dj), slot-major
    if (item >= (long long)m * rows) return;
    const int r = (int)(item / rows), row = (int)(item % rows);
    const int di = row / KSIZE - h, dj = row % KSIZE - h;
    int64_t *dst = nbr + (size_t)item * KSIZE;
    int c = -1, i = -1, j = -1, k = -1;
    if (r < kept) {
        if (wide) {
            const int4 v = *reinterpret_cast<const int4 *>(coord + (size_t)r * 4);
            c = v.x, i = v.y, j = v.z, k = v.w;
        } else {
            const int32_t *p = coord + (size_t)r * 4;
            c = p[0], i = p[1], j = p[2], k = p[3];
        }
    }
    // the source inside its fields first (so that the sums below stay far inside an int: dil <= 65536), then the target
    const bool source = (unsigned)c < (unsigned)kAxisCells && (unsigned)i < (unsigned)kAxisCells && (unsigned)j < (unsigned)kAxisCells &&
                        (unsigned)k < (unsigned)kAxisCells;
    const int ti = i + dil * di, tj = j + dil * dj, k0 = k - dil * h;
    if (!source || (unsigned)ti >= (unsigned)kAxisCells || (unsigned)tj >= (unsigned)kAxisCells) {
#pragma unroll
        for (int u = 0; u < KSIZE; u++) dst[u] = -1;
        return;
    }
    const u64 base = ((u64)(unsigned)c << 48) | ((u64)(unsigned)ti << 32) | ((u64)(unsigned)tj << 16);
    const bool centre = di == 0 && dj == 0;
    int pos = 0;  // the first entry of the list that is >= the last target looked for
    bool first = true;
#pragma unroll
    for (int u = 0; u < KSIZE; u++) {
        const int tk = k0 + u * dil;
        int64_t found = -1;
        if ((unsigned)tk < (unsigned)kAxisCells) {
            const u64 want = base | (u64)(unsigned)tk;
            int lo, hi;
            if (!first) {
                lo = pos, hi = (int)min((long long)pos + dil, (long long)kept);
            } else if (centre) {  // a cell of the slot's own line, at or before it
                lo = (int)max((long long)r - (long long)h * dil, 0ll), hi = r + 1;
            } else {              // the top of the bisection over the whole list, from LDS
                lo = 0, hi = kept;
                int node = 1;
                for (int s = 0; s < kTreeLevels && lo < hi; s++) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (tree[node] < want) lo = mid + 1, node = 2 * node + 1;
                    else hi = mid, node = 2 * node;
                }
            }
            pos = lower_bound(coord, wide, lo, hi, want);
            first = false;
            if (pos < kept && slot_key(coord, pos, wide) == want) found = pos;
        }
        dst[u] = found;
    }
}

template <int KSIZE>
void launch_map(int m, int dil, const int32_t *coord, const int32_t *n_cells, int64_t *nbr, hipStream_t st) {
    pcc::ProfScope prof(KSIZE == 3 ? "cell_map_ragged<3>" : "cell_map_ragged<5>", st);
    const unsigned blocks = (unsigned)(((long long)m * KSIZE * KSIZE + kMapThreads - 1) / kMapThreads);
    hipLaunchKernelGGL(cell_map_ragged_kernel<KSIZE>, dim3(blocks), dim3(kMapThreads), 0, st, m, dil, coord, n_cells, nbr);
}

}  // namespace

extern "C" int pcc_cell_neighbours_ragged(int m, int ksize, int dilation, const int32_t *coord, const int32_t *n_cells, int64_t *nbr,
                                          pcc_stream_t stream) {
    const char *name = "cell_neighbours_ragged";
    pcc::clear_error();
    if (m < 1) return pcc::invalidf("%s: m must be >= 1", name);
    if (ksize != 3 && ksize != 5) return pcc::invalidf("%s: ksize must be 3 or 5", name);
    if (dilation < 1) return pcc::invalidf("%s: dilation must be >= 1", name);
    if ((long long)m * ksize * ksize * ksize > INT_MAX) return pcc::invalidf("%s: map too large (m * ksize^3 >= 2^31)", name);
    if (!coord || !n_cells || !nbr) return pcc::invalidf("%s: null pointer", name);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (a dilation of 65536 or more reaches no cell but the centre: min keeps dil * ksize inside an int)
    const int dil = dilation < kAxisCells ? dilation : kAxisCells;
    if (ksize == 3) launch_map<3>(m, dil, coord, n_cells, nbr, st);
    else launch_map<5>(m, dil, coord, n_cells, nbr, st);
    return pcc::check_launch(name);
}
