// Spatial sort of the point clouds for gfx950 (MI355X), wave64: Hilbert key, register bitonic sort, sorted rows, the
// inverse permutation and one bounding box per 16 sorted points.  Both clouds of an approximate-EMD call are sorted once
// per call (approxmatch.hip skips exact zeros box by box); the k-NN graph sorts its clouds with the same kernel (knn_lowdim.hip).
#include "approxmatch.hpp"
#include "wave_ops.hpp"

#include <algorithm>

namespace {

// Spatial sort: one workgroup per (sample, cloud) orders the points along a 30-bit Hilbert curve with a
// bitonic sort of (code << 32 | index) keys in LDS and writes the sorted SoA coordinates, the inverse
// permutation (rank) and one bounding box per 16 consecutive sorted points.  Clouds too large for the LDS
// sort (> 32768 points = 64 keys per thread) keep their original order: culling then simply finds little to skip.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned part1by2(unsigned v) {
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x030000ff;
    v = (v | (v << 8)) & 0x0300f00f;
    v = (v | (v << 4)) & 0x030c30c3;
    v = (v | (v << 2)) & 0x09249249;
    return v;
}

// 30-bit Hilbert index of a 10-bit lattice point (Skilling's axes-to-transpose, then bit interleave).
// Unlike the Morton order, every contiguous run of the Hilbert order is spatially compact, so all owner
// tiles get similar, small bounding boxes (a Morton run that straddles an octant boundary spans the cloud).
__device__ __forceinline__ unsigned hilbert3(unsigned x0, unsigned x1, unsigned x2) {
    unsigned X[3] = {x0, x1, x2};
    const unsigned M = 1u << 9;
    for (unsigned Q = M; Q > 1; Q >>= 1) {
        const unsigned P = Q - 1;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (X[i] & Q) {
                X[0] ^= P;
            } else {
                const unsigned t = (X[0] ^ X[i]) & P;
                X[0] ^= t;
                X[i] ^= t;
            }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    unsigned t = 0;
    for (unsigned Q = M; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    X[0] ^= t;
    X[1] ^= t;
    X[2] ^= t;
    return (part1by2(X[0]) << 2) | (part1by2(X[1]) << 1) | part1by2(X[2]);
}

struct SortArgs {  // one entry per cloud; blockIdx.y selects it
    int n[2], n4[2], nb[2], npad[2];
    const float *xyz[2];
    // input layout: coordinate c of point i of sample s sits at xyz[s*sstride + i*pstride + c*cstride]; channels
    // >= nch read as 0 (the k-NN graph sorts channels-major clouds of 1..3 channels with the same kernel)
    long long sstride[2], pstride[2], cstride[2];
    int nch[2];
    float *soa[2];
    int *rank[2];
    int *perm[2];      // sorted position -> original index (inverse of rank)
    float4 *aos[2];    // optional [b][n]: (x, y, z, original index as bits) per sorted point (nn_sorted_kernel)
    float *box[2];
    // zero-fill riding along (replaces two memset launches): the two workgroups of a sample clear one region each
    float *zero[2];
    long long zero_stride[2], zero_count[2];  // per-sample stride and length in floats (multiples of 4)
    int *live_cnt;                            // [b][kLiveRow] live-owner counters of the passes B, cleared here
    unsigned *live_mask;                      // [b][kLevels][mask_words] live bits of set2: rows 4.. are preset to ones here
    int mask_words;
};

// Bitonic sort of NPAD = kSortT*SLOTS 32-bit keys held in registers (element i = tid*SLOTS + slot) by an 8-wave
// workgroup: strides < SLOTS are exchanges between a thread's registers, strides < 64*SLOTS between lanes (DPP where the
// partner is a quad / row permutation), only the three longest strides go through LDS.  Fully unrolled so that every
// register index is static.  A key is (truncated Hilbert code << idx_bits) | point index: keys are unique and
// one v_min_u32 / v_max_u32 pair is a whole compare-exchange.
constexpr int kSortT = 512;

template <int SLOTS>
__device__ __forceinline__ void bitonic_sort(unsigned (&key)[SLOTS], unsigned *lds, int tid) {
    // element tid * SLOTS + s sits in slot s of thread tid (a thread's keys are neighbours): the SHORT strides -- the ones
    // every merge repeats -- are exchanges between registers, the middle ones between lanes, and only the three longest
    // strides (6 stages of the 66 at 2048 keys) cross waves through LDS.  (With element tid + 512 s the three strides 64 /
    // 128 / 256 went through LDS, 12 stages with two barriers each: half of the sort's time, timed inside the kernel.)
    constexpr int NPAD = kSortT * SLOTS;
#pragma unroll
    for (int kk = 2; kk <= NPAD; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1) {
            if (j < SLOTS) {
#pragma unroll
                for (int s = 0; s < SLOTS; s++) {
                    const int sp = s ^ j;
                    if (sp > s) {
                        const bool asc = ((tid * SLOTS + s) & kk) == 0;
                        const unsigned mn = min(key[s], key[sp]), mx = max(key[s], key[sp]);
                        key[s] = asc ? mn : mx;
                        key[sp] = asc ? mx : mn;
                    }
                }
            } else {
                const int L = j / SLOTS;  // the partner is slot s of thread tid ^ L
                if (L >= 64) {
                    __syncthreads();
#pragma unroll
                    for (int s = 0; s < SLOTS; s++) lds[tid + kSortT * s] = key[s];
                    __syncthreads();
                }
#pragma unroll
                for (int s = 0; s < SLOTS; s++) {
                    // the partner lane ^ L: one DPP move for L = 1, 2 (quad permutations) and 8 (a rotation by 8 of the row
                    // of 16 IS lane ^ 8), two rotations and a select for 4; the LDS crossbar (ds_bpermute) for 16 and 32
                    unsigned other;
                    if (L >= 64) other = lds[(tid ^ L) + kSortT * s];
                    else if (L == 1) other = pcc::dpp<pcc::kQuadXor1>(key[s]);
                    else if (L == 2) other = pcc::dpp<pcc::kQuadXor2>(key[s]);
                    else if (L == 8) other = pcc::row_ror<8>(key[s]);
                    else if (L == 4) {
                        // (row_ror:n hands lane i the value of lane i - n of its row)
                        const unsigned lo4 = pcc::row_ror<4>(key[s]);    // from lane - 4
                        const unsigned hi4 = pcc::row_ror<12>(key[s]);   // from lane - 12 = lane + 4
                        other = (tid & 4) ? lo4 : hi4;
                    } else other = (unsigned)__shfl_xor((int)key[s], L, 64);
                    const bool take_min = ((tid & L) == 0) == (((tid * SLOTS + s) & kk) == 0);
                    key[s] = take_min ? min(key[s], other) : max(key[s], other);
                }
            }
        }
    }
}

template <int SLOTS>
__global__ __launch_bounds__(kSortT) void am_sort_kernel(SortArgs a) {
    constexpr bool MIRROR = SLOTS <= 8;  // clouds of up to 4096 points keep their coordinates in LDS (48 KB) for the gather
    __shared__ unsigned lds_keys[kSortT * SLOTS];
    __shared__ float lds_xyz[MIRROR ? 3 * kSortT * SLOTS : 1];
    __shared__ float red[6][16];
    const int which = blockIdx.y;
    const int n = a.n[which], n4 = a.n4[which], nb = a.nb[which], npad = a.npad[which];
    const int smp = blockIdx.x, tid = threadIdx.x, T = kSortT;
    if (a.live_cnt && which == 0 && (threadIdx.x < kInfSlot || threadIdx.x == kErrSlot))  // (kInfSlot.. are set below)
        a.live_cnt[(size_t)blockIdx.x * kLiveRow + threadIdx.x] = 0;
    if (a.live_mask && which == 1)  // (rows 4.. of the live masks start as all ones: PhaseArgs::mask_out)
        for (int i = 4 * a.mask_words + threadIdx.x; i < kLevels * a.mask_words; i += kSortT)
            a.live_mask[(size_t)blockIdx.x * kLevels * a.mask_words + i] = ~0u;
    if (a.zero[which]) {  // fire-and-forget stores, hidden under the sort
        float4 *z = reinterpret_cast<float4 *>(a.zero[which] + (size_t)smp * a.zero_stride[which]);
        const long long cnt4 = a.zero_count[which] / 4;
        for (long long i = tid; i < cnt4; i += T) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float *p = a.xyz[which] + (size_t)smp * a.sstride[which];
    const long long ps = a.pstride[which], cs = a.cstride[which];
    const int nch = a.nch[which];
    auto coord = [&](int i, int c) -> float { return c < nch ? p[i * ps + c * cs] : 0.f; };
    float *so = a.soa[which] ? a.soa[which] + (size_t)smp * 3 * n4 : nullptr;
    int *rk = a.rank[which] ? a.rank[which] + (size_t)smp * n : nullptr;
    int *pm = a.perm[which] + (size_t)smp * n;
    float4 *ao = a.aos[which] ? a.aos[which] + (size_t)smp * n : nullptr;
    float *bx = a.box[which] + (size_t)smp * nb * 8;
    int idx_bits = 10;
    while ((1 << idx_bits) < npad) idx_bits++;  // npad >= 1024
    const unsigned idx_mask = (1u << idx_bits) - 1;
    if (npad) {
        const int code_shift = 30 - 3 * ((32 - idx_bits) / 3);  // keep the leading 3*floor((32-idx_bits)/3) code bits
        // The thread's points: every load issued before anything consumes one (ONE round trip; read in a loop with the
        // min/max next to each load, and again for the keys, the kernel waited out eight), kept in registers for the
        // bounding box and the keys, and mirrored in LDS where the cloud fits, for the gather behind the sort.
        // (up to 16 slots -- 8192 points -- stay in registers; larger clouds read their points twice, as they come)
        constexpr bool KEEP = SLOTS <= 16;
        constexpr int BATCH = SLOTS < 8 ? SLOTS : 8;
        constexpr int NKEEP = KEEP ? SLOTS : BATCH;
        float px[NKEEP], py[NKEEP], pz[NKEEP];
        const int c1 = min(1, nch - 1), c2 = min(2, nch - 1);
        const int k1 = -(int)(nch > 1), k2 = -(int)(nch > 2);  // channels >= nch read as 0
        auto load_batch = [&](int s0, int r0) {  // slots s0 .. s0 + BATCH - 1 into registers r0 ..
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                const long long i = min(tid * SLOTS + (s0 + u), n - 1);
                px[r0 + u] = p[i * ps];
                py[r0 + u] = p[i * ps + c1 * cs];
                pz[r0 + u] = p[i * ps + c2 * cs];
            }
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                py[r0 + u] = __int_as_float(__float_as_int(py[r0 + u]) & k1);
                pz[r0 + u] = __int_as_float(__float_as_int(pz[r0 + u]) & k2);
            }
        };
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
        float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        if (!KEEP) {
            for (int i = tid; i < n; i += T)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float v = coord(i, c);
                    lo[c] = fminf(lo[c], v);
                    hi[c] = fmaxf(hi[c], v);
                }
        }
#pragma unroll
        for (int s0 = 0; s0 < (KEEP ? SLOTS : 0); s0 += BATCH) {
            const int r0 = s0;
            load_batch(s0, r0);
#pragma unroll
            for (int u = 0; u < BATCH; u++) {  // (a slot past the cloud repeats the last point: no effect on the box)
                lo[0] = fminf(lo[0], px[r0 + u]); hi[0] = fmaxf(hi[0], px[r0 + u]);
                lo[1] = fminf(lo[1], py[r0 + u]); hi[1] = fmaxf(hi[1], py[r0 + u]);
                lo[2] = fminf(lo[2], pz[r0 + u]); hi[2] = fmaxf(hi[2], pz[r0 + u]);
                if (MIRROR) {
                    lds_xyz[tid * SLOTS + (s0 + u)] = px[r0 + u];
                    lds_xyz[kSortT * SLOTS + tid * SLOTS + (s0 + u)] = py[r0 + u];
                    lds_xyz[2 * kSortT * SLOTS + tid * SLOTS + (s0 + u)] = pz[r0 + u];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // (inside the rows of 16 lanes by DPP rotations, across the four rows through the LDS crossbar)
            lo[c] = fminf(lo[c], pcc::row_ror<8>(lo[c])); hi[c] = fmaxf(hi[c], pcc::row_ror<8>(hi[c]));
            lo[c] = fminf(lo[c], pcc::row_ror<4>(lo[c])); hi[c] = fmaxf(hi[c], pcc::row_ror<4>(hi[c]));
            lo[c] = fminf(lo[c], pcc::row_ror<2>(lo[c])); hi[c] = fmaxf(hi[c], pcc::row_ror<2>(hi[c]));
            lo[c] = fminf(lo[c], pcc::row_ror<1>(lo[c])); hi[c] = fmaxf(hi[c], pcc::row_ror<1>(hi[c]));
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) {
                lo[c] = fminf(lo[c], __shfl_xor(lo[c], off, 64));
                hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], off, 64));
            }
            if ((tid & 63) == 0) {
                red[c][tid >> 6] = lo[c];
                red[3 + c][tid >> 6] = hi[c];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float l = red[c][0], h = red[3 + c][0];
            for (int i = 1; i < kSortT / 64; i++) {
                l = fminf(l, red[c][i]);
                h = fmaxf(h, red[3 + c][i]);
            }
            lo[c] = l;
            hi[c] = h > l ? 1023.f / (h - l) : 0.f;  // scale
        }
        unsigned key[SLOTS];
        if (!KEEP) {
#pragma unroll
            for (int s2 = 0; s2 < SLOTS; s2++) {
                const int i = tid * SLOTS + s2;
                key[s2] = ~0u;
                if (i < n) {
                    const unsigned qx = (unsigned)fminf(fmaxf((coord(i, 0) - lo[0]) * hi[0], 0.f), 1023.f);
                    const unsigned qy = (unsigned)fminf(fmaxf((coord(i, 1) - lo[1]) * hi[1], 0.f), 1023.f);
                    const unsigned qz = (unsigned)fminf(fmaxf((coord(i, 2) - lo[2]) * hi[2], 0.f), 1023.f);
                    key[s2] = ((hilbert3(qx, qy, qz) >> code_shift) << idx_bits) | (unsigned)i;
                }
            }
        }
#pragma unroll
        for (int s0 = 0; s0 < (KEEP ? SLOTS : 0); s0 += BATCH) {
            const int r0 = s0;
#pragma unroll
            for (int u = 0; u < BATCH; u++) {
                const int i = tid * SLOTS + (s0 + u);
                const unsigned qx = (unsigned)fminf(fmaxf((px[r0 + u] - lo[0]) * hi[0], 0.f), 1023.f);
                const unsigned qy = (unsigned)fminf(fmaxf((py[r0 + u] - lo[1]) * hi[1], 0.f), 1023.f);
                const unsigned qz = (unsigned)fminf(fmaxf((pz[r0 + u] - lo[2]) * hi[2], 0.f), 1023.f);
                const unsigned kv = ((hilbert3(qx, qy, qz) >> code_shift) << idx_bits) | (unsigned)i;
                key[s0 + u] = i < n ? kv : ~0u;
            }
        }
        bitonic_sort<SLOTS>(key, lds_keys, tid);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SLOTS; s++) lds_keys[tid * SLOTS + s] = key[s];
        __syncthreads();
    }
    // sorted SoA rows + inverse permutation; the box of every 16 consecutive sorted points falls out of a
    // 16-lane min/max butterfly on the coordinates the lanes already hold
    const int span = ((max(n4, nb * kBox) + 63) / 64) * 64;
    int has_inf = 0;
    auto emit = [&](int s) {  // sorted position s: its point, its rows, its box
        float x = 0.f, y = 0.f, z = 0.f;
        const bool real = s < n;
        if (real) {
            const int orig = npad ? (int)(lds_keys[s] & idx_mask) : s;
            if (MIRROR && npad) {
                x = lds_xyz[orig];
                y = lds_xyz[kSortT * SLOTS + orig];
                z = lds_xyz[2 * kSortT * SLOTS + orig];
            } else {
                x = coord(orig, 0);
                y = coord(orig, 1);
                z = coord(orig, 2);
            }
            has_inf |= (__builtin_isinf(x) || __builtin_isinf(y) || __builtin_isinf(z)) ? 1 : 0;
            if (rk) rk[orig] = s;
            pm[s] = orig;
            if (ao) ao[s] = make_float4(x, y, z, __int_as_float(orig));
        }
        if (so && s < n4) {
            so[s] = x;
            so[n4 + s] = y;
            so[2 * n4 + s] = z;
        }
        float l0 = real ? x : __builtin_inff(), l1 = real ? y : __builtin_inff(), l2 = real ? z : __builtin_inff();
        float h0 = real ? x : -__builtin_inff(), h1 = real ? y : -__builtin_inff(), h2 = real ? z : -__builtin_inff();
        // (min / max over the 16 lanes of a DPP row, in every lane: four rotations of the row)
        static_assert(kBox == 16, "a box is a DPP row");
        const auto fmin2 = [](float a, float b) { return fminf(a, b); };
        const auto fmax2 = [](float a, float b) { return fmaxf(a, b); };
        l0 = pcc::row_reduce16_ror(l0, fmin2); l1 = pcc::row_reduce16_ror(l1, fmin2); l2 = pcc::row_reduce16_ror(l2, fmin2);
        h0 = pcc::row_reduce16_ror(h0, fmax2); h1 = pcc::row_reduce16_ror(h1, fmax2); h2 = pcc::row_reduce16_ror(h2, fmax2);
        const int bb = s / kBox;
        if ((s & (kBox - 1)) == 0 && bb < nb) {
            float4 *dst = reinterpret_cast<float4 *>(bx + (size_t)bb * 8);
            dst[0] = make_float4(l0, l1, l2, 0.f);
            dst[1] = make_float4(h0, h1, h2, 0.f);
        }
    };
    if (npad && SLOTS <= 8) {  // (unrolled: the LDS reads of all of a thread's positions are in flight together)
#pragma unroll
        for (int k2 = 0; k2 < SLOTS; k2++)
            if (tid + k2 * T < span) emit(tid + k2 * T);  // (span is a multiple of 64: whole waves take the branch)
    } else {
        for (int s = tid; s < span; s += T) emit(s);
    }
    // An infinite coordinate makes every pair of its point exp(-inf) = 0 -- skipped here as an exact zero -- while the
    // reference goes on to multiply that 0 by sqrt(inf): its cost and gradients of the sample are NaN (approxmatch.cu:207,
    // 247-248).  The sample is flagged and the finish kernel reports NaN.  (NaN coordinates need no flag: they reach the
    // sums through the distances, as in the reference.)
    if (a.live_cnt) {
        const int any_inf = __syncthreads_or(has_inf);
        if (tid == 0) a.live_cnt[(size_t)blockIdx.x * kLiveRow + kInfSlot + which] = any_inf ? 1 : 0;
    }
}

void launch_sort(const SortArgs &a, int slots, dim3 grid, hipStream_t st) {
    // (the profiler names the instantiation; the prefix "am_sort_kernel" still counts them all)
    const char *name = slots == 4 ? "am_sort_kernel<4>" : slots == 8 ? "am_sort_kernel<8>" : slots == 16 ? "am_sort_kernel<16>"
                     : slots == 32 ? "am_sort_kernel<32>" : "am_sort_kernel<64>";
    pcc::ProfScope prof(name, st);
    switch (slots) {
    case 4: hipLaunchKernelGGL((am_sort_kernel<4>), grid, dim3(kSortT), 0, st, a); break;
    case 8: hipLaunchKernelGGL((am_sort_kernel<8>), grid, dim3(kSortT), 0, st, a); break;
    case 16: hipLaunchKernelGGL((am_sort_kernel<16>), grid, dim3(kSortT), 0, st, a); break;
    case 32: hipLaunchKernelGGL((am_sort_kernel<32>), grid, dim3(kSortT), 0, st, a); break;
    default: hipLaunchKernelGGL((am_sort_kernel<64>), grid, dim3(kSortT), 0, st, a); break;
    }
}

}  // namespace

namespace pcc {

// Sorts the bc samples of the view `v` (xyz1 / xyz2: their first sample); `aos`: also write the packed rows aos1 / aos2.
int sort_clouds(const AmDims &L, const WsView &v, int bc, const float *xyz1, const float *xyz2, bool aos, hipStream_t st) {
    SortArgs a{};
    a.live_cnt = v.live_cnt;
    a.live_mask = v.live_mask;
    a.mask_words = mask_words(L.m4);
    if (aos) { a.aos[0] = v.aos1; a.aos[1] = v.aos2; }
    // the padded tails of the weight rows are staged as float4: they must be finite (their candidates sit at the
    // origin with these weights), and V_COWN relies on zero-filled level arrays for the exhausted owners it never
    // touches: remain rows are cleared by the workgroup sorting set1, level rows by the one sorting set2
    a.zero[0] = v.rem; a.zero_stride[0] = a.zero_count[0] = (long long)L.rem_floats();
    a.zero[1] = v.lv; a.zero_stride[1] = a.zero_count[1] = (long long)L.lv_floats();
    const int nn[2] = {L.n, L.m};
    int slots = 4;
    for (int w = 0; w < 2; w++) {
        int npad = 4 * kSortT;
        while (npad < nn[w]) npad <<= 1;
        if (npad > 64 * kSortT) npad = 0;  // > 32768 points: keep the original order (nothing is culled)
        a.n[w] = nn[w];
        a.npad[w] = npad;
        slots = std::max(slots, npad / kSortT);
    }
    for (int w = 0; w < 2; w++)
        if (a.npad[w]) a.npad[w] = kSortT * slots;  // one SLOTS instantiation serves both clouds
    a.n4[0] = L.n4; a.n4[1] = L.m4; a.nb[0] = L.nb1; a.nb[1] = L.nb2;
    a.xyz[0] = xyz1; a.xyz[1] = xyz2; a.soa[0] = v.soa1; a.soa[1] = v.soa2;
    for (int w = 0; w < 2; w++) {
        a.sstride[w] = (long long)nn[w] * 3; a.pstride[w] = 3; a.cstride[w] = 1; a.nch[w] = 3;
    }
    a.rank[0] = v.rank1; a.rank[1] = v.rank2; a.perm[0] = v.perm1; a.perm[1] = v.perm2; a.box[0] = v.box1; a.box[1] = v.box2;
    launch_sort(a, slots, dim3(bc, 2), st);
    return pcc::check_launch("approxmatch(sort)");
}

// Hilbert sort of ONE channels-major cloud per sample (x[b][c][n], 1 <= c <= 3) for the k-NN graph (knn_lowdim.hip): packed
// sorted rows (x, y, z, original index), the 16-point boxes and the sorted -> original permutation.
int sort_cloud_cmajor(int b, int c, int n, const float *x, float4 *aos, float *box16, int *perm, hipStream_t st) {
    SortArgs a{};
    int npad = 4 * kSortT;
    while (npad < n) npad <<= 1;
    if (npad > 64 * kSortT) npad = 0;  // > 32768 points: original order (the k-NN graph stops at kSortedMaxN = 16384 and never gets here)
    a.n[0] = n; a.npad[0] = npad; a.n4[0] = (n + 3) & ~3; a.nb[0] = pcc::ceil_div(n, kBox);
    a.xyz[0] = x; a.sstride[0] = (long long)c * n; a.pstride[0] = 1; a.cstride[0] = n; a.nch[0] = c;
    a.aos[0] = aos; a.box[0] = box16; a.perm[0] = perm;
    launch_sort(a, npad ? npad / kSortT : 4, dim3(b, 1), st);
    return pcc::check_launch("knn(sort)");
}
}  // namespace pcc
