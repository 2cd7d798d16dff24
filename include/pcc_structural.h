/*
 * pcc_structural.h -- C ABI of libpcc_structural.so (MI355X / gfx950 structural-loss kernels).
 *
 * Drop-in boundary for the native half of the reference's `structural_losses` package: the five
 * launchers declared at external/pytorch_structural_losses/src/structural_loss.cpp:10-14 and
 * defined in nndistance.cu:125-128,149-154 and approxmatch.cu:299-326 of the reference.  Same names,
 * same argument order and meaning; the only change is `cudaStream_t` -> `hipStream_t` (passed as
 * `void *` so that the header needs no HIP include).  All pointers are device pointers to
 * contiguous row-major float32 / int32 arrays; inputs are borrowed and never written; outputs are
 * fully overwritten.  Calls enqueue work on `stream` and return without synchronising -- with one exception that is the
 * runtime's, not the library's: an entry that takes a workspace from the library's memory pool gives it back with
 * hipFreeAsync on `stream`, and when an earlier call on the same stream, not yet executed, had freed the very block this call
 * was handed, that hipFreeAsync waits on the host until the stream has reached the earlier free (ROCm 7.0).  A call on a
 * stream that holds no unfinished call of the library returns at once, however busy the stream is with other work.
 * tests/test_gpu_stream_order.py runs every entry point on a side stream behind late inputs and asserts both; the table
 * WAITS of tests/stream_order.py names the entries that take such a workspace.
 *
 * Error behaviour: the reference's approxmatch/matchcost/matchcostgrad launchers throw
 * std::runtime_error("CUDA kernel failed : <code>") (approxmatch.cu:303-306) and its nndistance
 * launchers check nothing.  A C ABI cannot throw, so every `pcc_*` entry returns an int
 * (0 = success, otherwise the hipError_t of the failed launch / a PCC_E* code) and records a message
 * retrievable with pcc_last_error(); the reference-named void launchers record the same message and
 * the host-side binding raises RuntimeError("HIP kernel failed : <code>") from it.
 *
 * Alignment: every tensor argument, input or output, may be any contiguous buffer aligned to its element size (4 bytes
 * here: float32 and int32).  The kernels take wider accesses only where the sizes and the address allow it and fall
 * back to element accesses otherwise (tests/test_gpu_unaligned_views.py runs every entry point on such buffers).  The one
 * exception is the caller-provided workspace of pcc_approxmatch_ws, which must be 16-byte aligned (PCC_EINVAL otherwise).
 */
#ifndef PCC_STRUCTURAL_H
#define PCC_STRUCTURAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built -fvisibility=hidden; only this ABI is exported */

typedef void *pcc_stream_t; /* hipStream_t */

#define PCC_OK 0
#define PCC_EINVAL (-22)  /* bad sizes / null pointers */
#define PCC_ENOMEM (-12)  /* workspace allocation failed */

/* ---- library info ------------------------------------------------------------------------- */
const char *pcc_version(void);
/* Message of the last failed call on this thread ("" if none). */
const char *pcc_last_error(void);
/* Status of the last reference-named (void) launcher call on this thread; reset to 0 by each call. */
int pcc_last_status(void);

/* ---- per-kernel timing (measurement aid, off by default) ----------------------------------------
 * pcc_profile_enable(1): every kernel launch of this library is bracketed by two hipEvents recorded on the
 * launch stream.  pcc_profile_enable(2): only whole launch SEQUENCES are bracketed (one event before the first
 * launch, one after the last; name "am_phase_sequence" = the 19 back-to-back am_phase_kernel launches of one
 * approxmatch) -- no event sits between the kernels, so sequence / launches is the per-launch duration a kernel
 * trace reports.  pcc_profile_enable(0): off.  pcc_profile_read synchronises on the recorded events and returns the
 * average duration (microseconds) and the number of recorded scopes whose name starts with `kernel_prefix` since the
 * last enable / pcc_profile_reset().  Returns 0, or PCC_EINVAL if nothing matched.  Not thread-safe against
 * concurrent launches; meant for bench.py.
 * pcc_profile_names is the exact launch record since the last enable / pcc_profile_reset(): one line
 * "name<TAB>launches<LF>" per distinct scope name, whole names (no prefix matching: "am_materialise_kernel" and
 * "am_materialise_kernel<cost>" are two lines), in the order of each name's first launch.  A name carries the template
 * instantiation wherever a launcher picks one of several ("fps_reg_kernel<256,8>").  Waits for the recorded events,
 * writes at most capacity - 1 bytes and a terminating 0 into buf (nothing if buf is NULL or capacity is 0) and returns
 * the bytes the whole text needs, terminator included: call again with a larger buffer if that exceeds capacity. */
void pcc_profile_enable(int on);
void pcc_profile_reset(void);
int pcc_profile_read(const char *kernel_prefix, double *avg_us, int *launches);
size_t pcc_profile_names(char *buf, size_t capacity);

/* ---- Chamfer nearest neighbour ---------------------------------------------------------------
 * Replaces `nndistance` (reference nndistance.cu:125-128; declared structural_loss.cpp:13).
 *   xyz[b,n,3], xyz2[b,m,3] -> result[b,n] = min_k |xyz_j - xyz2_k|^2, result_i[b,n] = argmin
 *   (lowest index on ties), and the same with roles swapped -> result2[b,m], result2_i[b,m].
 * Distances are evaluated as fmaf(dz,dz, fmaf(dx,dx, dy*dy)) on differences (bit-exact vs oracle).
 * Non-finite coordinates follow the reference's loop literally (nndistance.cu:26-28,116: `k == 0 || d < best` inside
 * 512-candidate chunks, chunks merged with `result > best`): a NaN query or a NaN candidate 0 gives NaN / index 0; a NaN
 * candidate at index 512 c (c >= 1) hides candidates 512 c .. 512 c + 511 from every query; a NaN candidate elsewhere never
 * wins.  (pcc_chamfer_emd, like the approximate EMD itself, is specified for finite coordinates.) */
void nndistance(int b, int n, const float *xyz, int m, const float *xyz2, float *result, int *result_i,
                float *result2, int *result2_i, pcc_stream_t stream);
int pcc_nndistance(int b, int n, const float *xyz, int m, const float *xyz2, float *result, int *result_i,
                   float *result2, int *result2_i, pcc_stream_t stream);

/* Replaces `nndistancegrad` (reference nndistance.cu:149-154; declared structural_loss.cpp:14).
 *   grad_xyz1[b,n,3] = 2 g1_j (p1_j - p2_{idx1_j}) + sum_{k: idx2_k = j} 2 g2_k (p1_j - p2_k), and
 *   symmetrically grad_xyz2[b,m,3].  Outputs are overwritten (no prior memset needed). */
void nndistancegrad(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                    const int *idx1, const float *grad_dist2, const int *idx2, float *grad_xyz1,
                    float *grad_xyz2, pcc_stream_t stream);
int pcc_nndistancegrad(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                       const int *idx1, const float *grad_dist2, const int *idx2, float *grad_xyz1,
                       float *grad_xyz2, pcc_stream_t stream);

/* ---- Chamfer loss with the reduction fused (extension) ----------------------------------------------
 * What the reference's training path computes around the nearest-neighbour search
 * (src/train/metrics_and_losses.py:21-47): loss[b] = mean_j dist1[b,j] + mean_k dist2[b,k] (`mean` != 0,
 * pykeops_chamfer) or the plain sums (`mean` == 0, torch_chamfer's scale).  pcc_chamfer_loss = pcc_nndistance + one
 * fixed-order reduction; pcc_chamfer_loss_grad = pcc_nndistancegrad with grad_dist1[b,:] = grad_loss[b] (/ n),
 * grad_dist2[b,:] = grad_loss[b] (/ m) formed inside the kernel; grad_loss_stride is 1, or 0 when the upstream
 * gradient is one scalar expanded over the batch (what `loss.sum().backward()` hands down). */
int pcc_chamfer_loss(int b, int n, const float *xyz1, int m, const float *xyz2, int mean, float *loss, float *dist1,
                     int *idx1, float *dist2, int *idx2, pcc_stream_t stream);
int pcc_chamfer_loss_grad(int b, int n, const float *xyz1, int m, const float *xyz2, const int *idx1, const int *idx2,
                          const float *grad_loss, int grad_loss_stride, int mean, float *grad_xyz1, float *grad_xyz2,
                          pcc_stream_t stream);

/* Forward of the reference's ChamferEMD reconstruction loss (src/train/metrics_and_losses.py:70-79: Chamfer and
 * match_cost on the same pair of clouds) in one call: pcc_chamfer_loss + pcc_match_cost, same outputs, same bits.
 * emd_grad1 / emd_grad2: both or neither (NULL: cost only).
 * Non-finite coordinates: the VALUES are specified for finite coordinates only (the chunk quirks of pcc_nndistance above
 * are not reproduced).  For ANY input, every index written to idx1 lies in [0, m) and every index written to idx2 in
 * [0, n), so the backward below never gathers outside a cloud.  A query point with a NaN coordinate -- and any query
 * whose every candidate distance is NaN -- gets distance NaN / index 0, as in pcc_nndistance, which makes the sample's
 * chamfer_loss NaN.  The samples of the batch without a non-finite coordinate are unaffected: same bits as without the
 * others. */
int pcc_chamfer_emd(int b, int n, const float *xyz1, int m, const float *xyz2, int mean, float *chamfer_loss,
                    float *dist1, int *idx1, float *dist2, int *idx2, float *emd_cost, float *emd_grad1,
                    float *emd_grad2, pcc_stream_t stream);

/* Backward of the reference's ChamferEMD reconstruction loss (src/train/metrics_and_losses.py:70-79: Chamfer and
 * match_cost on the same pair of clouds) in one launch: pcc_chamfer_loss_grad of grad_chamfer[b] plus the unscaled
 * match_cost gradients emd_grad1[b,n,3] / emd_grad2[b,m,3] (as pcc_match_cost returns them) times grad_emd[b]
 * (NULL = 1).  Strides as above (0 = one scalar for the batch).  Bit-identical to the two backward passes followed by
 * autograd's gradient accumulation. */
int pcc_chamfer_emd_grad(int b, int n, const float *xyz1, int m, const float *xyz2, const int *idx1, const int *idx2,
                         const float *grad_chamfer, int grad_chamfer_stride, int mean, const float *emd_grad1,
                         const float *emd_grad2, const float *grad_emd, int grad_emd_stride, float *grad_xyz1,
                         float *grad_xyz2, pcc_stream_t stream);

/* ---- all-pairs Chamfer distances between two banks of clouds (extension) -------------------------------
 * What scoring a generated SET needs (minimum matching distance, coverage, 1-NN accuracy): every cloud of one bank
 * against every cloud of the other, where the entry points above pair sample b with sample b.
 *   a[s,n,3], bank[r,m,3] -> d_ab[s,r] = mean_p min_q |a_i,p - bank_j,q|^2, d_ba[s,r] = mean_q min_p (same pairs);
 *   mean != 0: divide by n / m; mean == 0: plain sums.  Either output may be NULL (both: nothing is enqueued).
 * Distances: every point-pair distance is fmaf(dz,dz, fmaf(dx,dx, dy*dy)) on differences, the expression of
 *   pcc_nndistance, so each minimum is bit-equal to pcc_nndistance's result / result2 for that pair of clouds.
 * Reduction: an entry is a fixed-order float32 sum of those minima (no float atomics): it depends on a_i, bank_j, n, m
 *   and `mean` only -- not on s, r, the position of the clouds in their banks or the launch geometry -- and is
 *   bit-reproducible from run to run.
 * Self mode: a == bank (the same pointer) with s == r and n == m evaluates i <= j only and mirrors the results,
 *   d_ab[j,i] = d_ba[i,j]; the diagonal is exactly 0; the output equals, bit for bit, that of the general mode on
 *   (a, a copy of a).  Exception: clouds of more than 2048 points (n > 2048) are evaluated for all s * s pairs, the
 *   diagonal included, one direction per pair (the other is its mirror) -- no work is saved there; same bits.
 * Sizes: any n, m >= 1 (up to 2^30); s == 0 or r == 0 enqueues nothing and returns PCC_OK; negative sizes, an empty
 *   cloud or a null input return PCC_EINVAL.  Offsets are 64-bit.  No synchronisation, no allocation.
 * Non-finite coordinates: specified for finite coordinates; a cloud holding a NaN or an infinite coordinate gives NaN in
 *   every entry it takes part in (its row of both outputs for a cloud of a, its column for a cloud of bank). */
int pcc_chamfer_matrix(int s, int n, const float *a, int r, int m, const float *bank, int mean, float *d_ab,
                       float *d_ba, pcc_stream_t stream);

/* ---- voxel occupancy counts of a bank of clouds (extension) ------------------------------------------
 * What the Jensen-Shannon divergence between two SETS of clouds is computed from (the fourth number of the MMD / COV /
 * 1-NNA table), and per cloud what voxel IoU and density checks need.
 *   xyz[s,n,3] -> counts[res^3] (per_cloud == 0: the whole bank in one histogram) or counts[s,res^3] (per_cloud != 0);
 *   counts[cell] = the number of points whose cell it is.  counts is overwritten: the call zeroes what it must, on `stream`.
 * Grid: res points per axis on [lo, lo + extent]^3; grid point (i,j,k) sits at lo + i extent / (res - 1) on each axis and
 *   has the flat index (i res + j) res + k.
 * Cell of a finite point, full grid (in_sphere == 0): per axis, in float32 with exactly these roundings,
 *   t = (x - lo) * inv with inv = (float)(res - 1) / extent computed once on the host (subtract and multiply are two
 *   roundings: the library is built with -ffp-contract=off), i = (int)fminf(fmaxf(floorf(t + 0.5f), 0.f), (float)(res - 1)).
 *   The clamp is applied to floats, before the conversion.  This is the nearest grid point up to one rounding at a cell
 *   border (a midpoint goes up); a point outside the cube lands in a border cell, as a nearest-neighbour query puts it.
 * in_sphere != 0: only grid points inside the inscribed sphere count, tested in integers:
 *   (2i - (res-1))^2 + (2j - (res-1))^2 + (2k - (res-1))^2 <= (res-1)^2.  A point whose separable cell passes keeps it.  Any
 *   other point goes to its nearest in-sphere grid point, found column by column: for each (i,j) whose in-sphere interval
 *   [klo, khi] is not empty the candidate is k = the point's separable k clamped into the interval (the distance is convex
 *   in k), at distance pcc::sq3(px - gx, py - gy, pz - gz) = fmaf(dz,dz, fmaf(dx,dx, dy*dy)) with g = (float)index * step +
 *   lo (two roundings) and step = extent / (float)(res - 1); the lowest float32 distance wins, the lowest flat index among
 *   equal distances.
 * Non-finite points: a point with a NaN or infinite coordinate is counted nowhere; the counts sum to the number of finite
 *   points.
 * Determinism: integer adds only, so the counts are identical for every launch geometry, from run to run, and between
 *   the library's two paths (a workgroup-private histogram in LDS for res <= 32, one global atomic per point above).
 * Sizes: s >= 0 (s == 0 enqueues nothing), n >= 1, 2 <= res <= 128 (res >= 3 with in_sphere: at res 2 no grid point
 *   qualifies), extent finite and > 0, lo finite, s n <= INT_MAX, per_cloud: s res^3 <= INT_MAX; otherwise PCC_EINVAL, before
 *   anything is enqueued.  No host synchronisation; may be captured into a graph; with in_sphere the call takes
 *   4 (s n + 4) bytes of stream-ordered workspace (PCC_ENOMEM if that fails). */
int pcc_occupancy_grid(int s, int n, const float *xyz, int res, float lo, float extent, int in_sphere, int per_cloud,
                       int32_t *counts, pcc_stream_t stream);

/* ---- approximate EMD ---------------------------------------------------------------------------
 * Replaces `approxmatch` (reference approxmatch.cu:299-307; declared structural_loss.cpp:10).
 *   xyz1[b,n,3], xyz2[b,m,3] -> match[b,m,n] (query-major), temp[b,2(n+m)] =
 *   [remainL(n) | remainR(m) | ratioL(n) | ratioR(m)] after the last level.
 * The reference-named form allocates its per-level workspace with hipMallocAsync on `stream`;
 * pcc_approxmatch_ws takes a caller-provided workspace of pcc_approxmatch_workspace_bytes(b,n,m)
 * bytes instead (graph-capture friendly, no allocation in the call).
 * Failure: if a sample barrier of the resident launch of levels 0-2 times out, that sample's match and temp are NaN and
 * the next approximate-EMD call on the device (any entry point here) returns PCC_EINVAL ("did not complete"). */
void approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                 pcc_stream_t stream);
int pcc_approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                    pcc_stream_t stream);
size_t pcc_approxmatch_workspace_bytes(int b, int n, int m);
int pcc_approxmatch_ws(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                       void *workspace, size_t workspace_bytes, pcc_stream_t stream);

/* approxmatch + matchcost in one call (what the Python-level match_cost forward needs,
 * reference structural_losses/match_cost.py:25-27): the pass that materialises `match` also
 * accumulates cost[b], so `match` is not re-read.  Same results as pcc_approxmatch + pcc_matchcost up to
 * float summation order.  Failure as for pcc_approxmatch: NaN match, temp and cost for the sample. */
int pcc_approxmatch_cost(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *temp,
                         float *cost, pcc_stream_t stream);

/* Replaces `matchcost` (reference approxmatch.cu:309-316; declared structural_loss.cpp:11).
 *   out[b] = sum_{k<m} sum_{j<n} match[b,k,j] * sqrt(|xyz1_j - xyz2_k|^2).  `match` is read-only
 *   (the reference declares it non-const but never writes it).
 * b <= 65535 (the batch is a grid dimension): more returns PCC_EINVAL "matchcost: batch too large" before anything is
 * allocated or enqueued.  The same limit and message, under their own names, hold for matchcostgrad, approxmatch and
 * pcc_match_cost / pcc_chamfer_emd. */
void matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, float *match, float *out,
               pcc_stream_t stream);
int pcc_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *out,
                  pcc_stream_t stream);

/* Replaces `matchcostgrad` (reference approxmatch.cu:318-326; declared structural_loss.cpp:12).
 *   grad1[b,l,:] = sum_k match[b,k,l] (p1_l - p2_k) rsqrt(max(d2,1e-20));
 *   grad2[b,k,:] = sum_j match[b,k,j] (p2_k - p1_j) rsqrt(max(d2,1e-20)). */
void matchcostgrad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                   float *grad1, float *grad2, pcc_stream_t stream);
int pcc_matchcostgrad(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                      float *grad1, float *grad2, pcc_stream_t stream);
/* The same with the upstream gradient folded in: grad1[b] *= grad_cost[b], grad2[b] *= grad_cost[b] -- what the
 * Python wrapper does with two extra elementwise passes (match_cost.py:41-42).  grad_cost == NULL means 1.
 * Both refuse b > 65535 ("matchcostgrad: batch too large"). */
int pcc_matchcostgrad_scaled(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match,
                             const float *grad_cost, float *grad1, float *grad2, pcc_stream_t stream);

/* ---- match_cost without the match tensor (extension) ---------------------------------------------
 * The Python-level match_cost (reference structural_losses/match_cost.py:11-50) needs cost[b] in forward and
 * grad * grad_cost[b] in backward; `match` only travels from ApproxMatch to MatchCost / MatchCostGrad and the
 * gradient treats it as a constant (approxmatch.cu:229-291).  pcc_match_cost evaluates every match element in
 * registers (same level order and rounding as pcc_approxmatch) and feeds it straight into the cost and gradient
 * sums: no 4*b*n*m-byte tensor is written or read.
 *   cost[b]                     = what pcc_approxmatch + pcc_matchcost return (float summation order differs);
 *   grad1[b,n,3], grad2[b,m,3]  = what pcc_matchcostgrad_scaled returns; pass both or neither (NULL: cost only);
 *   grad_cost[b] or NULL (= 1).
 * Non-finite coordinates: a NaN propagates through the distances as in the reference; a sample with an infinite
 * coordinate returns NaN cost and NaN gradients (the reference's 0 * sqrt(inf), approxmatch.cu:207,247-248), the other
 * samples of the batch are unaffected.  Failure as for pcc_approxmatch: NaN cost and gradients for the sample. */
int pcc_match_cost(int b, int n, int m, const float *xyz1, const float *xyz2, const float *grad_cost, float *cost,
                   float *grad1, float *grad2, pcc_stream_t stream);

/* ---- sliced Wasserstein distance (extension) -------------------------------------------------------
 * The third set-to-set loss beside Chamfer and the approximate EMD: the squared 2-Wasserstein distance between the two
 * clouds projected onto p directions, averaged.  On a line the optimal transport plan is the sorted order, so the cost of
 * a direction is a sort.  x[b,n,3], y[b,n,3] point-major like the other losses (both clouds have n points); theta[p,3] is
 * shared by the batch and used as given (not normalised).  No counterpart in the reference.  Every word of cost_p and
 * cost is determined by the inputs:
 *   projection  t = (v0 * theta0 + v1 * theta1) + v2 * theta2: three rounded float32 products and two rounded sums, left
 *               to right, no fmaf.  A projection of -0 is taken as +0.
 *   order       the n projections of a cloud ascending; every NaN is one value above +inf; equal values go by ascending
 *               point index.  a_r / b_r: the sorted projections of x / y, pi_x(r) / pi_y(r): the point at rank r.
 *   slice cost  d_r = a_r - b_r, e_r = d_r * d_r; L = the smallest power of two >= n and e_r = +0 for n <= r < L; the
 *               halving tree: for h = L/2, L/4 .. 1: e_i = e_i + e_{i+h} for every i < h; cost_p[b,p] = e_0.
 *   cost        S = ((c_0 + c_1) + c_2) + .. over cost_p[b,:] in ascending p; cost[b] = S * inv, inv = the float32 nearest
 *               to 1 / (n p), formed in double on the host.
 *   gradient    of cost[b] with the permutations held constant: grad_x[b, pi_x(r), c] = (2 inv) * sum_p d_r * theta[p,c]
 *               and grad_y[b, pi_y(r), c] = (2 inv) * sum_p (-d_r) * theta[p,c]; every term is one rounded product, the sum
 *               over p runs in a fixed order that depends on p alone (the projections in ascending order inside chunks of
 *               PCC_SW_CHUNK, then the chunks in ascending order), no float atomics: the words of a cloud's gradient are
 *               the same from run to run and do not depend on b or on the cloud's position in the batch.  Every element of
 *               a requested gradient is written.
 * Any of cost, cost_p, grad_x, grad_y may be NULL; with all four NULL nothing is enqueued.  x and y may alias.
 * Non-finite coordinates: IEEE arithmetic on the order above: a cloud with a NaN coordinate gets a NaN cost, an infinite
 * one an infinite or NaN cost; the other clouds of the batch are unaffected.
 * Requires 1 <= n <= PCC_SW_MAX_N, p >= 1, b <= 65535, b * p < 2^31 and non-null x, y, theta (PCC_EINVAL otherwise, before
 * anything is enqueued); b = 0 enqueues nothing and returns PCC_OK.  64-bit offsets throughout.  Workspace (with
 * p > PCC_SW_CHUNK only: the partial gradients, b * ceil(p / PCC_SW_CHUNK) * n * 3 floats per requested gradient, and cost_p
 * when it is NULL and cost is not) comes from the library's private pool (PCC_ENOMEM if that fails). */
#define PCC_SW_MAX_N 8192
#define PCC_SW_CHUNK 8 /* projections per workgroup */
int pcc_sliced_wasserstein(int b, int n, int p, const float *x, const float *y, const float *theta, float *cost,
                           float *cost_p, float *grad_x, float *grad_y, pcc_stream_t stream);

/* ---- Sinkhorn divergence (extension) ---------------------------------------------------------------
 * The entropic optimal-transport loss between paired clouds, debiased: what GeomLoss's SamplesLoss("sinkhorn", p=2)
 * computes with uniform weights.  x[b,n,3], y[b,m,3] float32, n and m independent; weights a_i = 1/n, b_j = 1/m; pair cost
 * C(u,v) = |u - v|^2 / 2.  T = steps, eps_t = eps[t]: a HOST array of T temperatures (squared lengths), read when the call
 * is enqueued.  No counterpart in the reference.
 *   smoothed minimum   SM_eps(h; U->V)_i = -eps log sum_j exp(-log|V| + (h_j - C(u_i, v_j)) / eps), evaluated with its
 *               largest term subtracted: finite for any finite input and any eps > 0.  C is formed from coordinate
 *               differences, never from the expanded |u|^2 + |v|^2 - 2 u.v.
 *   potentials  f on x against y, g on y against x, p on x against x, q on y against y; all four are updated at once from
 *               the previous values (every launch reads one buffer and writes another):
 *                 initialisation, eps_0:    f = SM(0; x->y), g = SM(0; y->x), p = SM(0; x->x), q = SM(0; y->y)
 *                 t = 0 .. T-1, eps_t:      f <- (f + SM(g; x->y)) / 2, g <- (g + SM(f_old; y->x)) / 2,
 *                                           p <- (p + SM(p; x->x)) / 2, q <- (q + SM(q; y->y)) / 2
 *                 final, eps_{T-1}:         f* = SM(g; x->y), g* = SM(f; y->x), p* = SM(p; x->x), q* = SM(q; y->y)
 *               (not averaged, all from the pre-final values): T + 2 all-pairs rounds, GeomLoss's symmetric scheme with
 *               eps[0] used twice.
 *   outputs     pot_x[b,n] = f* - p*, pot_y[b,m] = g* - q* with debias != 0; f*, g* with debias == 0 (p and q are then never
 *               computed).  cost[b] = inv_n * tree(pot_x[b,:]) + inv_m * tree(pot_y[b,:]): tree = the halving tree of
 *               pcc_sliced_wasserstein (pad with +0 to a power of two L, then for h = L/2 .. 1: e_i = e_i + e_{i+h}); inv_n,
 *               inv_m = the float32 nearest to 1/n, 1/m, formed in double on the host; two products and one sum.
 *   gradients   of cost[b] with the other cloud and the pre-final potentials held constant (GeomLoss's convention):
 *               grad_x[b,i,:] = inv_n (sum_j P_ij (x_i - y_j) - sum_k Pxx_ik (x_i - x_k)), P_i. = the softmax row of the
 *               final x->y round, Pxx that of the final x->x round (dropped with debias == 0); grad_y symmetrically.  They are
 *               accumulated from coordinate differences inside the final round; no plan is stored.
 *   words       no float atomics and a fixed order of every sum, which depends on n and m only: the words of a cloud's
 *               outputs are the same from run to run, at any position of the batch and for any b.
 * Any subset of the five outputs may be NULL; with all five NULL nothing is enqueued.  x and y may alias: with debias != 0
 * the cost and both gradients are then exactly +0 (f and p, g and q are the same function of the same words).
 * Non-finite coordinates: a cloud holding a NaN or an infinite coordinate gets a non-finite cost; the other clouds of
 * the batch are unaffected.
 * Requires 1 <= n, m <= 65536, 1 <= steps <= PCC_SINKHORN_MAX_STEPS, every eps[t] finite and > 0, b <= 65535 and non-null x,
 * y, eps (PCC_EINVAL otherwise, before anything is enqueued); b = 0 enqueues nothing and returns PCC_OK.  64-bit offsets
 * throughout.  Workspace (two generations of the four potentials, the per-row partial sums of the final round) comes
 * from the library's private pool (PCC_ENOMEM if that fails). */
#define PCC_SINKHORN_MAX_STEPS 256
int pcc_sinkhorn(int b, int n, int m, const float *x, const float *y, int steps, const float *eps /* HOST, [steps] */,
                 int debias, float *cost /*[b]*/, float *pot_x /*[b,n]*/, float *pot_y /*[b,m]*/, float *grad_x /*[b,n,3]*/,
                 float *grad_y /*[b,m,3]*/, pcc_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PCC_STRUCTURAL_H */
