/*
 * pcc_neighbour.h -- C ABI of the kNN-graph / neighbour-gather / max-pool primitives in
 * libpcc_structural.so (MI355X / gfx950).
 *
 * The reference has no native boundary for these: they are Python functions in
 * src/utils/neighbour_ops.py that call PyKeOps (GPU) or torch (CPU).  Each entry cites the function it
 * replaces.  Tensors are contiguous row-major device arrays in the reference's layouts:
 *   x[b, c, n] float32 (channels-major), indices[b, n, k] int64.
 * All entries enqueue on `stream` (hipStream_t as void*), never synchronise, and return 0 or an error code
 * (message via pcc_last_error(), include/pcc_structural.h).  ("Never synchronise" with the runtime's one exception that
 * the head of include/pcc_structural.h describes: the second of two workspace-taking calls on a stream that has not yet
 * executed the first; tests/test_gpu_stream_order.py.)
 *
 * Alignment: every tensor argument, input or output, may be any contiguous buffer aligned to its element size -- 4 bytes,
 * 8 for an int64 list (a chunk of a batch, a parameter inside a flat buffer, a slice of a gradient).  The kernels take
 * wider accesses only where the sizes and the address allow it and fall back to element accesses otherwise
 * (tests/test_gpu_unaligned_views.py runs every entry point on such buffers).
 */
#ifndef PCC_NEIGHBOUR_H
#define PCC_NEIGHBOUR_H

#include <stddef.h>
#include <stdint.h>

#include "pcc_structural.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* knn / pykeops_knn (neighbour_ops.py:63-82): for every point the k nearest points of the same cloud in
 * feature space, ascending distance (the point itself first), ties by ascending index.
 *   c <= 3 : exact difference form sum_c (x_j - x_i)^2 on the f32 VALU (the GPU reference's formula, :35-40)
 *   c >= 4 : expanded form |x_i|^2 + |x_j|^2 - 2 x_i.x_j with the inner product on the f32 MFMA pipe
 *            (the reference CPU path's formula, self_square_distance :53-60): (-2*dot + |x_j|^2) + |x_i|^2 with
 *            dot and |x|^2 sequential fma chains over the channel index
 * Any c >= 1; requires 1 <= k <= min(n, 128) (k > 128: PCC_EINVAL).  A NaN distance never enters a list; a list that
 * runs short because of NaN distances is padded with the in-range index n - 1.  A +inf distance (a norm or a squared
 * difference that overflows) is a distance like any other: it is listed, behind the finite ones, in index order. */
int pcc_knn(int b, int c, int n, int k, const float *x, int64_t *indices, pcc_stream_t stream);

/* k-NN between two clouds: for every query q[b, :, i] (q[b, c, nq], channels-major like x) its k nearest candidates of
 * x[b, c, n]: indices[b, nq, k] into x and, when dist is non-null, dist[b, nq, k], the squared distances of those entries.
 * The contract is pcc_knn's with the query taken from q:
 *   c <= 3 : difference form, df = x[ch][j] - q[ch][i], acc = df0 * df0, then fmaf(df, df, acc) in channel order
 *   c >= 4 : expanded form (-2*dot + |x_j|^2) + |q_i|^2, dot and both norms sequential fma chains over the channel index
 * Per query the k candidates ascending by (distance, index); -0 equals +0 (and is reported as +0); a NaN distance never
 * enters a list; a list that runs short because of NaN distances is padded with index n - 1, and dist of a padded slot is
 * NaN; a +inf distance is listed like any other and reported as +inf.  Requires c >= 1, 1 <= k <= min(n, 128), b <= 65535, b * nq < 2^31, and n <= 65535 * 128 when c >= 4
 * (PCC_EINVAL otherwise); nq = 0 or b = 0 enqueues nothing and returns PCC_OK.  64-bit offsets throughout.  Workspace
 * comes from the library's private pool; the distance rows of c >= 4 are capped at 256 MB per launch pair (larger calls
 * run in chunks of samples or of queries).  With few queries and many candidates the candidate axis is searched in slices
 * that are merged afterwards; the result does not depend on it.
 * pcc_knn_cross(b, c, n, n, k, x, x, ...) returns the indices of pcc_knn(b, c, n, k, x, ...) bit for bit, and q and x may
 * alias. */
int pcc_knn_cross(int b, int c, int nq, int n, int k, const float *q, const float *x, int64_t *indices, float *dist,
                  pcc_stream_t stream);

/* Farthest point sampling: m points of every cloud xyz[b, n, 3] (point-major, the layout of the losses and of the
 * set-metric banks), each the point farthest from the ones selected before it: idx[b, m] into the cloud and, when dist is
 * non-null, dist[b, m].  No counterpart in the reference, whose readers draw random subsets on the host.
 *   start     idx[b,0] = start[b], or 0 when start is NULL; a start outside [0, n-1] is clamped into it by the kernel.
 *   mind      every point j has a running minimum mind[j], initially +inf.
 *   update    after selecting s = idx[b,t-1] every j computes d and then `if (d < mind[j]) mind[j] = d`; d is pcc_knn's
 *             c <= 3 form: df = x[j] - x[s] per coordinate, acc = df0 * df0, acc = fmaf(df1, df1, acc),
 *             acc = fmaf(df2, df2, acc).  A NaN d lowers nothing.
 *   select    idx[b,t] = argmax_j mind[j], the lowest index among equal maxima.
 *   dist      dist[b,t] = mind of the selected point at the moment it was selected: the squared coverage radius after t
 *             picks, non-increasing in t, dist[b,0] = +inf.
 *   excluded  a point with a non-finite coordinate is excluded: it is never selected while a point that is not excluded
 *             exists (not even one whose mind is 0); as a start it is written to idx[b,0] as asked and updates nothing;
 *             dist of a selected excluded point (a start included) is NaN; a cloud of excluded points only returns its
 *             start and then index 0 throughout.
 *   equal points need no rule: once every remaining mind is 0 the lowest index with the maximum is returned again.
 * Requires n >= 1, 1 <= m <= n, b <= 65535, non-null xyz and idx (PCC_EINVAL otherwise); b = 0 enqueues nothing and
 * returns PCC_OK.  64-bit offsets throughout; workspace (clouds of more than 16384 points only: b * n floats) comes from
 * the library's private pool.  One workgroup runs the whole chain of a cloud, so a batch of one cloud uses one compute
 * unit.  A cloud's result depends on that cloud, m and its start only: not on b, on the cloud's position in the batch or
 * on the kernel variant that ran. */
int pcc_fps(int b, int n, int m, const float *xyz, const int32_t *start, int64_t *idx, float *dist, pcc_stream_t stream);

/* Ball query: for every centre centres[b, i] (centres[b, m, 3], point-major float32 like xyz and like pcc_fps; centres may
 * alias xyz) the points of xyz[b, n, 3] inside the open ball of `radius` around it, capped at nsample: idx[b, m, nsample]
 * into xyz and, when cnt is non-null, cnt[b, m].  No counterpart in the reference; the query between pcc_fps and a gather
 * in a sampling-and-grouping pipeline.
 *   distance    d is pcc_knn's c <= 3 form with the centre as the query: df = xyz[j] - centres[i] per coordinate,
 *               acc = df0 * df0, acc = fmaf(df1, df1, acc), acc = fmaf(df2, df2, acc).
 *   membership  r2 = radius * radius, one float32 multiplication; point j is inside iff d < r2.  The comparison is strict
 *               (a point on the sphere is outside), so a NaN d is never inside, and neither is a d of +inf: a point or a
 *               centre with a non-finite coordinate has no neighbours and is nobody's neighbour.
 *   selection   the first nsample inside points in ascending index order; cnt[b,i] = min(number inside, nsample): counting
 *               stops at nsample, and so may the scan.
 *   padding     of the slots s >= cnt[b,i]: pad = PCC_BALL_PAD_FIRST: idx[b,i,s] = idx[b,i,0], and index 0 when the ball
 *               is empty (the set-abstraction convention: every slot is an in-range index and can be gathered without a
 *               mask); pad = PCC_BALL_PAD_NONE: -1.
 * Requires n >= 1, nsample >= 1 (it may exceed n), radius > 0 (NaN, 0 and negative: PCC_EINVAL; +inf is allowed: every
 * point at a finite distance is inside, and so is every radius whose square overflows), pad 0 or 1, b <= 65535,
 * b * m < 2^31, non-null xyz, centres and idx (PCC_EINVAL otherwise); b = 0 or m = 0 enqueues nothing and returns PCC_OK.
 * 64-bit offsets throughout, no workspace.  A query's row depends on its cloud, its centre, radius, nsample and pad only:
 * not on b, m, its position in the batch or the kernel variant that ran.  pcc_group_points gathers along the list, either
 * pad included (pcc_gather_neighbours cannot: it takes one index row per point of the cloud it reads). */
enum { PCC_BALL_PAD_FIRST = 0, PCC_BALL_PAD_NONE = 1 };
int pcc_ball_query(int b, int n, int m, int nsample, float radius, int pad, const float *xyz, const float *centres,
                   int64_t *idx, int32_t *cnt, pcc_stream_t stream);

/* Ragged batches: k-NN and ball query over packed clouds.  A packed batch is one xyz[n, 3] (point-major float32) that holds
 * the clouds of the batch end to end, and offset[b] int32, their cumulative ends: cloud c is the rows
 * [offset[c-1], offset[c]).  The queries (query[m, 3] with query_offset[b]; centres[m, 3] with centre_offset[b]) are packed
 * the same way and may alias the points.  The layout of the published pointops package; no counterpart in the reference.
 *   clouds      Every offset is clipped by the kernel and never trusted: lo_b = min(max(offset[b-1], 0), n) with
 *               offset[-1] = 0, and hi_b = min(max(offset[b], lo_b), n).  The query side is clipped the same way against m.
 *               Query row i belongs to the cloud whose clipped query range holds it.  A row behind the last range belongs
 *               to no cloud.  A cloud may have no points or no queries.  Offsets stay on the device.  The entry points read
 *               none of them on the host.  They need no host synchronisation and no workspace, so there is no pool
 *               allocation.  The grid is a function of m alone.
 *   indices     Indices are global: idx points into the packed xyz, so lo_b <= idx < hi_b for a real slot.  A row's words
 *               depend only on its own cloud's points, the query, and k or (radius, nsample, pad), plus the base lo_b that
 *               is added.  They do not depend on b, on where the cloud lies in the packed array, or on what else shares
 *               the workgroup.
 *   k-NN        The distance is pcc_knn's c <= 3 form with the query as in pcc_knn_cross: df = xyz[j] - query[i],
 *               acc = df0 * df0, then two fmaf.  Each row is ascending by (distance, index).  -0 equals +0 and is reported
 *               as +0.  A NaN distance is never listed.  +inf is listed like any other value.  A row that runs short is
 *               completed with idx = -1, dist = +inf.  Short rows come from a cloud with fewer than k points, from NaN
 *               distances, from a NaN query, or from a row of no cloud.  This deliberately differs from pcc_knn_cross's
 *               n - 1 / NaN, because here k may exceed the cloud and -1 is what every list op skips.  The weight
 *               1 / (+inf + eps) of such a slot is 0.  Requires 1 <= k <= 32 in this version.  k > 32 returns PCC_EINVAL
 *               with a message that says so.  b <= 65535.  64-bit element offsets throughout.  b = 0 or m = 0 enqueues
 *               nothing and returns PCC_OK.  n = 0 with m > 0 is allowed: every row is padding.  For a cloud with
 *               hi_b - lo_b >= k and no NaN, idx - lo_b and dist are bit for bit what pcc_knn_cross(1, 3, m_b, n_b, k, ...)
 *               returns for that cloud alone.  idx[m, k], and dist[m, k] when dist is non-null.
 *   ball query  Per cloud this is exactly pcc_ball_query's rule: r2 = radius * radius in float32, a strict d < r2, the
 *               first nsample inside points in ascending index, cnt, and pad FIRST / NONE.  With FIRST an empty ball is
 *               filled with lo_b, the cloud's first point.  A row of no cloud or of an empty cloud gets cnt = 0 and -1
 *               throughout, whatever pad is.  The argument checks are the same as pcc_ball_query's.  For every cloud,
 *               idx - lo_b (real and FIRST-padded slots) and cnt are word for word pcc_ball_query(1, n_b, m_b, ...).
 *               idx[m, nsample], and cnt[m] when cnt is non-null.
 *   alignment   Every tensor argument may be any buffer aligned to its element size (the alignment paragraph above).
 * Every query of a workgroup scans the union of the workgroup's clouds exhaustively: there is no culling and no split of
 * the candidates for few queries over a huge cloud (it would need a workspace). */
int pcc_knn_ragged(int b, int n, int m, int k, const float *xyz, const int32_t *offset, const float *query,
                   const int32_t *query_offset, int64_t *idx, float *dist, pcc_stream_t stream);
int pcc_ball_query_ragged(int b, int n, int m, int nsample, float radius, int pad, const float *xyz, const int32_t *offset,
                          const float *centres, const int32_t *centre_offset, int64_t *idx, int32_t *cnt,
                          pcc_stream_t stream);

/* Grouping: the gather along an index list that belongs to another point set, idx[b, m, k] int64 into a cloud of n points
 * (m != n allowed): the lists of pcc_ball_query around the centres of pcc_fps, or of pcc_knn_cross.  No counterpart in the
 * reference; what a user writes in torch instead is an expanded index tensor, a gather per input, a subtraction and a cat.
 *   layouts     point_major = 0: x[b, c, n], centre[b, c, m], grad_x[b, c, n], grad_centre[b, c, m] (the feature layout of
 *               the graph ops); point_major = 1: x[b, n, c], centre[b, m, c] and the gradients alike (the xyz layout of
 *               pcc_fps, pcc_ball_query and the losses).  out and grad_out are always channels-major [b, out_c, m, k], and a
 *               call touches their channels out_c0 .. out_c0 + c - 1 only: two calls fill one [b, 3 + C, m, k] tensor
 *               without a cat, and the backward reads its slice of the gradient in place.
 *   forward     out[b, out_c0 + ch, i, j] = x[b, ch, idx[b, i, j]], a copy of the float's bits (NaN payloads included); with
 *               a non-null centre x[b, ch, idx[b, i, j]] - centre[b, ch, i], one float32 subtraction.  A slot whose index
 *               is outside [0, n) (the -1 of PCC_BALL_PAD_NONE) is +0.0 in both modes.
 *   backward    grad_x[b, ch, t] = sum of grad_out[b, out_c0 + ch, i, j] over the slots with idx[b, i, j] == t; every
 *               element of grad_x is written, +0.0 where nothing points.  grad_centre[b, ch, i] = -(sum over the in-range
 *               slots j of grad_out[b, out_c0 + ch, i, j]), summed in a fixed order.  A slot outside [0, n) carries no
 *               gradient to either.  Either gradient pointer may be null; with both null nothing is enqueued.  grad_x is
 *               accumulated with float atomics (LDS bins, or global memory where a cloud's bins do not fit LDS) after the
 *               runs of equal consecutive indices have been summed inside a wave: like pcc_gather_neighbours_bwd and
 *               torch's scatter_add, the float summation order of grad_x is not fixed.
 * Requires c >= 1, n >= 1, k >= 1, m >= 0, 0 <= out_c0, out_c0 + c <= out_c, point_major 0 or 1, b <= 65535,
 * m * k < 2^31 and non-null x, idx, out / idx, grad_out (PCC_EINVAL otherwise, under "group_points:" /
 * "group_points_bwd:"); centre may be null.  b = 0 enqueues nothing and returns PCC_OK; m = 0: the forward enqueues nothing,
 * the backward zero-fills grad_x.  64-bit offsets throughout, no workspace, and no n is refused: where not even one channel
 * row of a cloud fits a workgroup's LDS (n > 40960) the gathers and the atomics go to global memory.  A row of the output
 * depends on its cloud, its index row and its centre only: not on b, m, its position in the batch or the variant that ran. */
int pcc_group_points(int b, int c, int n, int m, int k, int point_major, const float *x, const int64_t *idx,
                     const float *centre, float *out, int out_c, int out_c0, pcc_stream_t stream);
int pcc_group_points_bwd(int b, int c, int n, int m, int k, int point_major, const int64_t *idx, const float *grad_out,
                         int out_c, int out_c0, float *grad_x, float *grad_centre, pcc_stream_t stream);

/* Feature propagation: every one of m dense points becomes the weighted sum of the features of the k sparse points its list
 * names: idx[b, m, k] int64 into a cloud of n points (the list of pcc_knn_cross with the dense points as queries), w[b, m, k]
 * float32 (inverse-distance weights, or any others).  No counterpart in the reference; what a user writes in torch instead
 * is an expanded gather of [b, c, m, k], a multiplication and a sum over k.
 *   layouts     x[b, c, n] and grad_x[b, c, n] channels-major (the feature layout of the graph ops).  out and grad_out are
 *               [b, out_c, m], and a call touches their channels out_c0 .. out_c0 + c - 1 only (the slice convention of
 *               pcc_group_points): the skip features are concatenated without a cat of the interpolated half.
 *   forward     out[b, out_c0 + ch, i]: acc = +0.0f, then for j = 0 .. k - 1 in order acc = acc + (w[b, i, j] *
 *               x[b, ch, idx[b, i, j]]): one float32 multiplication and one float32 addition per slot, two roundings, not an
 *               fmaf.  A slot whose index is outside [0, n) is skipped: it adds nothing, whatever its weight (a NaN
 *               included), and carries no gradient.  Everything else is IEEE: 0 * inf is NaN, NaN weights propagate.  IEEE
 *               leaves the sign and payload of a NaN result open, so a NaN acc is written as the word 0x7fc00000.  Every
 *               output word is determined by x, the point's index row and its weight row: it does not depend on b, m, the
 *               position in the batch or the variant that ran.
 *   backward    grad_x[b, ch, t] = sum of w[b, i, j] * grad_out[b, out_c0 + ch, i] (one rounded product per slot) over the
 *               in-range slots with idx[b, i, j] == t; every element of grad_x is written, +0.0 where nothing points.  The
 *               products are accumulated with float atomics (LDS bins, or global memory where a cloud's bins do not fit
 *               LDS), as in pcc_group_points_bwd: the float summation order of grad_x is not fixed.
 *               grad_w[b, i, j]: acc = +0.0f, then for ch = 0 .. c - 1 in order acc = acc + (grad_out[b, out_c0 + ch, i] *
 *               x[b, ch, idx[b, i, j]]): a fixed order, so the words are determined (up to the payload of a NaN); +0.0 for a
 *               slot outside [0, n).  Either gradient pointer may be null; with both null nothing is enqueued; x may be
 *               null when grad_w is.
 * Requires c >= 1, n >= 1, k >= 1, m >= 0, 0 <= out_c0, out_c0 + c <= out_c, b <= 65535, m * k < 2^31 and non-null x, idx,
 * w, out / idx, w, grad_out (PCC_EINVAL otherwise, under "interpolate:" / "interpolate_bwd:", before anything is enqueued).
 * b = 0 enqueues nothing and returns PCC_OK; m = 0: the forward enqueues nothing, the backward zero-fills grad_x.  64-bit
 * offsets throughout, no workspace, and no n is refused: where not even one channel row of a cloud fits a workgroup's LDS
 * (n > 40960) the gathers and the atomics go to global memory. */
int pcc_interpolate(int b, int c, int n, int m, int k, const float *x, const int64_t *idx, const float *w, float *out,
                    int out_c, int out_c0, pcc_stream_t stream);
int pcc_interpolate_bwd(int b, int c, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                        const float *grad_out, int out_c, int out_c0, float *grad_x, float *grad_w, pcc_stream_t stream);

/* Vector attention (Point Transformer; the aggregation published implementations ship as pointops.aggregation): a softmax
 * over the k slots of every row of a list that leaves out the slots the list has padded, and a weighted sum over the
 * neighbourhood in which S = c / g consecutive channels share one weight and the values are gathered inside the kernel.
 * No counterpart in the reference; what a user writes in torch instead materialises the gathered values, their sum with
 * the position encoding and the product, three tensors of [b, c, m, k], and a masked_fill in front of the softmax.
 *   layouts     x[b, c, n] and grad_x[b, c, n] channels-major; idx[b, m, k] int64 into the n points (m != n allowed: the list
 *               of pcc_knn, pcc_knn_cross or pcc_ball_query); w, logits, attn and their gradients [b, g, m, k]; rel and
 *               grad_rel [b, c, m, k], the layout pcc_group_points writes; out and grad_out [b, c, m].  float32 throughout.
 *               The group of channel ch is ch / S: the S channels of a group are consecutive.
 *   valid slots a slot is valid iff its index is in [0, n).  An invalid slot (the -1 of PCC_BALL_PAD_NONE) takes no part
 *               in any sum, carries no gradient, whatever its weight, logit or rel word (a NaN included), and is +0.0
 *               wherever a per-slot output is written.  A NaN result is written as the word 0x7fc00000.
 *   pcc_neighbour_softmax      per row (b, gi, i): mx = the largest logit over the valid slots, e_j = exp(l_j - mx) in
 *               float32 (one rounded difference), s = the sum of the e_j over the valid slots in slot order from +0.0,
 *               attn_j = e_j / s, one division.  A row without a valid slot is all +0.0.  Non-finite logits behave as
 *               torch.softmax restricted to the valid slots: a NaN, or a +inf maximum, makes the row's valid slots NaN, a
 *               -inf slot beside a finite maximum is 0, a row whose valid logits are all -inf is NaN.  The words of exp are
 *               not fixed by this contract (the device library's expf, 1 ulp); the order of the sum is, so every variant
 *               returns the same words.  The tests bound attn against float64: |attn_j - ref_j| <= ((k + 8 + 4 |l_j - mx|)
 *               2^-24) ref_j + 2^-126.
 *   pcc_neighbour_softmax_bwd  d = the sum of (attn_j * grad_attn_j) over the valid slots in slot order from +0.0, a rounded
 *               product and a rounded sum each; grad_logits_j = attn_j * (grad_attn_j - d), a rounded difference and a
 *               rounded product.  The words are fixed.
 *   pcc_aggregate_points       out[b, ch, i]: acc = +0.0f, then for every valid slot j in order v = x[b, ch, idx[b, i, j]]
 *               (with a non-null rel v = x[b, ch, idx[b, i, j]] + rel[b, ch, i, j], one rounded sum) and acc = acc +
 *               (w[b, ch / S, i, j] * v): a rounded product, then a rounded sum, not an fmaf.  The words are fixed; with
 *               g = 1 and a null rel they are those of pcc_interpolate.  The weights are any numbers, not only the
 *               output of the softmax.
 *   pcc_aggregate_points_bwd   any subset of the three outputs; a null one costs nothing, all three null enqueue nothing.
 *               grad_rel[b, ch, i, j] = w[b, ch / S, i, j] * grad_out[b, ch, i], one rounded product; every word is written,
 *               the words are fixed; rel is not read.  grad_x[b, ch, t] = the sum of those same products over the valid
 *               slots with idx[b, i, j] == t; every element is written, +0.0 where nothing points.  It is accumulated
 *               with float atomics (LDS bins, or global memory where a cloud's bins do not fit LDS) after the runs of
 *               equal consecutive indices have been summed inside a wave, as in pcc_group_points_bwd: the float summation
 *               order of grad_x is not fixed.  grad_w[b, gi, i, j]: acc = +0.0f, then over the channels ch of the group in
 *               ascending order acc = acc + (grad_out[b, ch, i] * v) with v as in the forward; the words are fixed.  x and
 *               rel are read for grad_w only: x may be null when grad_w is.
 * Every output word depends on the row's own inputs only: not on b, m, the position in the batch or the variant that ran.
 * Requires c >= 1, g >= 1, c % g == 0, n >= 1, 1 <= k <= 128 (what the searches return), m >= 0, b <= 65535, m * k < 2^31
 * (PCC_EINVAL otherwise, under "neighbour_softmax:" / "neighbour_softmax_bwd:" / "aggregate_points:" /
 * "aggregate_points_bwd:", sizes before pointers, before anything is enqueued) and non-null idx, logits, attn / idx, attn,
 * grad_attn, grad_logits / x, idx, w, out / idx, w, grad_out; rel may be null.  b = 0 enqueues nothing and returns PCC_OK;
 * m = 0: the forwards enqueue nothing, the backward zero-fills grad_x.  64-bit offsets throughout, no workspace, no host
 * synchronisation, and no n is refused: where a channel row of a cloud does not fit a workgroup's LDS beside the forward's
 * tile (n > 39424; for the bins of grad_x n > 40960) the gathers and the atomics go to global memory. */
int pcc_neighbour_softmax(int b, int g, int n, int m, int k, const int64_t *idx, const float *logits, float *attn,
                          pcc_stream_t stream);
int pcc_neighbour_softmax_bwd(int b, int g, int n, int m, int k, const int64_t *idx, const float *attn, const float *grad_attn,
                              float *grad_logits, pcc_stream_t stream);
int pcc_aggregate_points(int b, int c, int g, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                         const float *rel, float *out, pcc_stream_t stream);
int pcc_aggregate_points_bwd(int b, int c, int g, int n, int m, int k, const float *x, const int64_t *idx, const float *w,
                             const float *rel, const float *grad_out, float *grad_x, float *grad_w, float *grad_rel,
                             pcc_stream_t stream);

/* Kernel point convolution (rigid KPConv, Thomas et al. 2019): the features of the neighbours a list names, weighted by the
 * influence of each of kp kernel points on each neighbour and summed per kernel point.  The convolution proper is then
 * W.view(O, kp * c) @ out, one batched GEMM that stays with the caller.  No counterpart in the reference; what a user writes
 * in torch instead gathers [b, c, m, k] and [b, m, k, 3], forms [b, m, k, kp, 3] differences and a matmul per centre.
 *   layouts     xyz[b, n, 3] and centres[b, m, 3] point-major (the layout of pcc_fps and pcc_ball_query); idx[b, m, k] int64
 *               into the n points (m != n allowed); x[b, c, n] and grad_x[b, c, n] channels-major; kernel_points[kp, 3],
 *               shared by the batch; out and grad_out [b, kp * c, m], channel t * c + ch belonging to kernel point t.
 *               float32 throughout.
 *   valid slots a slot is valid iff its index is in [0, n): the -1 of PCC_BALL_PAD_NONE and KPConv's shadow index n are
 *               not.  An invalid slot takes no part in anything.
 *   influence   inv = 1.0f / sigma, computed once on the host in float32.  For a valid slot j of centre i and kernel point
 *               t, every operation float32 and rounded, no fmaf (the file is built with -ffp-contract=off):
 *               r_a = xyz[b, idx[b, i, j], a] - centres[b, i, a]; e_a = r_a - kernel_points[t, a];
 *               d2 = (e_x * e_x + e_y * e_y) + e_z * e_z; d = sqrtf(d2), correctly rounded; v = 1.0f - d * inv;
 *               h = v > 0 ? v : +0.0 (KPConv's "linear" influence).  A NaN or infinite distance therefore gives h = +0.0.
 *               The words of h are fixed.
 *   forward     out[b, t * c + ch, i]: acc = +0.0f, then over the valid slots in slot order, for every pair with h > 0,
 *               acc = acc + (h * x[b, ch, idx[b, i, j]]): a rounded product, then a rounded sum.  A pair with h = +0.0 is
 *               skipped by definition, whatever the feature word, a NaN included.  Elsewhere IEEE holds; a NaN result is
 *               written as the word 0x7fc00000.  The words are fixed: every output word depends on the row's own inputs
 *               only, not on b, m, the position in the batch or the variant that ran.
 *   backward    per valid slot and channel p = +0.0f, then over t ascending, for the pairs with h > 0,
 *               p = p + (h * grad_out[b, t * c + ch, i]).  grad_x[b, ch, u] = the sum of the words p over the valid slots
 *               with idx[b, i, j] == u; every element is written, +0.0 where nothing points.  It is accumulated with float
 *               atomics (LDS bins, or global memory where a cloud's bins do not fit LDS) after the runs of equal
 *               consecutive indices have been summed inside a wave, as in pcc_aggregate_points_bwd: only this order is not
 *               fixed.  Coordinates and kernel points carry no gradient.
 * Other contracts, not this one: deformable KPConv (kernel points per centre, gradients in the coordinates), the Gaussian
 * and constant influences, the division by the neighbour count, and the GEMM fused into the kernel.
 * Requires c >= 1, n >= 1, k >= 1, m >= 0, b <= 65535, m * k < 2^31 (the messages of the other list ops), then 1 <= kp <= 32
 * ("kernel points must be 1..32"), k <= 128 ("k > 128"), sigma finite and > 0 ("sigma must be finite and > 0"), then
 * non-null pointers ("null pointer"): PCC_EINVAL otherwise, under "kpconv_aggregate:" / "kpconv_aggregate_bwd:", sizes before
 * pointers, before anything is enqueued.  b = 0 enqueues nothing and returns PCC_OK; m = 0: the forward enqueues nothing, the
 * backward zero-fills grad_x.  64-bit offsets throughout, no workspace, no host synchronisation, and no n is refused: the
 * forward gathers the features of the pairs with h > 0 from global memory for every n, and where the bins of a channel of
 * grad_x do not fit a workgroup's LDS (n > 40960) the backward's atomics go to global memory. */
int pcc_kpconv_aggregate(int b, int c, int n, int m, int k, int kp, const float *xyz, const float *centres,
                         const int64_t *idx, const float *x, const float *kernel_points, float sigma, float *out,
                         pcc_stream_t stream);
int pcc_kpconv_aggregate_bwd(int b, int c, int n, int m, int k, int kp, const float *xyz, const float *centres,
                             const int64_t *idx, const float *kernel_points, float sigma, const float *grad_out,
                             float *grad_x, pcc_stream_t stream);

/* Local surface geometry: for every row of an index list idx[b, m, k] int64 into the cloud xyz[b, n, 3] (point-major float32,
 * the layout of pcc_fps and pcc_ball_query; m != n allowed: the list of pcc_knn, pcc_knn_cross or pcc_ball_query) the mean of
 * the points it names, their scatter matrix, its eigen-decomposition and the surface variation: mean[b, m, 3],
 * cov[b, m, 3, 3], eval[b, m, 3], evec[b, m, 3, 3], curv[b, m].  The fused form of the reference's get_local_covariance
 * (neighbour_ops.py:97-103: gather, subtract the mean, matmul) and of the torch.linalg.eigh a user runs on its result for
 * normals.  Every output pointer may be null: only what is asked for is computed and written (eval, evec and curv need the
 * scatter matrix but not its store); with all five null nothing is enqueued.
 *   valid slots a slot is valid iff its index is in [0, n); cnt is the number of valid slots of the row.  The -1 of
 *               PCC_BALL_PAD_NONE is skipped, as in pcc_group_points and pcc_interpolate.  A repeated index counts as often
 *               as it occurs, so a PCC_BALL_PAD_FIRST list weighs its first point by the padding: PCC_BALL_PAD_NONE is the
 *               unbiased choice.
 *   mean        per coordinate acc = +0.0f, then acc = acc + x over the valid slots in slot order, then one float32 division
 *               by (float)cnt; +0.0 if cnt = 0.
 *   cov         the scatter matrix, NOT divided by cnt (the reference's convention).  d_j = x_j - mean, one float32
 *               subtraction per coordinate; for a <= b acc = +0.0f, then acc = acc + (d_a * d_b) over the valid slots in slot
 *               order: a rounded product and a rounded sum, not an fmaf.  The lower triangle is a copy of the upper one.
 *               A NaN in mean or cov is written as the word 0x7fc00000 (the convention of pcc_interpolate).  Every word of
 *               mean and cov is determined by the cloud and the index row: it does not depend on b, m, the position in the
 *               batch or the variant that ran.
 *   eval, evec  the eigenvalues of the scatter matrix in ascending order; evec[b, i, r, :] is the unit eigenvector of
 *               eval[b, i, r], so row 0 is the surface normal.  Sign: the component of largest magnitude of each row is
 *               non-negative, the lowest axis deciding a tie.  An axis whose two off-diagonal entries are exactly 0 is
 *               decoupled: its unit vector is returned exactly and its eigenvalue is the diagonal entry.  A zero matrix
 *               (cnt <= 1) gives eigenvalues +0.0 and the rows e_x, e_y, e_z.  A non-finite entry of the scatter matrix
 *               makes eval, evec and curv of the row the word 0x7fc00000.  The words of these three outputs depend on the
 *               row's scatter matrix only.  They are not pinned to a CPU formula (a cyclic Jacobi iteration in float32 on
 *               the matrix scaled by a power of two); the tests bound them against float64: residual and eigenvalue error
 *               <= 64 * 2^-24 * |S|_F, |V V^T - I| <= 64 * 2^-24.
 *   curv        the surface variation max(eval0, 0) / (eval0 + eval1 + eval2), taken on the scaled matrix (the scale
 *               cancels); +0.0 where the sum is not positive.
 *   backward    pcc_local_covariance_bwd: the gradient of cov and mean in xyz.  Gs = grad_cov + grad_cov^T, one rounded sum
 *               per entry; gm = grad_mean / (float)cnt, one division per coordinate, absent when grad_mean is null.  For
 *               every valid slot grad_xyz[b, idx[b,i,j], a] += ((Gs_a0 * d_0 + Gs_a1 * d_1) + Gs_a2 * d_2) + gm_a with d
 *               recomputed from xyz and the saved mean (the mean's own contribution through d cancels: sum_j d_j = 0).
 *               Every element of grad_xyz is written, +0.0 where nothing points.  The terms are accumulated with float
 *               atomics (LDS bins where a cloud's 3 * n floats fit beside the index tile, global memory otherwise) after the
 *               runs of equal consecutive indices of a row have been summed: as in pcc_group_points_bwd the float summation
 *               order of grad_xyz is not fixed.  A null grad_xyz enqueues nothing.
 * Requires n >= 1, k >= 1, m >= 0, b <= 65535, m * k < 2^31 and non-null xyz and idx, for the backward also mean and
 * grad_cov (PCC_EINVAL otherwise, under "local_geometry:" / "local_covariance_bwd:", before anything is enqueued).  b = 0 or
 * m = 0 returns PCC_OK; the backward zero-fills grad_xyz for m = 0.  64-bit offsets throughout, no workspace, and no n is
 * refused. */
int pcc_local_geometry(int b, int n, int m, int k, const float *xyz, const int64_t *idx, float *mean, float *cov,
                       float *eval, float *evec, float *curv, pcc_stream_t stream);
int pcc_local_covariance_bwd(int b, int n, int m, int k, const float *xyz, const int64_t *idx, const float *mean,
                             const float *grad_cov, const float *grad_mean, float *grad_xyz, pcc_stream_t stream);

/* The point-voxel branch (PVCNN): point features averaged into a dense grid of res^3 cells per cloud, and a grid read back
 * at the points by trilinear interpolation.  No counterpart in the reference; what a user writes in torch instead is an
 * index_add_ mean and eight gathers of [b, c, n].  The grid is pcc_occupancy_grid's (include/pcc_structural.h): res points
 * per axis over [lo, lo + extent]^3, inv = (float)(res - 1) / extent rounded once on the host.
 *   layouts     x[b, c, n], out[b, c, n] channels-major; xyz[b, n, 3]; grid[b, c, res, res, res] with the flat cell
 *               (i * res + j) * res + k; cell[b, n], order[b, n], counts[b, res^3] int32.  float32 and 64-bit offsets
 *               throughout.  Coordinates carry no gradient in any of the five functions.
 *   pcc_voxel_index   cell[b, p]: the flat cell of pcc_occupancy_grid with in_sphere = 0, rounding by rounding (t = (x - lo) *
 *               inv, floorf(t + 0.5f) clamped to [0, res - 1] as a float: a midpoint goes up), -1 for a point with a NaN or
 *               infinite coordinate.  counts[b, cell]: the points of cloud b in the cell, every element written, word for
 *               word what pcc_occupancy_grid(per_cloud = 1) returns.  order[b, :]: a permutation of 0 .. n - 1, the finite
 *               points first, ascending by (cell, point index), the non-finite ones behind them in index order.  Every word
 *               of the three outputs is fixed by the cloud alone: not by b, the position in the batch, the variant or the run.
 *               n <= 16384 (a cloud is sorted by one workgroup in LDS).
 *   pcc_voxelize      for every cell and channel acc = +0.0f, then acc = acc + x[b, ch, p] over the cell's points in ascending
 *               point index, then grid = acc / (float)count: one IEEE division.  An empty cell is +0.0, a NaN result the word
 *               0x7fc00000.  Every word of the dense grid is written exactly once and there are no float atomics, so the
 *               words are fixed.  cell, order and counts are those of pcc_voxel_index for the same cloud and res.  Takes
 *               b * res^3 * 4 bytes from the library's stream-ordered workspace.
 *   pcc_voxelize_bwd  grad_x[b, ch, p] = grad_grid[b, ch, cell] / (float)counts[cell], one division; +0.0 for cell = -1.  A
 *               gather: the words are fixed.
 *   pcc_devoxelize    per axis of a finite point t = fminf(fmaxf((x - lo) * inv, 0), res - 1) (two roundings, then the
 *               clamp: a point outside the cube reads the border), i0 = min((int)floorf(t), res - 2), f = t - (float)i0
 *               (exact), w1 = f, w0 = 1.f - f.  The weight of corner (di, dj, dk) is (wx * wy) * wz, two rounded products.
 *               out[b, ch, p]: acc = +0.0f, then over the corners 000, 001, 010, ... 111 acc = acc + (w * grid[corner]), a
 *               rounded product and a rounded sum each, not an fmaf.  A NaN result is the word 0x7fc00000; a non-finite
 *               point gives +0.0 and carries no gradient.  Every word is fixed by the point, the grid row and the scalars.
 *   pcc_devoxelize_bwd  grad_grid[b, ch, cell] = sum of w * grad_out[b, ch, p] (one rounded product, the forward's w) over
 *               the finite points and their corners; every element is written, +0.0 where nothing points.  The products are
 *               accumulated with float atomics (LDS bins streamed out whole for res <= 32, a zero fill and global atomics
 *               above): as in pcc_group_points_bwd the float summation order of this one output is not fixed.
 * Requires c >= 1, n >= 1, 2 <= res <= 128, extent finite and > 0 with a finite positive inv, lo finite, b <= 65535,
 * b * n <= INT_MAX, b * res^3 <= INT_MAX and non-null pointers (PCC_EINVAL otherwise, under "voxel_index:", "voxelize:",
 * "voxelize_bwd:", "devoxelize:", "devoxelize_bwd:", before anything is enqueued).  b = 0 enqueues nothing and returns
 * PCC_OK.  No host synchronisation: the calls can be captured into a graph. */
int pcc_voxel_index(int b, int n, const float *xyz, int res, float lo, float extent, int32_t *cell, int32_t *order,
                    int32_t *counts, pcc_stream_t stream);
int pcc_voxelize(int b, int c, int n, int res, const float *x, const int32_t *cell, const int32_t *order,
                 const int32_t *counts, float *grid, pcc_stream_t stream);
int pcc_voxelize_bwd(int b, int c, int n, int res, const int32_t *cell, const int32_t *counts, const float *grad_grid,
                     float *grad_x, pcc_stream_t stream);
int pcc_devoxelize(int b, int c, int n, int res, float lo, float extent, const float *grid, const float *xyz, float *out,
                   pcc_stream_t stream);
int pcc_devoxelize_bwd(int b, int c, int n, int res, float lo, float extent, const float *xyz, const float *grad_out,
                       float *grad_grid, pcc_stream_t stream);

/* Grid pooling (Point Transformer V2's partition-based pooling, KPConv's grid subsampling): the sparse form of pcc_voxelize,
 * one output slot per OCCUPIED cell of the grid of pcc_voxel_index instead of a dense res^3 grid.  No counterpart in the
 * reference; what a user writes in torch instead is a torch.unique over b * res^3 + cell (a global sort and a host
 * synchronisation for the output size) and a scatter_reduce_ (float atomics).  The output is ragged -- every cloud has its
 * own number U of occupied cells -- and is padded to a capacity m the caller chooses: a padded slot has an empty run.
 *   layouts     cell[b, n], order[b, n] int32: those of pcc_voxel_index for the cloud; cluster[b, n], seg[b, m + 1], n_cells[b]
 *               int32; x[b, c, n], grad_x[b, c, n], out[b, c, m], grad_out[b, c, m] float32 channels-major, arg[b, c, m] int32.
 *               64-bit offsets throughout.
 *   pcc_grid_cluster   U: the number of distinct cells >= 0 of the cloud, F: the number of its finite points (the first F
 *               entries of order).  The occupied cells are ranked 0 .. U - 1 in ascending cell.  cluster[b, p]: the rank of
 *               the cell of point p if that rank is < m; -1 for a dropped rank (>= m) and for cell = -1.  seg[b, r], r <
 *               min(U, m): the first sorted position of rank r's run; every later entry up to seg[b, m]: the end of the last
 *               kept run, F when U <= m and the first position of rank m otherwise.  So run r is order[seg[r] : seg[r + 1]],
 *               in ascending point index, and a padded slot's run is empty.  n_cells[b] = U, the true count: U > m is how a
 *               caller sees that cells were dropped.  The outputs at capacity m are those at capacity n restricted to their
 *               first m (+ 1) entries, apart from the -1 of the dropped ranks.  Integers only: every word is fixed by the
 *               cloud alone, not by b, the position in the batch or the run.  order is trusted to be pcc_voxel_index's (as in
 *               pcc_voxelize: an entry outside [0, n) is skipped, never dereferenced).  n <= 16384 (pcc_voxel_index's limit:
 *               one workgroup scans a cloud).
 *   pcc_segment_pool   per slot r and channel over the run order[seg[r] : seg[r + 1]], in ascending position:
 *               mode 0, mean  acc = +0.0f, then acc = acc + x[b, ch, order[pos]], then acc / (float)len, one IEEE division:
 *                             word for word what pcc_voxelize writes into that cell;
 *               mode 1, sum   the same without the division;
 *               mode 2, max   torch.max over the run: the first NaN wins; otherwise the greatest value, the lowest point
 *                             index among equal ones (-0 equals +0).  out is the word of x[b, ch, arg] (a NaN keeps its
 *                             payload) and arg[b, ch, r] that point index; arg may be null, and is written in mode 2 only.
 *               An empty run gives +0.0 and arg = -1.  A NaN from a mean or a sum is the word 0x7fc00000.  No float atomics:
 *               every word of out and arg is written exactly once and is fixed by x, order and seg.  A run of more than 64
 *               points is summed by one wave with a lane per channel, so a cell holding the whole cloud costs n wave steps.
 *   pcc_segment_pool_bwd   a gather: with r = cluster[b, p], grad_x[b, ch, p] = grad_out[b, ch, r] / (float)(seg[r + 1] -
 *               seg[r]) (mean, one division), grad_out[b, ch, r] (sum), grad_out[b, ch, r] where arg[b, ch, r] == p and +0.0
 *               elsewhere (max); +0.0 for r = -1.  Every word is written and fixed.
 * Requires c >= 1, n >= 1 (pcc_grid_cluster: n <= 16384), 1 <= m <= n, mode in {0, 1, 2}, b <= 65535, b * (n + 1) < 2^31 and
 * non-null pointers (arg: in pcc_segment_pool_bwd with mode 2 only) -- PCC_EINVAL otherwise, under "grid_cluster:",
 * "segment_pool:", "segment_pool_bwd:", before anything is enqueued.  b = 0 enqueues nothing and returns PCC_OK.  No c is
 * refused (the kernels stride over the channel blocks beyond 65535 launch rows).  No workspace and no host synchronisation:
 * the calls can be captured into a graph. */
int pcc_grid_cluster(int b, int n, int m, const int32_t *cell, const int32_t *order, int32_t *cluster, int32_t *seg,
                     int32_t *n_cells, pcc_stream_t stream);
int pcc_segment_pool(int b, int c, int n, int m, int mode, const float *x, const int32_t *order, const int32_t *seg,
                     float *out, int32_t *arg, pcc_stream_t stream);
int pcc_segment_pool_bwd(int b, int c, int n, int m, int mode, const int32_t *cluster, const int32_t *seg,
                         const int32_t *arg, const float *grad_out, float *grad_x, pcc_stream_t stream);

/* Ragged grid pooling: the index of pcc_grid_cluster for a whole packed batch (the layout of pcc_knn_ragged) with clouds of
 * any size and up to 2^16 cells per axis -- the partition of Point Transformer V2 / V3's GridPool, of KPConv's grid
 * subsampling and of the sparse-convolution front ends on scenes.  No counterpart in the reference; what a user writes in
 * torch instead is a key, torch.unique(sorted, return_inverse, return_counts) and a scatter_reduce_.
 *   layouts     xyz[n, 3] float32 packed, offset[b] int32 cumulative ends (on the device), start[b, 3] float32 (the origin of
 *               every cloud's grid), size > 0 finite (the cell edge).  Outputs, all int32: cluster[n], order[n], seg[m + 1],
 *               coord[m, 4], new_offset[b], n_cells[1].  64-bit address arithmetic throughout.
 *   cloud       Exactly pcc_knn_ragged's rule.  Offsets are clipped and never trusted: lo_c = min(max(offset[c-1], 0), n)
 *               with offset[-1] = 0, hi_c = min(max(offset[c], lo_c), n).  A row belongs to the cloud whose clipped range
 *               holds it (bisection, <= 16 steps).  A row behind the last range belongs to none.  Nothing is read outside
 *               xyz[0, n), offset[0, b), start[0, b), whatever the offsets hold.
 *   cell        Per axis a, in float32 with every operation rounded (IEEE): t = (x[a] - start[c][a]) / size.  The point is
 *               valid on that axis iff t >= 0 (false for NaN) and floorf(t) < 2^axis_bits; then q[a] = (int)floorf(t).  The
 *               division is a correctly rounded division, not a reciprocal multiply.  A point is dropped if any axis is
 *               invalid, if it is non-finite, or if it belongs to no cloud.  For coordinates at or above start this is
 *               div(coord - start, size, rounding_mode='trunc').
 *   key         cloud_bits is the bit width of b: the field holds 0 .. b, and the value b is the dropped key.
 *               key = (c << 3 axis_bits) | (q0 << 2 axis_bits) | (q1 << axis_bits) | q2.  A dropped point keys as
 *               b << 3 axis_bits, behind every valid key.  Requires 1 <= axis_bits <= 16 and
 *               cloud_bits + 3 axis_bits <= 63.
 *   outputs     With U the number of distinct valid keys and rank(key) the number of distinct valid keys below it:
 *               order: all n points ascending by (key, point index); dropped points come last, in index order.
 *               cluster[p] = rank if the point is valid and rank < m, else -1.
 *               seg[r] for r < min(U, m) is the first sorted position of slot r's run; seg[min(U, m) .. m] is the end of
 *               the last kept run.  This is pcc_grid_cluster's rule, so a padded slot's run is empty and
 *               pcc_segment_pool(b = 1, ...) takes order / seg as they are.
 *               coord[r] = (c, q0, q1, q2) for a kept slot, (-1, -1, -1, -1) for a padded one.
 *               new_offset[c] = min(m, number of distinct valid keys of clouds <= c): the cumulative ends of the pooled
 *               level, which is the offset of the next stage.
 *               n_cells[0] = U, the true count; U > m is how a caller sees that cells were dropped.
 *               The outputs at capacity m are those at capacity n restricted to their first m (+ 1) entries, apart from
 *               the -1 of the dropped ranks.  Integers only.  Every word of all six outputs is written exactly once per
 *               call.  Each word is fixed by the inputs: not by the run, not by what shares a workgroup.  A cloud's
 *               coord[:, 1:], its runs and its slot numbers relative to new_offset[c-1] do not depend on the other clouds
 *               or on the cloud's position in the batch.
 *   refusals    PCC_EINVAL under "grid_cluster_ragged:" before anything is enqueued: n < 1, m < 1 or m > n, b < 1 or
 *               b > 65535, n + 1 >= 2^31, axis_bits out of range or the key wider than 63 bits, size not finite or <= 0, a
 *               null pointer.
 *   launches    No host synchronisation: nothing is read on the host, and the grid of every launch is a function of
 *               (b, n, m, axis_bits) alone.  The device-wide steps -- the key, ceil((cloud_bits + 3 axis_bits) / 8) passes
 *               of a stable least-significant-digit radix sort over tiles of PCC_GRID_RAGGED_TILE keys, the run heads and
 *               their scan, the outputs -- are separate launches on the caller's stream; no workgroup waits on another.
 *               The sort's ping-pong buffers, histograms and scans come from the library's stream-ordered workspace
 *               (PCC_ENOMEM when it cannot be had), about 28 bytes per point.
 *   capture     Graph capture is neither claimed nor tested for this entry point.
 *   alignment   Every tensor argument may be any buffer aligned to its element size (the alignment paragraph above). */
#define PCC_GRID_RAGGED_TILE 2048
int pcc_grid_cluster_ragged(int b, int n, int m, int axis_bits, const float *xyz, const int32_t *offset, const float *start,
                            float size, int32_t *cluster, int32_t *order, int32_t *seg, int32_t *coord, int32_t *new_offset,
                            int32_t *n_cells, pcc_stream_t stream);

/* Submanifold sparse convolution (MinkUNet, SparseUNet, the conditional position encoding of Point Transformer V3) on the
 * slots of pcc_grid_cluster: every occupied cell sums, over the ksize^3 offsets of a kernel, a weight matrix applied to the
 * features of the occupied cell at that offset; the set of occupied cells does not grow.  No counterpart in the reference;
 * what a user writes in torch instead is a dense [b, c, res, res, res] grid under torch.nn.Conv3d, or a ksize^3-wide list, a
 * pcc_group_points along it (ksize^3 times the features) and one matmul.
 *   layouts     cell[b, n], order[b, n], seg[b, m + 1], n_cells[b] int32: those of pcc_voxel_index and pcc_grid_cluster for the
 *               same clouds, the same res and the same capacity m; nbr[b, m, t] int64, -1 where there is no neighbour, like
 *               every other list here (pcc_group_points, pcc_aggregate_points and pcc_local_geometry take it unchanged);
 *               x[b, c, n], out[b, o, m] float32 channels-major; weight[t, c, o], bias[o] float32.  64-bit offsets throughout.
 *   pcc_cell_neighbours   the kernel map.  Slot r < min(U, m) has the flat cell cell[order[seg[r]]] = (i * res + j) * res + k.
 *               With h = (ksize - 1) / 2 and offsets di, dj, dk in [-h, h], tap t = ((di + h) * ksize + (dj + h)) * ksize + (dk +
 *               h).  nbr[b, r, t]: the rank of the cell (i + dilation * di, j + dilation * dj, k + dilation * dk) if that cell
 *               lies inside [0, res)^3 (the triple is decomposed BEFORE the offset is added: nothing wraps around), is occupied
 *               and has a rank < m; -1 otherwise, and in every tap of a padded slot (r >= min(U, m)).  So the centre tap of a
 *               real slot is r itself, and the map is symmetric: nbr[r, t] = s >= 0 exactly when nbr[s, ksize^3 - 1 - t] = r.  The
 *               map at capacity m is the map at capacity n cut to its first m rows, with the ranks >= m turned into -1.
 *               Integers only: every word is written once and fixed by the cloud alone, not by b, the position in the batch or
 *               the run.  The four index arrays are trusted to be the library's (an entry outside its range is skipped, never
 *               dereferenced).  ksize is 3 or 5, dilation >= 1, 2 <= res <= 128, 1 <= m <= n <= 16384, b * m * ksize^3 < 2^31.
 *   pcc_sparse_conv   out[b, oc, r] = bias[oc] + sum over t and ch of weight[t, ch, oc] * x[b, ch, nbr[b, r, t]], over the taps
 *               with 0 <= nbr < n (n: the points of x; with a map of pcc_cell_neighbours n = m).  A row with no such tap is +0.0,
 *               without the bias: with a map of pcc_cell_neighbours that row is exactly a padded slot.  Every word of out is
 *               written exactly once; no float atomics; the [b, c, m, t] tensor of gathered features is never written.  The
 *               contract is a bound, not fixed words: the result of a row depends on that row's list, on x and on weight
 *               only -- so it is float-equal from run to run, at any batch position and for any b (the sign of a zero result
 *               is not fixed) --, and against exact arithmetic, with D = (valid taps) * c + 1 and S = |bias| + sum of |w| * |x|
 *               over the valid terms, |out - exact| <= D * 2^-24 / (1 - D * 2^-24) * S + D * 2^-126.  Non-finite features
 *               propagate as IEEE.  A tap that is empty in one row and not in a neighbouring row may be computed with a +0.0
 *               feature, so "an empty tap takes no part" holds for FINITE weights only: an infinite or NaN weight can turn rows
 *               with an empty tap into NaN.  bias may be null.  t is any length >= 1 (ksize^3 for a map).
 *               FORWARD ONLY for a general list: the gradient in x is the same entry point on the mirrored weights
 *               (weight'[t, oc, ch] = weight[t' - 1 - t, ch, oc], no bias) only because the map of pcc_cell_neighbours is
 *               symmetric, and the Python autograd node accepts such maps only.
 * Requires c, o, n, m, t >= 1, b <= 65535, m * t < 2^31, t * c * o < 2^31 and non-null pointers but for bias -- PCC_EINVAL
 * otherwise, under "cell_neighbours:", "sparse_conv:", before anything is enqueued.  b = 0 enqueues nothing and returns
 * PCC_OK.  No workspace and no host synchronisation: the calls can be captured into a graph. */
int pcc_cell_neighbours(int b, int n, int m, int res, int ksize, int dilation, const int32_t *cell, const int32_t *order,
                        const int32_t *seg, const int32_t *n_cells, int64_t *nbr, pcc_stream_t stream);
int pcc_sparse_conv(int b, int c, int o, int n, int m, int t, const float *x, const int64_t *nbr, const float *weight,
                    const float *bias, float *out, pcc_stream_t stream);

/* The kernel map of a submanifold sparse convolution over a RAGGED grid level: pcc_cell_neighbours for the slots of
 * pcc_grid_cluster_ragged -- scenes of any size, up to 2^16 cells per axis, a packed batch of clouds of unequal size.  The
 * result is an ordinary list with b = 1: pcc_sparse_conv, pcc_group_points, pcc_aggregate_points and pcc_local_geometry take
 * it unchanged.  What a user writes in torch instead: int64 keys, one searchsorted of m * ksize^3 targets, a mask.
 *   inputs      coord[m, 4] int32 and n_cells[1] int32 are those of pcc_grid_cluster_ragged at capacity m.  The real slots
 *               are r < kept = min(max(n_cells[0], 0), m), ascending by (c, i, j, k).  Rows at or after kept are never read.
 *               nbr[m, ksize^3] int64.
 *   rule        Let h = (ksize - 1) / 2, offsets di, dj, dk in [-h, h], and t = ((di + h) * ksize + (dj + h)) * ksize + (dk + h).
 *               nbr[r, t] is the rank s < kept of the slot whose row is (c, i + dilation * di, j + dilation * dj,
 *               k + dilation * dk): the same cloud, with every target coordinate inside [0, 65536).  It is -1 if there is no
 *               such slot.  It is -1 in every tap of a padded slot (r >= kept).
 *               The offsets are added to the decomposed coordinates in 32-bit integers, and the range test comes before any
 *               packing into a key.  Nothing wraps.  A carry from k into j must not turn (i, j, 65535) + 1 into
 *               (i, j + 1, 0), and cloud c's cell must not become cloud c +- 1's.
 *   so          The centre tap of a real slot is r.
 *               The map is symmetric: nbr[r, t] = s >= 0 exactly when nbr[s, ksize^3 - 1 - t] = r.
 *               The map at capacity m is the map at capacity n cut to m rows, with ranks >= m turned into -1.
 *               Integers only.  Every word is written exactly once and is fixed by coord alone.
 *   trust       coord is trusted to be the library's for the MEANING of the result, never for safety.  No value read from
 *               coord or n_cells becomes an address.  Every position read lies in [0, kept).  Every loop is bounded (a
 *               bisection by 32 steps, the taps by ksize).  On arbitrary int32 garbage every output word is in [-1, kept).
 *               (A real slot with a component outside [0, 65536) has -1 in every tap.)
 *   refusals    PCC_EINVAL under "cell_neighbours_ragged:" before anything is enqueued: m < 1, m * ksize^3 >= 2^31, ksize not
 *               3 or 5, dilation < 1, a null pointer.  A dilation of 65536 or more reaches only the centre and is clamped to
 *               65536, as pcc_cell_neighbours clamps to res.
 *   launches    One launch.  No workspace, no host synchronisation, no atomics, no inter-workgroup communication; the grid
 *               is a function of (m, ksize) alone.
 *   capture     Graph capture is neither claimed nor tested for this entry point.
 *   alignment   coord and n_cells may be any 4-byte-aligned address, nbr any 8-byte-aligned one (the alignment paragraph
 *               above): a row of coord is one 16-byte load only where coord lies on a 16-byte boundary. */
int pcc_cell_neighbours_ragged(int m, int ksize, int dilation, const int32_t *coord, const int32_t *n_cells, int64_t *nbr,
                               pcc_stream_t stream);

/* get_neighbours (neighbour_ops.py:85-94): out[b,c,n,j] = x[b,c,indices[b,n,j]]. */
int pcc_gather_neighbours(int b, int c, int n, int k, const float *x, const int64_t *indices, float *out,
                          pcc_stream_t stream);
/* backward of the gather: grad_x[b,c,t] = sum over (n,j) with indices[b,n,j]==t of grad_out[b,c,n,j].
 * grad_x is overwritten.  Accumulated in per-workgroup LDS bins (ds_add_f32): like the torch scatter_add the
 * reference's gather backward runs, the float summation order is not fixed. */
int pcc_gather_neighbours_bwd(int b, int c, int n, int k, const int64_t *indices, const float *grad_out,
                              float *grad_x, pcc_stream_t stream);

/* get_graph_features (neighbour_ops.py:113-119): out[b, 0:c, n, j] = x[b,:,indices[b,n,j]] - x[b,:,n],
 * out[b, c:2c, n, j] = x[b,:,n]. */
int pcc_graph_features(int b, int c, int n, int k, const float *x, const int64_t *indices, float *out,
                       pcc_stream_t stream);
/* backward: grad_x[b,c,t] = sum_{(n,j): idx=t} g[b,c,n,j] + sum_j (g[b,c+C,t,j] - g[b,c,t,j]). */
int pcc_graph_features_bwd(int b, int c, int n, int k, const int64_t *indices, const float *grad_out,
                           float *grad_x, pcc_stream_t stream);

/* graph_max_pooling (neighbour_ops.py:106-110): out[b,c,n] = max_j x[b,c,indices[b,n,j]];
 * argmax[b,c,n] (int32, the winning j, first on ties as torch.max) is written when non-null. */
int pcc_graph_max_pool(int b, int c, int n, int k, const float *x, const int64_t *indices, float *out,
                       int32_t *argmax, pcc_stream_t stream);
int pcc_graph_max_pool_bwd(int b, int c, int n, int k, const int64_t *indices, const int32_t *argmax,
                           const float *grad_out, float *grad_x, pcc_stream_t stream);

/* Building blocks of the fused EdgeConv front-end (pointcloudcounterfactual_amd/edgeconv.py): because
 * the 1x1 convolution is linear, W.[x_j - x_i ; x_i] = Wa.x_j + (Wb - Wa).x_i, so everything the EdgeConv block
 * (get_graph_features -> conv2d -> BatchNorm2d -> LeakyReLU -> max over k; src/module/encoders.py:50-53,
 * layers.py:159-203) needs from the [B,2C,N,k] edge tensor can be had from [B,C',N] tensors:
 *   pcc_neighbour_sum            out[b,c,n] = sum_j y[b,c,indices[b,n,j]]          (BatchNorm statistics)
 *   pcc_neighbour_sum_bwd        grad_y[b,c,t] = sum_{(n,j): idx=t} grad_out[b,c,n]
 *   pcc_neighbour_minmax_target  tsel[b,0,c,n] / tsel[b,1,c,n] = the neighbour (point index) with the largest /
 *                                smallest y among the k neighbours of n (first on ties) -- the edge that survives
 *                                max-over-k for a positive / negative BatchNorm scale. */
int pcc_neighbour_sum(int b, int c, int n, int k, const float *y, const int64_t *indices, float *out,
                      pcc_stream_t stream);
int pcc_neighbour_sum_bwd(int b, int c, int n, int k, const int64_t *indices, const float *grad_out,
                          float *grad_y, pcc_stream_t stream);
int pcc_neighbour_minmax_target(int b, int c, int n, int k, const float *y, const int64_t *indices, int64_t *tsel,
                                pcc_stream_t stream);

/* Encoder / classifier global pooling (src/module/encoders.py:58,90; classifier.py:63-64):
 * out_max[b,c] = max_n x[b,c,n] with argmax[b,c] (int32, first maximum), out_mean[b,c] = mean_n (either
 * output pointer may be null). */
int pcc_global_pool(int b, int c, int n, const float *x, float *out_max, int32_t *argmax, float *out_mean,
                    pcc_stream_t stream);

/* ---- generic-dimension pairwise reductions (the KeOps reductions of the reference outside the 3-D paths) ----------
 * D[b,i,j] = sum_c (p[b,i,c] - q[b,j,c])^2 over p[b,np,d], q[b,nq,d] (pykeops_square_distance, neighbour_ops.py:35-40),
 * difference form, channels accumulated in order with fma; never materialised.
 * pcc_pair_argmin: idx[b,i] = argmin_j D[b,i,j] (lowest index on ties), dist[b,i] = the minimum (may be NULL) --
 *   VectorQuantizer.quantize's `dist.argmin(axis=2)` (src/module/quantize.py:26-28); swap p and q for axis=1.
 * pcc_pair_sqdist_sum: out[b,i] = sum_j D[b,i,j] -- `dist.sum(1)` of quantize.py:31 (with p = codebook rows, q = the
 *   single query); pcc_pair_sqdist_sum_bwd: its gradients, grad_p[b,i,:] = 2 g[b,i] sum_j (p_i - q_j),
 *   grad_q[b,j,:] = -2 sum_i g[b,i] (p_i - q_j); either output may be NULL.
 * pcc_pair_argmin: a NaN distance never wins; a row whose distances are all NaN (or all +inf) returns index 0 and
 *   dist = +inf.  nq = 0: pcc_pair_argmin is PCC_EINVAL, pcc_pair_sqdist_sum writes zeros. */
int pcc_pair_argmin(int b, int np, int nq, int d, const float *p, const float *q, int64_t *idx, float *dist,
                    pcc_stream_t stream);
int pcc_pair_sqdist_sum(int b, int np, int nq, int d, const float *p, const float *q, float *out, pcc_stream_t stream);
int pcc_pair_sqdist_sum_bwd(int b, int np, int nq, int d, const float *p, const float *q, const float *grad_out,
                            float *grad_p, float *grad_q, pcc_stream_t stream);

/* ---- BatchNorm1d + ReLU (+ channel-repeated residual) over [b,c,n] --------------------------------------------------
 * The tail of the reference's PointsConv block (src/module/layers.py:159-166: conv -> BatchNorm1d -> activation ->
 * `+ x.repeat_interleave(r, 1)[:, :c]`), fused into streaming passes: pcc_bn_stats (training: per-channel mean and
 * biased variance over b*n, accumulated in double), pcc_bn_relu_res_fwd
 *   y[b,ch,i] = max(0, (z - mean[ch]) * rsqrt(var[ch] + eps) * gamma[ch] + beta[ch]) + res[b, ch / r, i]   (res may be NULL)
 * and pcc_bn_relu_bwd (grad_z, grad_gamma[c], grad_beta[c]; `training` = the statistics depend on z).  The gradient of
 * the residual operand is grad_y summed over each group of r channels (left to the caller).  b*c <= 65535.
 * Non-finite values follow the PyTorch composition: a channel whose sum or sum of squares is not finite gets a NaN
 * variance (only a finite negative rounding residue is clamped to 0); relu(NaN) = NaN; the backward zeroes the gradient
 * where the pre-activation is <= 0 only, so a NaN pre-activation passes it (threshold_backward).
 * The 16-byte accesses are used only when n % 4 == 0 and z, y, res / z, grad_y, grad_z are 16-byte aligned; any
 * 4-byte-aligned contiguous tensor is accepted, and for n % 4 == 0 the backward's sums run in the same order either way. */
int pcc_bn_stats(int b, int c, int n, const float *z, float *mean, float *var, pcc_stream_t stream);
int pcc_bn_relu_res_fwd(int b, int c, int n, const float *z, const float *mean, const float *var, float eps,
                        const float *gamma, const float *beta, const float *res, int res_c, int r, float *y,
                        pcc_stream_t stream);
int pcc_bn_relu_bwd(int b, int c, int n, const float *z, const float *mean, const float *var, float eps,
                    const float *gamma, const float *beta, const float *grad_y, int training, float *grad_z,
                    float *grad_gamma, float *grad_beta, pcc_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* PCC_NEIGHBOUR_H */
