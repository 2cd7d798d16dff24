"""Timings of the vector-attention op (attention_aggregate: pcc_neighbour_softmax + pcc_aggregate_points and their backwards,
attention.hip) beside the two ways to the same result without it, on the same GPU in the same process:
  torch   what a user writes: the index list expanded to every channel, one gather of [B,C,M,k], masked_fill + softmax of
          the logits, the sum with the position encoding, the product with the attention and a sum over k; the backward
          through autograd;
  group   group_points(x, idx) (pcc_group_points) for the gather, then the same torch softmax, sum, product and sum.
Clouds are N Gaussian points with Gaussian values[B,C,N]; the M query points are other points (the cloud itself where
M = N); lists by knn_cross, and one degenerate ball_query(pad='first') list at radius 1e-4 around the cloud's own points:
every row repeats one index k times.  `fwd` is the forward alone, `f+b` the forward and the backward into the values, the
logits and (where there is one) the position encoding `rel` from a fixed incoming gradient.  The variants of a row
alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the
stream.  `kernels` are the library's own per-launch averages (pcc_profile_enable(1): one event pair around each launch) over
5 further forward + backward calls; behind the forward kernel the rate at which it reads the rel stream (B C M k 4 bytes)
and behind the grad_x / grad_rel kernel the rate at which it writes grad_rel, each as a share of the 8 TB/s HBM peak.
Output: profiles/attention_times.txt (or --out)."""
import argparse
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')  # the A/B switches of include/pcc_test_hooks.h

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')
HBM_PEAK = 8.0e12  # bytes per second
KERNELS = ((b'softmax_fwd_kernel', 'softmax'), (b'agg_fwd_kernel<lds>', 'fwd'), (b'agg_bwd_kernel<lds>', 'grad_x(+rel)'),
           (b'agg_bwd_kernel<direct>', 'grad_rel alone'), (b'agg_bwd_w_kernel', 'grad_w'), (b'softmax_bwd_kernel', 'softmax bwd'))


def _read_out(values, idx, logits, rel):
    """values[B,C,M,k] already gathered -> out[B,C,M], in torch."""
    b, c, m, k = values.shape
    g, n_valid = logits.shape[1], idx >= 0
    attn = torch.softmax(logits.masked_fill(~n_valid[:, None], float('-inf')), -1)
    if rel is not None:
        values = values + rel
    return (values.view(b, g, c // g, m, k) * attn[:, :, None]).sum(-1).view(b, c, m)


def torch_attention(x, idx, logits, rel=None):
    b, m, k = idx.shape
    c = x.shape[1]
    values = x.gather(2, idx.clamp_min(0).reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    return _read_out(values, idx, logits, rel)


def group_attention(x, idx, logits, rel=None):
    return _read_out(ops.group_points(x, idx), idx, logits, rel)


def kernel_times(run, stream_bytes):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name, label in KERNELS:
            us, cnt = read(name)
            if cnt:
                text += f' {label} {us:.1f}'
                if stream_bytes and label in ('fwd', 'grad_x(+rel)', 'grad_rel alone'):
                    rate = stream_bytes / (us * 1e-6)
                    text += f' ({rate / 1e12:.2f} TB/s of rel = {100 * rate / HBM_PEAK:.0f}% of peak)'
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, Gaussian clouds of N points with values[B,C,N], M queries, logits[B,G,M,k], rel[B,C,M,k]; '
             'out [B,C,M]; microseconds per call: median of 7 rounds (min-max), the variants of a row alternating']
    # (B, N, M, k, C, G, the list)
    rows = [(32, 2048, 2048, 16, 32, 4, 'knn'), (32, 2048, 2048, 16, 64, 8, 'knn'), (32, 512, 512, 16, 128, 16, 'knn'),
            (32, 15000, 15000, 16, 32, 4, 'knn'), (1, 15000, 15000, 16, 64, 8, 'knn'), (32, 2048, 2048, 16, 64, 8, 'first')]
    for b, n, m, k, c, g, kind in rows:
        xyz = torch.randn(b, 3, n, device=dev)
        queries = xyz if m == n else torch.randn(b, 3, m, device=dev)
        if kind == 'knn':
            idx = ops.knn_cross(queries, xyz, k)
        else:
            idx = ops.ball_query(xyz.transpose(1, 2).contiguous(), queries.transpose(1, 2).contiguous(), 1e-4, k, pad='first')
            assert (idx == idx[:, :, :1]).all()  # every row repeats one index
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        logits = torch.randn(b, g, m, k, device=dev).requires_grad_(True)
        rel_t = torch.randn(b, c, m, k, device=dev).requires_grad_(True)
        grad = torch.randn(b, c, m, device=dev)
        big = b * c * m * k > 1 << 26
        for rel in (None, rel_t):
            with torch.no_grad():  # the three formulations agree before they are timed
                ours = ops.attention_aggregate(x, idx, logits, rel)
                for other in (torch_attention, group_attention):
                    assert torch.allclose(ours, other(x, idx, logits, rel), rtol=1e-4, atol=1e-4)

            def fwd(fn, rel=rel):
                def run():
                    with torch.no_grad():
                        return fn(x, idx, logits, rel)
                return run

            def fwd_bwd(fn, rel=rel):
                def run():
                    x.grad = logits.grad = rel_t.grad = None
                    fn(x, idx, logits, rel).backward(grad)
                return run

            variants = {}
            for name, fn in (('ours', ops.attention_aggregate), ('torch', torch_attention), ('group', group_attention)):
                variants[name + '_fwd'], variants[name + '_fb'] = fwd(fn), fwd_bwd(fn)
            t = medians(variants, iters=3 if big else 10, rounds=7, warm=2)
            line = f'B={b:2d} N={n:5d} M={m:5d} k={k} C={c:3d} G={g:2d} {kind:5s} {"rel" if rel is not None else "   "}:'
            for key, label in (('ours_fwd', 'fwd'), ('torch_fwd', 'torch fwd'), ('group_fwd', 'group fwd'), ('ours_fb', 'f+b'),
                               ('torch_fb', 'torch f+b'), ('group_fb', 'group f+b')):
                line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
            line += (f'  [torch / ours: fwd {t["torch_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x; '
                     f'group / ours: fwd {t["group_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["group_fb"][0] / t["ours_fb"][0]:.2f}x]')
            line += '  kernels:' + kernel_times(fwd_bwd(ops.attention_aggregate), b * c * m * k * 4 if rel is not None else 0)
            print(line, flush=True)
            lines.append(line)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
