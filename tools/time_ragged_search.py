"""Timings of the searches over packed (ragged) batches (neighbour_ops.knn_ragged / ball_query_ragged) beside the other ways to
run the same search on the same GPU in the same process:
  loop     a Python loop over the clouds through knn_cross / ball_query with b = 1 (the transposes into channels-major that
           knn_cross needs included), the per-cloud lists written into one packed result;
  padded   the NaN-padded rectangular batch [B, Nmax] through the same ops, the pad and the unpad included;
  dense    the dense masked [m, n] formulation, cdist + topk (k-NN) or + sort + slice (ball query), wherever the float32
           matrix stays under 2 GB ('n/a' with its size otherwise);
  sorted   workload (i) only, the self search: pcc_knn, the Hilbert-sorted search of equal clouds (the exhaustive ragged kernel
           is expected to lose to it).
Clouds are points on the unit sphere, fixed seed.  Searches: k-NN with k = 16, self and cross with m_b = n_b / 4 centres picked
by farthest point sampling; ball query with r = 0.2, nsample = 32 around the same centres.  Workloads: (i) 32 equal clouds of
2048, (ii) 32 clouds of sizes uniform in [512, 4096], (iii) 8 clouds of 20 000 - 60 000, (iv) one cloud of 100 000.  The variants
of a row alternate round by round; a figure is the median over 7 rounds (min-max) of the mean time per call inside a hipEvent
bracket on the stream.  No ratio is asserted: the tool writes what it measures.  Output: profiles/ragged_search_times.txt (or
--out)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')
K, RADIUS, NSAMPLE = 16, 0.2, 32
DENSE_LIMIT = 2 << 30


def pieces(t, offset):
    ends = [0] + offset.tolist()
    return [t[lo:hi] for lo, hi in zip(ends[:-1], ends[1:])]


def loop_knn(xs, qs, offset, m):
    idx = torch.empty((m, K), dtype=torch.int64, device=dev)
    lo = qlo = 0
    for x, q in zip(xs, qs):
        idx[qlo:qlo + len(q)] = ops.knn_cross(q.t()[None], x.t()[None], K)[0] + lo
        lo, qlo = lo + len(x), qlo + len(q)
    return idx


def loop_ball(xs, qs, offset, m):
    idx = torch.empty((m, NSAMPLE), dtype=torch.int64, device=dev)
    lo = qlo = 0
    for x, q in zip(xs, qs):
        idx[qlo:qlo + len(q)] = ops.ball_query(x[None], q[None], RADIUS, NSAMPLE) + lo
        lo, qlo = lo + len(x), qlo + len(q)
    return idx


def pad(t, batch, pos, b, width):
    out = torch.full((b, width, 3), float('nan'), device=dev)
    out[batch, pos] = t
    return out


def padded_knn(xyz, xb, xpos, query, qb, qpos, b, nmax, mmax, lo):
    idx = ops.knn_cross(pad(query, qb, qpos, b, mmax).transpose(1, 2), pad(xyz, xb, xpos, b, nmax).transpose(1, 2), K)
    return idx[qb, qpos] + lo[qb][:, None]


def padded_ball(xyz, xb, xpos, query, qb, qpos, b, nmax, mmax, lo):
    idx = ops.ball_query(pad(xyz, xb, xpos, b, nmax), pad(query, qb, qpos, b, mmax), RADIUS, NSAMPLE)
    return idx[qb, qpos] + lo[qb][:, None]


def dense_knn(xyz, xb, query, qb):
    d = torch.cdist(query, xyz)
    d.masked_fill_(qb[:, None] != xb[None, :], float('inf'))
    return d.topk(K, dim=1, largest=False)[1]


def dense_ball(xyz, xb, query, qb):
    n = len(xyz)
    inside = (torch.cdist(query, xyz) < RADIUS) & (qb[:, None] == xb[None, :])
    idx = torch.where(inside, torch.arange(n, device=dev)[None, :], n).sort(1)[0][:, :NSAMPLE]
    return torch.where(idx == n, idx[:, :1], idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ragged_search_times.txt'))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    workloads = [('i', [2048] * 32), ('ii', rng.integers(512, 4097, 32).tolist()), ('iii', rng.integers(20000, 60001, 8).tolist()),
                 ('iv', [100000])]
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere, seed 0; microseconds per call: median of 7 rounds (min-max), the '
             f'variants of a row alternating; k-NN k = {K}, ball query r = {RADIUS} nsample = {NSAMPLE}, cross searches and ball query around '
             'm_b = n_b / 4 farthest-point centres; ragged = one launch over the packed batch, loop = per-cloud calls with b = 1, padded = '
             'NaN-padded rectangular batch, dense = masked cdist + topk / sort, sorted = pcc_knn (equal clouds only)']
    torch.manual_seed(0)
    for tag, sizes in workloads:
        b, n = len(sizes), sum(sizes)
        offset = torch.tensor(np.cumsum(sizes), device=dev)
        new_offset = torch.tensor(np.cumsum([s // 4 for s in sizes]), device=dev)
        xyz = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1)
        sel = ops.farthest_point_sample_ragged(xyz, offset, new_offset)
        centres = xyz[sel].contiguous()
        m = len(centres)
        xb, qb = ops.offset2batch(offset), ops.offset2batch(new_offset)
        lo, qlo = offset - ops.offset2bincount(offset), new_offset - ops.offset2bincount(new_offset)
        xpos, qpos = torch.arange(n, device=dev) - lo[xb], torch.arange(m, device=dev) - qlo[qb]
        xs, qs = pieces(xyz, offset), pieces(centres, new_offset)
        nmax, mmax = max(sizes), max(s // 4 for s in sizes)
        label = f'({tag}) B={b} n={n} (clouds {min(sizes)}-{max(sizes)})'
        rows = [
            (f'knn self  m={n}', n * n,
             {'ragged': lambda: ops.knn_ragged(xyz, offset, K), 'loop': lambda: loop_knn(xs, xs, offset, n),
              'padded': lambda: padded_knn(xyz, xb, xpos, xyz, xb, xpos, b, nmax, nmax, lo),
              'dense': lambda: dense_knn(xyz, xb, xyz, xb)}),
            (f'knn cross m={m}', m * n,
             {'ragged': lambda: ops.knn_ragged(xyz, offset, K, centres, new_offset), 'loop': lambda: loop_knn(xs, qs, offset, m),
              'padded': lambda: padded_knn(xyz, xb, xpos, centres, qb, qpos, b, nmax, mmax, lo),
              'dense': lambda: dense_knn(xyz, xb, centres, qb)}),
            (f'ball      m={m}', m * n,
             {'ragged': lambda: ops.ball_query_ragged(xyz, offset, centres, new_offset, RADIUS, NSAMPLE),
              'loop': lambda: loop_ball(xs, qs, offset, m),
              'padded': lambda: padded_ball(xyz, xb, xpos, centres, qb, qpos, b, nmax, mmax, lo),
              'dense': lambda: dense_ball(xyz, xb, centres, qb)}),
        ]
        for what, cells, variants in rows:
            note = ''
            if cells * 4 > DENSE_LIMIT:
                del variants['dense']
                note = f'  dense n/a ([m, n] float32 = {cells * 4 / 2 ** 30:.1f} GB)'
            if tag == 'i' and what.startswith('knn self'):
                grid = xyz.view(b, 2048, 3).transpose(1, 2).contiguous()
                variants['sorted'] = lambda: ops.knn(grid, K)
            # the variants agree (indices of exact ties aside, which the unit sphere does not have; the dense forms round differently)
            want = variants['ragged']()
            agree = {name: float((fn() == want).float().mean()) for name, fn in variants.items() if name not in ('ragged', 'sorted')}
            t = medians(variants, iters=3, rounds=7, warm=2)
            line = f'{label} {what}:'
            for name, v in t.items():
                line += f'  {name} {v[0]:10.1f} ({v[1]:.1f}-{v[2]:.1f})'
            line += note + '  [' + ', '.join(f'{name} / ragged {t[name][0] / t["ragged"][0]:.2f}x' for name in t if name != 'ragged') + '; '
            line += 'same entries: ' + ', '.join(f'{name} {share:.4f}' for name, share in agree.items()) + ']'
            print(line, flush=True)
            lines.append(line)
        del xyz, centres, xs, qs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
