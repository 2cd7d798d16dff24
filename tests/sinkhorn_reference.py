"""numpy float64 reference of the Sinkhorn divergence (``pcc_sinkhorn``, include/pcc_structural.h) for
tests/test_sinkhorn_host.py and tests/test_gpu_sinkhorn.py: the contract on the float32 inputs, dense, every smoothed
minimum a log-sum-exp with its maximum subtracted; together with the error units the bars are stated in.

Error units (per cloud).  A smoothed minimum is 1-Lipschitz in its input potential and one round's float32 error is a
small multiple of 2^-24 S whatever eps is, S = max(max C, max |f*|, max |g*|); so after the T + 2 rounds
    potentials, cost:  U  = (T + 2) 2^-24 S
    gradients:         Ug = U / eps_{T-1} * D / n  per component (D / m for grad_y), D = max |x_i - y_j| of that component.
A numpy float32 run of the contract stays inside 0.65 U (potentials), 0.004 U (cost), 0.002 Ug (gradients)."""

import numpy as np

# The asserted bars, in the units above: 4 x the largest multiple measured for the kernel on one MI355X over the grid of
# tests/test_gpu_sinkhorn.py (hardware exp2 / log2, its own summation order), rounded up to a power of two.
#   measured: potentials 1.65 U (257 x 1, T = 2), cost 0.66 U (1 x 1, T = 2), gradients 0.19 Ug (1 x 2, T = 1); at 2049 x 2047 with
#   the default schedule 0.06 U, 0.00005 U and 0.001 Ug.  (The float32 torch path: 0.73 U, 0.006 U, 0.006 Ug on its own grid.)
BAR_POT, BAR_COST, BAR_GRAD = 8.0, 4.0, 1.0
#   Either side of the sizes where the product changes its number of slices (32766 .. 65536 x 1): 1.46 U, 0.12 U, 0.05 Ug.
# A forced number of column slices against the product's choice, in the potentials, by the same rule.
#   measured: 0.103 U (700 x 1300, no split against the product's 8 slices)
BAR_SPLIT = 0.5

SCALES = ((1.0, 0.0), (1e-3, 0.0), (1000.0, 300.0))  # (scale, centre) of the clouds, rotated through by the grids


def clouds(seed, b, n, m, scale=1.0, centre=0.0):
    """Gaussian clouds ``x[b,n,3]``, ``y[b,m,3]`` float32, the second one shifted and a little narrower."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((b, n, 3)) * scale + centre).astype(np.float32)
    y = (rng.standard_normal((b, m, 3)) * (0.8 * scale) + (centre + 0.3 * scale)).astype(np.float32)
    return x, y


def diameter(x, y):
    """The largest per-axis extent over both clouds and the batch (``losses.sinkhorn_divergence``'s rule)."""
    both = np.concatenate((x.reshape(-1, 3), y.reshape(-1, 3))).astype(np.float64)
    return float((both.max(0) - both.min(0)).max())


def schedule(steps, diam):
    """The schedules of the grids, scaled by the diameter: 8 = the default one (blur = diameter / 40, scaling 0.5), 2 and
    1 = short ones whose last temperature is (diameter / 10)^2."""
    if steps == 8:
        out = [diam**2] + [diam**2 * 0.25**i for i in range(6)] + [(diam / 40) ** 2]
    elif steps == 2:
        out = [diam**2, (diam / 10) ** 2]
    else:
        out = [(diam / 10) ** 2] * steps
    return [float(np.float32(e)) for e in out]  # (the library reads float32)


def softmin(eps, cost, h=None):
    """SM_eps(h; U->V) over the rows of ``cost[rows, cols]`` and the log-sum-exp weights: -> (sm[rows], plan rows summing to 1)."""
    arg = (-cost if h is None else h[None, :] - cost) / eps - np.log(cost.shape[1])
    top = arg.max(axis=1, keepdims=True)
    e = np.exp(arg - top)
    tot = e.sum(axis=1, keepdims=True)
    return -eps * (top[:, 0] + np.log(tot[:, 0])), e / tot


def pair_cost(u, v):
    d = u[:, None, :] - v[None, :, :]
    return 0.5 * (d * d).sum(-1)


class Result:
    """``cost[b]``, ``pot_x[b,n]``, ``pot_y[b,m]``, ``grad_x[b,n,3]``, ``grad_y[b,m,3]`` in float64, and the units ``S[b]``, ``D[b,3]``,
    ``U[b]``, ``Ug_x[b,3]``, ``Ug_y[b,3]``."""

    def __init__(self, x, y, eps, debias=True):
        x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        eps = [float(e) for e in eps]
        b, n, m = x64.shape[0], x64.shape[1], y64.shape[1]
        self.cost, self.pot_x, self.pot_y = np.zeros(b), np.zeros((b, n)), np.zeros((b, m))
        self.grad_x, self.grad_y = np.zeros((b, n, 3)), np.zeros((b, m, 3))
        self.S, self.D = np.zeros(b), np.zeros((b, 3))
        for k in range(b):
            u, v = x64[k], y64[k]
            cxy, cyx = pair_cost(u, v), pair_cost(v, u)  # (each its own array: the four scans are one function of their arguments)
            f, g = softmin(eps[0], cxy)[0], softmin(eps[0], cyx)[0]
            if debias:
                cxx, cyy = pair_cost(u, u), pair_cost(v, v)
                p, q = softmin(eps[0], cxx)[0], softmin(eps[0], cyy)[0]
            for e in eps:
                f, g = 0.5 * (f + softmin(e, cxy, g)[0]), 0.5 * (g + softmin(e, cyx, f)[0])
                if debias:
                    p, q = 0.5 * (p + softmin(e, cxx, p)[0]), 0.5 * (q + softmin(e, cyy, q)[0])
            e = eps[-1]
            (fs, pxy), (gs, pyx) = softmin(e, cxy, g), softmin(e, cyx, f)
            # sum_j P_ij (u_i - v_j) = u_i - (P v)_i: the rows of P sum to 1
            gx, gy = u - pxy @ v, v - pyx @ u
            self.S[k] = max(cxy.max(), np.abs(fs).max(), np.abs(gs).max())
            self.D[k] = np.abs(u[:, None, :] - v[None, :, :]).max(axis=(0, 1))
            if debias:
                (ps, pxx), (qs, pyy) = softmin(e, cxx, p), softmin(e, cyy, q)
                fs, gs = fs - ps, gs - qs
                gx, gy = gx - (u - pxx @ u), gy - (v - pyy @ v)
            self.pot_x[k], self.pot_y[k] = fs, gs
            self.grad_x[k], self.grad_y[k] = gx / n, gy / m
            self.cost[k] = fs.mean() + gs.mean()
        self.U = (len(eps) + 2) * 2.0 ** -24 * self.S
        unit = (self.U / eps[-1])[:, None] * self.D
        self.Ug_x, self.Ug_y = unit / n, unit / m

    def multiples(self, got):
        """The largest error of each output in ``got`` (a dict by the contract's names) in its unit: {'pot', 'cost', 'grad'}."""
        out = {}
        with np.errstate(invalid='ignore', divide='ignore'):
            for name, key, unit in (('pot_x', 'pot', self.U[:, None]), ('pot_y', 'pot', self.U[:, None]), ('cost', 'cost', self.U),
                                    ('grad_x', 'grad', self.Ug_x[:, None, :]), ('grad_y', 'grad', self.Ug_y[:, None, :])):
                if name in got:
                    err = np.abs(np.asarray(got[name], dtype=np.float64) - getattr(self, name))
                    ratio = np.where(err == 0, 0.0, err / unit)  # (an exact result passes a unit of 0: n = m = 1, x = y)
                    out[key] = max(out.get(key, 0.0), float(np.max(ratio)) if np.all(np.isfinite(ratio)) else float('inf'))
        return out

    def check(self, got, what=''):
        mult = self.multiples(got)
        for key, bar in (('pot', BAR_POT), ('cost', BAR_COST), ('grad', BAR_GRAD)):
            assert mult.get(key, 0.0) <= bar, (what, key, mult)
        return mult


# ---- how many column slices a call's scans take (include/pcc_test_hooks.h, sinkhorn_split) ----
MAX_SPLIT, TILE, GROUP = 16, 256, 8


def slices(n, m, debias=True, forced=0):
    """The slices S the launch-profile name of the scans carries ("sk_scan_kernel S=..."): the allowance is the forced value
    (16 at the most), or by the row count (n + m, twice that with debias) the power of two that brings rows x slices to
    4096 waves' worth (262144), 16 at the most; a scan over c columns then takes ceil(c / chunk) slices of chunk = the
    columns over the allowance rounded up to whole groups of 8, none shorter than a 256-column tile; S is the most any scan
    takes (the scans run over n and over m columns)."""
    if forced >= 1:
        allow = min(forced, MAX_SPLIT)
    else:
        rows, allow = (n + m) * (2 if debias else 1), 1
        while allow < MAX_SPLIT and rows * allow < 4096 * 64:
            allow *= 2
    taken = [-(-cols // max(TILE, -(-(-(-cols // allow)) // GROUP) * GROUP)) for cols in (n, m)]
    return max(taken)


def scan_kernel(n, m, debias=True, forced=0):
    return f'sk_scan_kernel S={slices(n, m, debias, forced)}'
