"""Seeded inputs of the two-cell (and three-cell) LFC-fit tests, host build and GPU: the few-cell IRLS kernels
k_irls<P, 3> / k_irls<P, 2> (csrc/dsq_k_irls.hip) in their staged (LDS-typed operands) and unstaged instantiations.

Every case holds genes with counts >= 64 and >= 256 (the memo of the gamma differences and the log-factorial table end
there), genes that are all zero in one group (their IRLS diverges: the rescue list), a design cell with two replicates
(its Cook's flags are off) and size factors over two decades.  The sample counts straddle the wavefront (64, 65, 130),
take the benchmark's 1000 and the two sides of the launcher's staging limit; G = 1, 5, 259 gives partial workgroups.

    python -m tests.irls_two_cell_cases --dump DIR     (GPU) everything the kernel writes for every case, as .npy
"""
import ctypes as C
import functools
import sys

import numpy as np

from oracle import nbglm_oracle as orc

_vp = C.c_void_p
MIN_MU, BETA_TOL, MAXITER = 0.5, 1e-8, 250
# tests/test_gpu_parity.py: irls beta / mu / H (:95-97), Wald (:120-122), Cook's layer (:621) - (rtol, atol)
TOL = {"beta": (1e-8, 1e-10), "mu": (1e-8, 1e-10), "H": (1e-8, 1e-12), "se": (1e-10, 0.0), "stat": (1e-9, 1e-13),
       "p": (1e-8, 1e-300), "cooks": (1e-6, 1e-12)}

# ---- the launcher's staging rule (launch_irls, few-cell branch): dynamic LDS of a staged launch =
#      kLgammaIntN doubles + npad (16 B size factor and its log + 1 B cell index and flags + 4 B count per wave)
#      + the cells' tables C (T + P) doubles, at most 48 KB; npad = N rounded up to 16
K_LGAMMA_INT_N, K_WAVES_PER_BLOCK, K_STAGE_LIMIT = 256, 4, 48 * 1024


def staged_bytes(N, C_, P):
    npad = (N + 15) & ~15
    return K_LGAMMA_INT_N * 8 + npad * (16 + 1 + 4 * K_WAVES_PER_BLOCK) + C_ * (P * (P + 1) // 2 + P) * 8


def largest_staged_n(C_, P):
    n = 16
    while staged_bytes(n + 16, C_, P) <= K_STAGE_LIMIT:
        n += 16
    return n


def two_group(N, interleaved):
    """intercept + group; group 1 has TWO samples (a cell below three replicates): the last two, or - interleaved -
    samples 1 and N - 2"""
    x = np.zeros(N)
    x[[1, N - 2] if interleaved else [N - 2, N - 1]] = 1.0
    return np.column_stack([np.ones(N), x])


def three_cell(N, P, interleaved):
    """three design cells of N/2 - 1, N/2 - 1 and 2 samples: P = 2 a dose 0 / 1 / 2, P = 3 three groups"""
    lvl = np.repeat([0, 1], N // 2) if not interleaved else np.arange(N) % 2
    lvl = lvl.copy()
    lvl[[1, N - 2] if interleaved else [N - 2, N - 1]] = 2
    if P == 2:
        return np.column_stack([np.ones(N), lvl.astype(float)])
    return np.column_stack([np.ones(N), lvl == 1, lvl == 2]).astype(float)


class Case:
    def __init__(self, name, X, G, seed, want):
        self.name, self.X, self.G, self.want = name, X, G, want
        N, P = X.shape
        self.N, self.P = N, P
        rng = np.random.default_rng(seed)
        self.sf = np.exp(rng.uniform(np.log(0.1), np.log(10.0), N))  # two decades
        self.sf[:2] = (0.1, 10.0)
        b0 = rng.normal(3.0, 1.5, G)
        b0[0] = 7.0  # counts >= 256 (and, in the cells that are not zeroed below, >= 64)
        if G > 1:
            b0[1] = 5.0
        beta = np.vstack([b0] + [rng.normal(0.0, 0.7, G) for _ in range(P - 1)])
        self.disp = np.exp(rng.uniform(np.log(0.02), np.log(1.5), G))
        mu = self.sf[:, None] * np.exp(X @ beta)
        r = 1.0 / self.disp[None, :]
        y = rng.negative_binomial(r, r / (r + mu)).astype(np.int64)
        cell = orc.design_cells(X)[0]
        big, small = int(np.argmax(np.bincount(cell))), int(np.argmin(np.bincount(cell)))
        # all zero in one group: gene 0 (the big cell; its other samples hold the high counts), every 37th in the big and
        # gene 4 and every 41st in the two-sample cell
        y[cell == small, 0] = np.maximum(y[cell == small, 0], 300)
        for g in range(G):
            if g % 37 == 0:
                y[cell == big, g] = 0
            elif g == 4 or g % 41 == 0:
                y[cell == small, g] = 0
        if G > 2:
            y[:, 2] = np.maximum(y[:, 2], 64)  # a gene wholly beyond the memo
        self.counts = y
        self.contrast = np.zeros(P)
        self.contrast[1] = 1.0
        self.cutoff = 0.9  # (any positive number: a threshold on the Cook's distances)
        self.robust_disp = orc.robust_mom_disp(y / self.sf[:, None], X)
        for a in (self.sf, self.disp, self.counts, self.robust_disp, self.X):
            a.setflags(write=False)

    @functools.cached_property
    def oracle(self):
        """beta, mu, H, conv, iterations of orc.irls; Cook's distances and Wald statistics from them.  Read-only."""
        beta, mu, H, conv, it = orc.irls(self.counts, self.sf, self.X, self.disp, MIN_MU, BETA_TOL, return_iters=True)
        p, stat, se = orc.wald_test(self.X, self.disp, beta, mu, np.diag(np.repeat(1e-6, self.P)), self.contrast)
        ck = orc.cooks_distance(self.counts, self.counts / self.sf[:, None], self.X, mu, H)
        out = dict(beta=beta, mu=mu, H=H, conv=conv, iters=it, p=p, stat=stat, se=se, cooks=ck)
        for a in out.values():
            a.setflags(write=False)
        return out

    @functools.cached_property
    def host(self):
        """tests/hostsim.lfc_fit (the host build of the same templates) with everything requested."""
        from tests import hostsim

        return hostsim.lfc_fit(self.counts, self.sf, self.X, self.disp, cells=True, robust_disp=self.robust_disp,
                               cutoff=self.cutoff, contrast=self.contrast, want_layers=True)


# what a launch is asked for: (mu / hat layers, Cook's bookkeeping, Cook's layer, Wald, two launches)
WANTS = {
    "all": (True, True, True, True, False),
    "bench": (False, True, True, True, False),     # the benchmark's LFC launch
    "layers": (True, False, False, False, False),
    "wald": (False, False, False, True, False),
    "flags": (False, True, False, False, False),   # Cook's flag vectors without the layer
    "parts": (False, True, True, True, True),      # dsq_lfc_set_part: two launches
}


@functools.lru_cache(maxsize=None)
def cases():
    ns = largest_staged_n(2, 2)
    plan = [  # (N, interleaved, G, outputs)
        (5, False, 259, "all"), (5, True, 1, "bench"),
        (64, False, 5, "layers"), (64, True, 259, "wald"),
        (65, False, 259, "flags"), (65, True, 5, "all"),
        (130, False, 1, "all"), (130, True, 259, "parts"),
        (1000, False, 259, "bench"), (1000, True, 5, "all"),
        (ns, False, 5, "wald"), (ns, True, 259, "all"),
        (ns + 1, False, 259, "all"), (ns + 1, True, 1, "flags"),
    ]
    out = []
    for k, (N, il, G, want) in enumerate(plan):
        out.append(Case(f"two_N{N}_{'il' if il else 'sorted'}_G{G}_{want}", two_group(N, il), G, 100 + k, want))
    out.append(Case("three_p2_N90_sorted_G259_all", three_cell(90, 2, False), 259, 200, "all"))
    out.append(Case("three_p2_N90_il_G5_bench", three_cell(90, 2, True), 5, 201, "bench"))
    out.append(Case("three_p3_N90_il_G259_parts", three_cell(90, 3, True), 259, 202, "parts"))
    out.append(Case("three_p3_N90_sorted_G1_layers", three_cell(90, 3, False), 1, 203, "layers"))
    return tuple(out)


def case_names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() if c.name == name)


def excess(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|); NaN patterns and infinities must agree"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (np.isnan(a) == np.isnan(b)).all(), "NaN patterns differ"
    fin = np.isfinite(b)
    assert (a[~fin & ~np.isnan(b)] == b[~fin & ~np.isnan(b)]).all(), "infinities differ"
    err, tol = np.abs(a[fin] - b[fin]), atol + rtol * np.abs(b[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0.0, 0.0, err / tol)
    return float(frac.max()) if fin.any() else 0.0


def compare(got, ref, what, names):
    """every named quantity of `got` within TOL of `ref`; returns the fractions of the tolerances used"""
    used = {k: excess(got[k], ref[k], *TOL[k]) for k in names}
    print(f"[irls two-cell] {what}: fractions of the tolerances {used}")
    bad = {k: v for k, v in used.items() if not v <= 1.0}
    assert not bad, f"{what}: beyond the tolerance (fraction of it): {bad}"
    return used


# ------------------------------------------------------------------ the device
def device_fit(ctx, c, want=None):
    """dsq_dev_lfc_fit2 on the case with the outputs its `want` names -> dict of host arrays (layers N x G).  Outputs
    start as NaN / 0xEE: whatever the kernel does not write stays that."""
    from pydeseq2_amd._design import DesignPack
    from pydeseq2_amd._lib import DeviceArray, DsqCells

    layers, cooks, cooks_layer, wald, parts = WANTS[want or c.want]
    N, G, P = c.N, c.G, c.P
    D = DesignPack(c.X)
    assert D.cell_path and D.n_design_cells <= 4
    ldn = D.ldx
    up = lambda a, dt: DeviceArray.from_host(ctx, np.ascontiguousarray(a, dtype=dt))  # noqa: E731
    y = np.zeros((G, ldn), np.int32)
    y[:, :N] = c.counts.T
    d_y, d_sf, d_Xt, d_pinv = up(y, np.int32), up(c.sf, np.float64), up(D.Xt, np.float64), up(D.pinvXt, np.float64)
    d_disp = up(c.disp, np.float64)
    d_cof, d_Xc, d_XX = up(D.cell_of, np.int32), up(D.Xc, np.float64), up(D.XXc, np.float64)
    cells = DsqCells(d_cof.ptr, d_Xc.ptr, d_XX.ptr, D.n_design_cells)
    nan_v = lambda n: up(np.full(n, np.nan), np.float64)  # noqa: E731
    ee_v = lambda n: up(np.full(n, 0xEE, np.uint8), np.uint8)  # noqa: E731
    d_beta, d_conv, d_it = nan_v(G * P), ee_v(G), up(np.full(G, -1, np.int32), np.int32)
    d_mu = nan_v(G * ldn) if layers else None
    d_hat = nan_v(G * ldn) if layers else None
    d_ck = nan_v(G * ldn) if cooks_layer else None
    d_rd, d_fl = up(c.robust_disp, np.float64), up(D.flags, np.uint8)
    fl4 = [ee_v(G) for _ in range(4)]
    pse = [nan_v(G) for _ in range(3)]
    ridge = np.ascontiguousarray(np.diag(np.repeat(1e-6, P)))
    con = np.ascontiguousarray(c.contrast)
    ptr = lambda d: _vp(d.ptr) if d is not None else None  # noqa: E731
    ck_args = [ptr(d_rd), ptr(d_fl), C.c_double(c.cutoff), ptr(d_ck)] + [ptr(a) for a in fl4] if cooks else \
        [None, None, C.c_double(0.0), None, None, None, None, None]
    wald_args = [_vp(ridge.ctypes.data), _vp(con.ctypes.data), C.c_double(0.0), 0] + [ptr(a) for a in pse] if wald else \
        [None, None, C.c_double(0.0), 0, None, None, None]

    def fit():
        ctx.call("dsq_dev_lfc_fit2", ptr(d_y), ldn, ptr(d_sf), ptr(d_Xt), ptr(d_pinv), D.ldx, N, G, P, int(D.full_rank),
                 ptr(d_disp), C.c_double(MIN_MU), C.c_double(BETA_TOL), C.c_double(-30.0), C.c_double(30.0), MAXITER,
                 ptr(d_beta), ptr(d_mu), ptr(d_hat), ptr(d_conv), ptr(d_it), C.byref(cells), *ck_args, *wald_args, None, 0)

    if parts:
        part = (np.arange(G) % 3 == 0).astype(np.uint8)
        d_part = up(part, np.uint8)
        ctx.call("dsq_lfc_fork_begin")
        ctx.call("dsq_lfc_set_part", ptr(d_part), 1, 1)
        fit()
        ctx.call("dsq_lfc_fork_end")
        ctx.call("dsq_lfc_set_part", ptr(d_part), 0, 2)
        fit()
    else:
        fit()
    ctx.sync()
    out = dict(beta=d_beta.to_host().reshape(G, P), conv=d_conv.to_host(), iters=d_it.to_host())
    lay = lambda d: d.to_host().reshape(G, ldn)[:, :N].T.copy()  # noqa: E731
    if layers:
        out["mu"], out["H"] = lay(d_mu), lay(d_hat)
    if cooks:
        out["flags"] = np.stack([a.to_host() for a in fl4])
    if cooks_layer:
        out["cooks"] = lay(d_ck)
    if wald:
        out["p"], out["stat"], out["se"] = (a.to_host() for a in pse)
    return out


def main(argv):
    import os

    from pydeseq2_amd._lib import Context

    assert len(argv) == 2 and argv[0] == "--dump", __doc__
    os.makedirs(argv[1], exist_ok=True)
    ctx = Context(0)
    for c in cases():
        for want in sorted({c.want, "all"}):
            for k, v in device_fit(ctx, c, want).items():
                np.save(os.path.join(argv[1], f"{c.name}__{want}__{k}.npy"), v)
    print(f"dumped {len(cases())} cases to {argv[1]}")


if __name__ == "__main__":
    main(sys.argv[1:])
