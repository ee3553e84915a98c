"""ctypes front-end of the TEST-ONLY device build of dsq_math.h / dsq_wave.h (see devunit.hip) and of dsq_wide.h /
dsq_wider.h / row_chol_solve (see devunit_linalg.hip), of dsq_stats.h / dsq_lds_sort.h (see devunit_stats.hip) and of
dsq_lbfgsb_wave.h / dsq_lbfgsb.h / dsq_lbfgsb_par.h (see devunit_optim.hip), and of dsq_alpha.h's objective and the row
kernels of the dispersion fit (see devunit_alpha.hip), of the trend fit's passes and the product's trend unit (see
devunit_trend.hip), and of dsq_shrink.h's objective (see devunit_shrink.hip).

Every function takes numpy arrays, pads them to whole 256-thread blocks where the caller has not, runs one entry point
(allocate, copy, launch, synchronise, free) and raises on a non-zero hipError_t."""
import ctypes as C

import numpy as np

from .build import build

_lib = None

MATH_OPS = ["frcp", "frsq", "frcp_g", "fdiv", "flog", "flog_t", "flog1p", "flog1p_t", "fexp_t", "lgamma_pos",
            "digamma_pos", "lgdg00", "lgdg10", "lgdg01", "lgdg11", "norm_sf", "stirling_big", "log_count"]
WAVE_OPS = ["sum", "sumi", "maxi", "max", "excl_scan_i", "from_lane", "uniform", "readlane_d", "row_bcast", "any",
            "hist_add", "slot_add", "slot_add_third", "cell_add"]
LIN_OPS = ["chol", "logdet", "solve", "inverse", "frob", "quad_xs", "cells"]
ROW_P = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16)  # k_irls_row's widths, and 16
SUM_N_K = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 24, 48)
BLOCK = 256


class DevunitError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _check(rc, what):
    if rc != 0:
        raise DevunitError(f"{what}: hipError_t {rc}")


def _pad(x, dtype, fill):
    """x flattened, padded with `fill` to a multiple of the block size (whole waves)."""
    x = np.asarray(x, dtype=dtype).ravel()
    n = max(BLOCK, -(-x.size // BLOCK) * BLOCK)
    out = np.full(n, fill, dtype=dtype)
    out[: x.size] = x
    return out


def math(op, x, y=None, pad=1.0):
    """(first result, second result) of dsq_math op `op` (MATH_OPS) for every element of x (and y for fdiv)."""
    xs = np.asarray(x, dtype=np.float64).ravel()
    xp = _pad(xs, np.float64, pad)
    yp = _pad(y, np.float64, 1.0) if y is not None else None
    if yp is not None and yp.size != xp.size:
        raise ValueError("x and y differ in size")
    o1, o2 = np.zeros_like(xp), np.zeros_like(xp)
    _check(lib().du_math(C.c_int(MATH_OPS.index(op)), _p(xp, C.c_double), _p(yp, C.c_double), _p(o1, C.c_double),
                         _p(o2, C.c_double), C.c_int(xp.size)), f"du_math({op})")
    return o1[: xs.size], o2[: xs.size]


def tables():
    """{'lgamma_int', 'log_int', 'log_tab', 'exp_tab'} as a kernel reads them (constant memory / LDS copies)."""
    n = lib().du_tables_n()
    o = np.full(n, np.nan)
    _check(lib().du_tables(_p(o, C.c_double)), "du_tables")
    return {"lgamma_int": o[:256], "log_int": o[256:512], "log_tab": o[512:768], "exp_tab": o[768:896]}


def lgdiff(wave, y, a, grad=True, big=False):
    """lgamma_digamma_diff<Wv, grad, big>: y is [genes][wave] counts, a one value per gene -> (dl, dd), same shape."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    G = y.shape[0]
    if y.shape != (G, wave) or a.size != G:
        raise ValueError("y must be [genes][wave], a one per gene")
    per = BLOCK // wave
    Gp = -(-G // per) * per
    yp = np.full((Gp, wave), 256 if big else 0, np.int32)
    yp[:G] = y
    ap = np.ones(Gp)
    ap[:G] = a
    dl, dd = np.zeros(yp.size), np.zeros(yp.size)
    _check(lib().du_lgdiff(C.c_int(wave), C.c_int(int(grad)), C.c_int(int(big)), _p(yp, C.c_int), _p(ap, C.c_double),
                           _p(dl, C.c_double), _p(dd, C.c_double), C.c_int(yp.size)), "du_lgdiff")
    return dl.reshape(Gp, wave)[:G], dd.reshape(Gp, wave)[:G]


def irls_cst(y, a):
    """irls_init's cst for one-sample genes: -[(lgamma(a) - lgamma(y + a)) + log(y!)] per (y, a)."""
    y = np.asarray(y, dtype=np.int32).ravel()
    G = y.size
    Gp = -(-G // 4) * 4
    yp = np.zeros(Gp, np.int32)
    yp[:G] = y
    ap = np.ones(Gp)
    ap[:G] = np.broadcast_to(np.asarray(a, dtype=np.float64), (G,))
    c = np.full(Gp, np.nan)
    _check(lib().du_irls_cst(_p(yp, C.c_int), _p(ap, C.c_double), _p(c, C.c_double), C.c_int(64 * Gp)), "du_irls_cst")
    return c[:G]


def wave(wave, op, x=None, xi=None, even_only=False, nout=1, fill=np.nan, ifill=-7):
    """Run the Wave policy's op (WAVE_OPS) on whole waves: x / xi hold n = multiple of 256 values (lane order).
    Returns (double results, int results), each [nout][n]; entries the kernel did not write keep fill / ifill."""
    n = (np.asarray(x) if x is not None else np.asarray(xi)).size
    if n % BLOCK:
        raise ValueError("n must be a multiple of 256")
    xd = np.ascontiguousarray(x, dtype=np.float64).ravel() if x is not None else None
    xin = np.ascontiguousarray(xi, dtype=np.int32).ravel() if xi is not None else None
    o = np.full(n * nout, fill, dtype=np.float64)
    oi = np.full(n * nout, ifill, dtype=np.int32)
    _check(lib().du_wave(C.c_int(wave), C.c_int(WAVE_OPS.index(op)), C.c_int(int(even_only)), _p(xd, C.c_double),
                         _p(xin, C.c_int), _p(o, C.c_double), _p(oi, C.c_int), C.c_int(n), C.c_int(nout)),
           f"du_wave({wave}, {op})")
    return o.reshape(nout, n), oi.reshape(nout, n)


def sum_n(wave, x, even_only=False, fill=np.nan):
    """x: [K][n] -> (sum_n<K> results, sum() of each value), both [K][n]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    K, n = x.shape
    o, r = np.full_like(x, fill), np.full_like(x, fill)
    _check(lib().du_sumn(C.c_int(wave), C.c_int(K), C.c_int(int(even_only)), _p(x, C.c_double), _p(o, C.c_double),
                         _p(r, C.c_double), C.c_int(n)), f"du_sumn({wave}, {K})")
    return o, r


def ksum(wave, x, even_only=False, fill=np.nan):
    """x: [T][n] terms; lane i accumulates x[:, i] in a KSum -> (lane s, lane c, sum_comp result), each [n]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    T, n = x.shape
    ls, lc, o = np.full(n, fill), np.full(n, fill), np.full(n, fill)
    _check(lib().du_ksum(C.c_int(wave), C.c_int(T), C.c_int(int(even_only)), _p(x, C.c_double), _p(ls, C.c_double),
                         _p(lc, C.c_double), _p(o, C.c_double), C.c_int(n)), f"du_ksum({wave})")
    return ls, lc, o


# ------------------------------------------------------------------------------- dsq_wide.h / dsq_wider.h / dsq_linalg.h
def wide_ld(P):
    return P | 1


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def gram(mp, two, Xt, w0, w1=None, N=None, blocks=0):
    """WideGram<Wv, two, mp> over the product's call sequence.  Xt: [G][P][ldx], w0 / w1: [G][N] (N <= ldx) ->
    (M, dM), each [G][P][ld] as the workspace holds them; what the kernel did not write is NaN."""
    Xt, w0 = _d(Xt), _d(w0)
    G, P, ldx = Xt.shape
    N = w0.shape[1] if N is None else N
    w1 = _d(w1) if w1 is not None else None
    if w0.shape != (G, N) or (w1 is not None and w1.shape != (G, N)):
        raise ValueError("w0 / w1 must be [G][N]")
    M = np.full((G, P, wide_ld(P)), np.nan)
    dM = np.full_like(M, np.nan)
    _check(lib().du_gram(C.c_int(mp), C.c_int(int(two)), C.c_int(P), C.c_int(N), C.c_int(ldx), C.c_int(G),
                         C.c_int(blocks), _p(Xt, C.c_double), _p(w0, C.c_double), _p(w1, C.c_double),
                         _p(M, C.c_double), _p(dM, C.c_double)), f"du_gram({mp}, {two}, P={P}, N={N})")
    return M, dM


def wide_linalg(mp, op, P, in0, in1=None, diag_add=0.0, cells=0, blocks=0):
    """One op of LIN_OPS per gene.  in0 / in1: [G][...] (dense P x P matrices, P vectors, xs as [P][64], Xc as [C][P],
    cell sums [C]).  Returns [G][nout]: P x ld for chol / cells, 2 x P x ld (Li, inv) for inverse, P for solve, the 64
    lanes' values for logdet / frob / quad_xs."""
    in0 = _d(in0)
    G = in0.shape[0]
    in0 = in0.reshape(G, -1)
    in1 = _d(in1).reshape(G, -1) if in1 is not None else None
    ld = wide_ld(P)
    nout = {"chol": P * ld, "cells": P * ld, "inverse": 2 * P * ld, "solve": P}.get(op, 64)
    out = np.full((G, nout), np.nan)
    _check(lib().du_wide_linalg(C.c_int(mp), C.c_int(LIN_OPS.index(op)), C.c_int(P), C.c_int(G), C.c_int(blocks),
                                C.c_int(cells), C.c_double(diag_add), _p(in0, C.c_double), C.c_int(in0.shape[1]),
                                _p(in1, C.c_double), C.c_int(in1.shape[1] if in1 is not None else 0),
                                _p(out, C.c_double), C.c_int(nout)), f"du_wide_linalg({mp}, {op}, P={P})")
    return out


def irls_rhs(mp, Xt, y, sf, beta, disp, min_mu, a, blocks=0):
    """One irls_sweep_wide (no cells) at beta.  Xt: [G][P][ldx], y / sf: [G][N], beta: [G][P] ->
    (W.v(1) [G][P], W.M [G][P][ld])."""
    Xt, sf, beta = _d(Xt), _d(sf), _d(beta)
    y = np.ascontiguousarray(y, dtype=np.int32)
    G, P, ldx = Xt.shape
    N = y.shape[1]
    if y.shape != (G, N) or sf.shape != (G, N) or beta.shape != (G, P):
        raise ValueError("y / sf must be [G][N], beta [G][P]")
    v1 = np.full((G, P), np.nan)
    M = np.full((G, P, wide_ld(P)), np.nan)
    _check(lib().du_irls_rhs(C.c_int(mp), C.c_int(P), C.c_int(N), C.c_int(ldx), C.c_int(G), C.c_int(blocks),
                             _p(Xt, C.c_double), _p(y, C.c_int), _p(sf, C.c_double), _p(beta, C.c_double),
                             C.c_double(disp), C.c_double(min_mu), C.c_double(a), _p(v1, C.c_double),
                             _p(M, C.c_double)), f"du_irls_rhs({mp}, P={P}, N={N})")
    return v1, M


def row_solve(P, ent, ridge, even_only=False):
    """row_chol_solve<RowWave, P>: ent [G][P (P + 1) / 2 + P] (packed lower triangle, then b) -> x [G][16 lanes][P];
    rows that left early (even_only: genes 1 and 3 of every four) keep NaN."""
    ent = _d(ent)
    G = ent.shape[0]
    if ent.shape != (G, P * (P + 1) // 2 + P):
        raise ValueError("ent must be [G][T + P]")
    x = np.full((G, 16, P), np.nan)
    _check(lib().du_row_solve(C.c_int(P), C.c_int(G), C.c_int(int(even_only)), _p(ent, C.c_double),
                              C.c_double(ridge), _p(x, C.c_double)), f"du_row_solve({P})")
    return x


# ------------------------------------------------------------------------------- dsq_stats.h / dsq_lds_sort.h
def _proto():
    """argument types of the devunit_stats.hip entry points (set once per process)"""
    L = lib()
    if getattr(L, "_stats_proto", False):
        return L
    pd, pi, p32, pu8 = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    for f in (L.du_lds_sort, L.du_lds_merge, L.du_lds_sort_merge):
        f.argtypes = [pd, pi, C.c_int, C.c_int, pd]
        f.restype = C.c_int
    L.du_trimmed_select.argtypes = [pd, pi, pi, C.c_int, C.c_int, pd]
    for f in (L.du_bucket_rank_sum, L.du_select_rank_sum):
        f.argtypes = [pd, p32, pd, p32, pd, pi, pi, C.c_int, C.c_int, pd, pi]
        f.restype = C.c_int
    L.du_seg_variances.argtypes = [p32, pd, p32, p32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, pd]
    L.du_cooks_acc.argtypes = [C.c_int, p32, pd, pd, pu8, C.c_int, C.c_int, C.c_int, pd, C.c_double, C.c_int, pd, pi]
    for f in (L.du_trimmed_select, L.du_seg_variances, L.du_cooks_acc):
        f.restype = C.c_int
    L._stats_proto = True
    return L


def _rows(rows, dtype=np.float64):
    """rows of different lengths -> (concatenated values, offsets [len + 1])"""
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, dtype=dtype).ravel() for r in rows]) if rows else np.zeros(0, dtype)
    return np.ascontiguousarray(flat, dtype=dtype), off


def _split(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def lds_sort(rows, fill=0, merge=False):
    """LdsSorter::operator() on every row (merge = True: ::merge; merge = "after sort": the product's sequence sort,
    squared errors around the sorted row's element n // 3, merge); the rows as the sorter leaves them."""
    v, off = _rows(rows)
    out = np.full_like(v, -7.0)
    name = {False: "du_lds_sort", True: "du_lds_merge", "after sort": "du_lds_sort_merge"}[merge]
    _check(getattr(_proto(), name)(_p(v, C.c_double), _p(off, C.c_int), len(rows), fill, _p(out, C.c_double)), name)
    return _split(out, off)


def trimmed_select(rows, nts, fill=0):
    """trimmed_sum_select(row, n, nt) per row"""
    v, off = _rows(rows)
    nt = np.ascontiguousarray(nts, dtype=np.int32)
    out = np.full(len(rows), np.nan)
    _check(_proto().du_trimmed_select(_p(v, C.c_double), _p(off, C.c_int), _p(nt, C.c_int), len(rows), fill,
                                      _p(out, C.c_double)), "du_trimmed_select")
    return out


def rank_sum(problems, select, use_range, fill=0):
    """bucket_rank_sum (select: select_rank_sum) per problem.  A problem is a dict with j_lo, j_hi and either v (a
    buffer of doubles, -1 = inactive) or y, sf, idx (None: samples in order), tm, squared (a NormedValues accessor).
    Returns (sums, accepted flags)."""
    n_prob = len(problems)
    acc_mode = ["y" in q for q in problems]
    lens = [len(q["y"] if a else q["v"]) for q, a in zip(problems, acc_mode)]
    v, off = _rows([q["v"] if not a else np.zeros(n) for q, a, n in zip(problems, acc_mode, lens)])
    y, _ = _rows([q["y"] if a else np.zeros(n) for q, a, n in zip(problems, acc_mode, lens)], np.int32)
    sf, _ = _rows([q["sf"] if a else np.ones(n) for q, a, n in zip(problems, acc_mode, lens)])
    idx, _ = _rows([q["idx"] if a and q.get("idx") is not None else np.arange(n)
                    for q, a, n in zip(problems, acc_mode, lens)], np.int32)
    tm = np.array([float(q.get("tm", 0.0)) for q in problems])
    ip = np.zeros((n_prob, 4), np.int32)
    for i, (q, a) in enumerate(zip(problems, acc_mode)):
        n_act = int((np.asarray(q["y"]) != 0).sum()) if a else int((~(np.asarray(q["v"]) < 0)).sum())
        mode = int(bool(select)) | (int(bool(use_range)) << 1) | (int(a) << 2)
        if a:
            mode |= (int(bool(q.get("squared", False))) << 3) | (int(q.get("idx") is not None) << 4)
        ip[i] = (n_act, q["j_lo"], q["j_hi"], mode)
    out, ok = np.full(n_prob, np.nan), np.full(n_prob, -7, np.int32)
    entry = _proto().du_select_rank_sum if select else _proto().du_bucket_rank_sum
    _check(entry(_p(v, C.c_double), _p(y, C.c_int32), _p(sf, C.c_double), _p(idx, C.c_int32),
                                _p(tm, C.c_double), _p(off, C.c_int), _p(ip, C.c_int), n_prob, fill,
                                _p(out, C.c_double), _p(ok, C.c_int)), "du_select_rank_sum" if select else "du_bucket_rank_sum")
    return out, ok


def seg_variances(y, sf, sizes, index, L, fill=0):
    """One seg_trimmed_variances pass per batch of 128 / L cells from vmax = -inf.  y: [G][N] counts, sizes: the
    cells' sizes, index: their sample ids one cell after the other.  Returns [G][n_cells]: lane q of batch b holds
    cell b * (128 / L) + q; and the lanes beyond the cells of every batch, which must still hold -inf."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    G, N = y.shape
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ci = np.ascontiguousarray(index, dtype=np.int32)
    nc, per = len(sizes), 128 // L
    nb = -(-nc // per)
    out = np.full((G, nb, 64), np.nan)
    _check(_proto().du_seg_variances(_p(y, C.c_int32), _p(sf, C.c_double), _p(co, C.c_int32), _p(ci, C.c_int32), nc, N, G,
                                     L, fill, _p(out, C.c_double)), "du_seg_variances")
    cells = np.concatenate([out[:, b, :min(per, nc - b * per)] for b in range(nb)], axis=1)
    rest = np.concatenate([out[:, b, min(per, nc - b * per):] for b in range(nb)], axis=1)
    return cells, rest


def cooks_acc(y, mu, hat, flags, ar, cutoff, P, counted=False, fill=0):
    """CooksAcc<DeviceWave>: add() over every sample, then finish() (counted: finish_counted with a counting lambda).
    y / mu / hat: [G][N].  Returns (ck [G][N], ints [G][6]: any_gt_all, any_gt_use, any_gt_use_nr, few_above, the
    winner's index, the winner's count)."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    G, N = y.shape
    mu, hat = _d(mu), _d(hat)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    ar = np.ascontiguousarray(np.broadcast_to(np.asarray(ar, dtype=np.float64), (G,)))
    ck, io = np.full((G, N), -7.0), np.full((G, 6), -7, np.int32)
    _check(_proto().du_cooks_acc(int(counted), _p(y, C.c_int32), _p(mu, C.c_double), _p(hat, C.c_double), _p(fl, C.c_uint8),
                                 N, G, P, _p(ar, C.c_double), float(cutoff), fill, _p(ck, C.c_double), _p(io, C.c_int)),
           "du_cooks_acc")
    return ck, io


# ------------------------------------------------------------------------------- dsq_lbfgsb_wave.h / dsq_lbfgsb.h / _par.h
TRACE_CAP = 256
NAN_WORD, ZERO_WORD, FF_WORD = 0x7FF8000000000000, 0, 0xFFFFFFFFFFFFFFFF
LBP_OPS = ["dpofa", "dtrsl01", "dtrsl11", "batch11"]


def groupsum(R, which, v):
    """wv8 / wv16 / wv32 (R) rowsum or colsum (which) of one value per lane: v holds whole 256-thread blocks."""
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    out = np.full_like(v, np.nan)
    _check(lib().du_groupsum(C.c_int(R), C.c_int(["rowsum", "colsum"].index(which)), _p(v, C.c_double),
                             _p(out, C.c_double), C.c_int(v.size)), f"du_groupsum({R}, {which})")
    return out


def direction(R, col, head, theta, S, Y, RHO, g, x):
    """lbfgsb_wave_direction<R> per problem.  S, Y: [n][10][R], RHO: [n][10], g, x: [n][R] -> (d, z), each [n][R]."""
    S, Y, RHO, g, x = _d(S), _d(Y), _d(RHO), _d(g), _d(x)
    n = S.shape[0]
    if S.shape != (n, 10, R) or Y.shape != S.shape or RHO.shape != (n, 10) or g.shape != (n, R) or x.shape != (n, R):
        raise ValueError("S / Y must be [n][10][R], RHO [n][10], g / x [n][R]")
    col = np.ascontiguousarray(col, dtype=np.int32)
    head = np.ascontiguousarray(head, dtype=np.int32)
    theta = _d(theta)
    if col.shape != (n,) or head.shape != (n,) or theta.shape != (n,):
        raise ValueError("col / head / theta must be [n]")
    d, z = np.full((n, R), np.nan), np.full((n, R), np.nan)
    _check(lib().du_direction(C.c_int(R), C.c_int(n), _p(col, C.c_int), _p(head, C.c_int), _p(theta, C.c_double),
                              _p(S, C.c_double), _p(Y, C.c_double), _p(RHO, C.c_double), _p(g, C.c_double),
                              _p(x, C.c_double), _p(d, C.c_double), _p(z, C.c_double)), f"du_direction({R})")
    return d, z


def optimise(form, problems, P=0, R=0, block=64, pattern=NAN_WORD):
    """One optimiser run per problem (dicts with Q [n][n], c, w, x0 and optionally bounds, scipy's convention; one n).
    form "wave": lbfgsb_wave<P, R>, `block` threads per block (64: a problem per block, 256: four); "one" / "lanes":
    lbfgsb_nd<R, ., 10, OneLane / DeviceWave>.  The workspace holds `pattern` in every 64-bit word before x0 goes in.
    Returns a list of dicts: x, f, g (the evaluations, in order, at most TRACE_CAP), nev (evaluations made), xfin, ffin,
    success, nfev, nit, status."""
    n = len(problems[0]["c"])
    k = len(problems)
    Q = _d([q["Q"] for q in problems])
    c, w, x0 = (_d([q[key] for q in problems]) for key in ("c", "w", "x0"))
    if Q.shape != (k, n, n) or c.shape != (k, n) or w.shape != (k, n) or x0.shape != (k, n):
        raise ValueError("the problems of one call share n")
    l, u, nbd = np.zeros((k, n)), np.zeros((k, n)), np.zeros((k, n), np.int32)
    for i, q in enumerate(problems):
        for j, (lo, hi) in enumerate(q.get("bounds") or [(None, None)] * n):
            has_l, has_u = lo is not None and np.isfinite(lo), hi is not None and np.isfinite(hi)
            l[i, j], u[i, j] = (lo if has_l else 0.0), (hi if has_u else 0.0)
            nbd[i, j] = {(False, False): 0, (True, False): 1, (True, True): 2, (False, True): 3}[(has_l, has_u)]
    if form == "wave" and nbd.any():
        raise ValueError("lbfgsb_wave takes no bounds")
    tx, tg = np.full((k, TRACE_CAP, n), np.nan), np.full((k, TRACE_CAP, n), np.nan)
    tf, xo, fo = np.full((k, TRACE_CAP), np.nan), np.full((k, n), np.nan), np.full(k, np.nan)
    res = np.full((k, 5), -7, np.int32)
    f = lib().du_optimise
    f.argtypes = [C.c_int] * 6 + [C.c_uint64] + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int)] + \
        [C.POINTER(C.c_double)] * 5 + [C.POINTER(C.c_int)]
    f.restype = C.c_int
    _check(f(["wave", "one", "lanes"].index(form), P, R, block, n, k, pattern, _p(Q, C.c_double), _p(c, C.c_double),
             _p(w, C.c_double), _p(x0, C.c_double), _p(l, C.c_double), _p(u, C.c_double), _p(nbd, C.c_int),
             _p(tx, C.c_double), _p(tf, C.c_double), _p(tg, C.c_double), _p(xo, C.c_double), _p(fo, C.c_double),
             _p(res, C.c_int)), f"du_optimise({form}, P={P}, R={R}, n={n})")
    out = []
    for i in range(k):
        nev = int(res[i, 4])
        m = min(max(nev, 0), TRACE_CAP)
        out.append(dict(x=tx[i, :m], f=tf[i, :m], g=tg[i, :m], nev=nev, xfin=xo[i], ffin=fo[i], success=bool(res[i, 0]),
                        nfev=int(res[i, 1]), nit=int(res[i, 2]), status=int(res[i, 3])))
    return out


def lbp(wave64, op, lda, ns, a, b=None, sacc=None):
    """lbp::dpofa / dtrsl_upper (jobs 01, 11) / the batch of dtrsl_upper_t_own on columns n + 1 .. 2 n (LBP_OPS) with
    DeviceWave (wave64) or OneLane, both on the device.  a: [k][lda][lda] as the routine indexes it (a[p].ravel()[(i - 1)
    + (j - 1) lda]), b / sacc: [k][lda] (default NaN).  Returns (a, b, sacc, ret [k][64]: every lane's return value)."""
    a = _d(a).copy()
    k = a.shape[0]
    if a.shape != (k, lda, lda):
        raise ValueError("a must be [k][lda][lda]")
    b = _d(b).copy() if b is not None else np.full((k, lda), np.nan)
    sacc = _d(sacc).copy() if sacc is not None else np.full((k, lda), np.nan)
    ns = np.ascontiguousarray(ns, dtype=np.int32)
    ret = np.full((k, 64), -7, np.int32)
    _check(lib().du_lbp(C.c_int(int(wave64)), C.c_int(LBP_OPS.index(op)), C.c_int(lda), C.c_int(k), _p(ns, C.c_int),
                        _p(a, C.c_double), _p(b, C.c_double), _p(sacc, C.c_double), _p(ret, C.c_int)), f"du_lbp({op})")
    return a, b, sacc, ret


# ------------------------------------------------------------------------------- dsq_alpha.h, dsq_k_alpha_rows*.hip
# (P, GRAD, PAD, NB, CELL) as devunit_alpha.hip instantiates alpha_eval (DU_EVAL_LIST)
EVAL_INST = [(P, g, d, nb, c)
             for P, g, d, c in ([(P, 1, 1, 0) for P in (1, 2, 3, 4, 8, 9, 12)] + [(2, 1, 0, 0), (9, 1, 0, 0), (2, 0, 0, 0),
                                                                                 (8, 0, 0, 0), (3, 1, 1, 1), (8, 1, 1, 1)])
             for nb in (1, 2, 4)]
CONST_COMPUTE, CONST_STORE, CONST_LOAD = 0, 1, 2
ROUTES = ["rows", "coef", "cell_mu"]
SENT_D, SENT_I, SENT_U8 = -7.0, -7, 0xEE  # what the outputs hold where no kernel wrote
STATE_D, STATE_I = ("x", "f", "g", "xold", "fold"), ("nfev", "it", "col", "done", "status")


def _xx(Xc):
    """x_i x_j of the cells' rows, packed lower triangle (dsq_linalg.h tri(i, j) = i (i + 1) / 2 + j)"""
    P = Xc.shape[1]
    ii = [i for i in range(P) for j in range(i + 1)]
    jj = [j for i in range(P) for j in range(i + 1)]
    return np.ascontiguousarray(Xc[:, ii] * Xc[:, jj])


def cus():
    return int(lib().du_cus())


def rowsc_tail(N, P, C_):
    """alpha_rowsc_tail: the many-cell row kernel's tail-table size for (N, P, C); 0: not eligible"""
    return int(lib().du_rowsc_tail(int(N), int(P), int(C_)))


def row_tail():
    return int(lib().du_row_tail())


def alpha_eval(inst, y, mu, X, la, la_hat, prior_var=1.0, cr_reg=True, prior_reg=False, cell_of=None, Xc=None):
    """alpha_eval<DeviceWave, *inst> for G genes of one design.  y / mu: [G][N], X: [N][P], la / la_hat: [G] ->
    (f [G][64], g [G][64], cst [G]): every lane's results and alpha_const of the rows.  The caller picks NB as k_alpha
    does: a gene whose largest count is >= 64 NB needs a larger memo (NB = 4 takes any count)."""
    P, grad, pad, nb, cell = inst
    y = np.ascontiguousarray(y, dtype=np.int32)
    mu = _d(mu)
    G, N = y.shape
    Xt = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    la, la_hat = _d(np.broadcast_to(la, (G,))), _d(np.broadcast_to(la_hat, (G,)))
    if mu.shape != (G, N) or Xt.shape != (P, N):
        raise ValueError("y / mu must be [G][N], X [N][P]")
    if nb < 4 and y.max() >= 64 * nb:
        raise ValueError("the memo does not cover the gene's largest count")
    co = xc = xx = None
    nc = 0
    if cell:
        co = np.ascontiguousarray(cell_of, dtype=np.int32)
        xc = _d(Xc)
        xx = _xx(xc)
        nc = xc.shape[0]
        if co.shape != (N,) or xc.shape[1] != P or co.min() < 0 or co.max() >= nc:
            raise ValueError("cell_of must be [N] with values below the number of rows of Xc [C][P]")
    f, g, cst = np.full((G, 64), np.nan), np.full((G, 64), np.nan), np.full(G, np.nan)
    fn = lib().du_alpha_eval
    fn.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                   C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    fn.restype = C.c_int
    _check(fn(P, grad, pad, nb, cell, _p(y, C.c_int32), _p(mu, C.c_double), N, _p(Xt, C.c_double), N, N, G,
              _p(la, C.c_double), _p(la_hat, C.c_double), float(prior_var), int(cr_reg), int(prior_reg),
              _p(co, C.c_int32), _p(xc, C.c_double), _p(xx, C.c_double), nc, _p(f, C.c_double), _p(g, C.c_double),
              _p(cst, C.c_double)), f"du_alpha_eval{inst}")
    return f, g, cst


def alpha_const(y, mu):
    """(alpha_const, alpha_const_max, the largest count) of every gene as all 64 lanes return them, each [G][64]"""
    y = np.ascontiguousarray(y, dtype=np.int32)
    mu = _d(mu)
    G, N = y.shape
    c, cm, mx = np.full((G, 64), np.nan), np.full((G, 64), np.nan), np.full((G, 64), SENT_I, np.int32)
    fn = lib().du_alpha_const
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                   C.POINTER(C.c_double), C.POINTER(C.c_int)]
    fn.restype = C.c_int
    _check(fn(_p(y, C.c_int32), _p(mu, C.c_double), N, N, G, _p(c, C.c_double), _p(cm, C.c_double), _p(mx, C.c_int)),
           "du_alpha_const")
    return c, cm, mx


def _rows_launch(entry, route, y, sf, cell_of, Xc, alpha_hat, min_disp, max_disp, min_mu, coef, cell_mu, genes,
                 prior_var, prior_reg, const_mode, eval_cap, nll_const):
    y = np.ascontiguousarray(y, dtype=np.int32)
    G, N = y.shape
    sf, xc, ah = _d(sf), _d(Xc), _d(alpha_hat)
    nc, P = xc.shape
    xx = _xx(xc)
    co = np.ascontiguousarray(cell_of, dtype=np.int32)
    cf = _d(coef) if coef is not None else None
    cm = _d(cell_mu) if cell_mu is not None else None
    lst = np.ascontiguousarray(genes, dtype=np.int32) if genes is not None else None
    n_list = lst.size if lst is not None else G
    if sf.shape != (N,) or co.shape != (N,) or ah.shape != (G,) or (cf is not None and cf.shape != (G, P)) or \
            (cm is not None and cm.shape != (G, nc)):
        raise ValueError("sf / cell_of [N], alpha_hat [G], coef [G][P], cell_mu [G][C]")
    if lst is not None and np.unique(lst).size != lst.size:
        raise ValueError("a gene may be listed once")
    nl = np.full(G, np.nan) if nll_const is None else _d(nll_const).copy()
    o = dict(alpha=np.full(G, SENT_D), conv=np.full(G, SENT_U8, np.uint8), nfev=np.full(G, SENT_I, np.int32),
             grid_list=np.full(G, SENT_I, np.int32), park_list=np.full(G, SENT_I, np.int32))
    gc, pc, wgc = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    sd, si = np.full((G, 5), np.nan), np.full((G, 5), SENT_I, np.int32)
    pd, pi, pu = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    common_in = [pi, C.c_int, C.c_int, C.c_int, pi, C.c_int, pd]
    tail = [C.c_double, pd, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, pd, pd, pu, pi, pi, pi, pi, pi,
            pd, pi]
    common = (_p(nl, C.c_double), _p(o["alpha"], C.c_double), _p(o["conv"], C.c_uint8), _p(o["nfev"], C.c_int32),
              _p(o["grid_list"], C.c_int32), C.byref(gc), _p(o["park_list"], C.c_int32), C.byref(pc), _p(sd, C.c_double),
              _p(si, C.c_int32))
    scal = (float(min_mu), _p(ah, C.c_double), float(min_disp), float(max_disp), float(prior_var), int(prior_reg),
            int(const_mode), int(eval_cap))
    if entry == "du_rows_trace":
        fn = lib().du_rows_trace
        fn.argtypes = [C.c_int] + common_in + [pd, pd, pi, pd, pd, C.c_int, C.c_int] + tail
        fn.restype = C.c_int
        rc = fn(ROUTES.index(route), _p(y, C.c_int32), N, N, G, _p(lst, C.c_int32), n_list, _p(cf, C.c_double),
                _p(cm, C.c_double), _p(sf, C.c_double), _p(co, C.c_int32), _p(xc, C.c_double), _p(xx, C.c_double), nc, P,
                *scal, *common)
    else:
        o.update(wg_alpha=np.full(G, SENT_D), wg_conv=np.full(G, SENT_U8, np.uint8), wg_nfev=np.full(G, SENT_I, np.int32),
                 wg_grid_list=np.full(G, SENT_I, np.int32))
        fn = lib().du_alpha_wg
        fn.argtypes = common_in + [pd, pi, pd, pd, C.c_int] + tail + [pd, pu, pi, pi, pi]
        fn.restype = C.c_int
        rc = fn(_p(y, C.c_int32), N, N, G, _p(lst, C.c_int32), n_list, _p(cf, C.c_double), _p(sf, C.c_double),
                _p(co, C.c_int32), _p(xc, C.c_double), _p(xx, C.c_double), P, *scal, *common, _p(o["wg_alpha"], C.c_double),
                _p(o["wg_conv"], C.c_uint8), _p(o["wg_nfev"], C.c_int32), _p(o["wg_grid_list"], C.c_int32), C.byref(wgc))
    _check(rc, f"{entry}({route}, P={P}, C={nc}, N={N}, eval_cap={eval_cap})")
    o["nll_const"] = nl
    o["grid_count"], o["park_count"] = int(gc.value), int(pc.value)
    o["grid"] = o["grid_list"][:max(0, min(G, gc.value))]
    o["parked"] = o["park_list"][:max(0, min(G, pc.value))]
    o["state"] = {**{k: sd[:, i] for i, k in enumerate(STATE_D)}, **{k: si[:, i] for i, k in enumerate(STATE_I)}}
    if entry != "du_rows_trace":
        o["wg_grid_count"] = int(wgc.value)
        o["wg_grid"] = o["wg_grid_list"][:max(0, min(G, wgc.value))]
    return o


def rows_trace(route, y, sf, cell_of, Xc, alpha_hat, min_disp, max_disp, min_mu, coef=None, cell_mu=None, genes=None,
               prior_var=1.0, prior_reg=False, const_mode=CONST_COMPUTE, eval_cap=0, nll_const=None):
    """One launch of k_alpha_rows (route "rows": P = C <= 4) or k_alpha_rows_c ("coef" / "cell_mu") with its own zeroed
    queue and counters; eval_cap = 0 runs every fit to its end.  y: [G][N]; genes: the list (default: all, in order).
    Returns a dict: alpha, conv, nfev, grid_list, park_list [G] (SENT_* where the kernel did not write), nll_const [G],
    grid / parked (the lists up to their counts), grid_count, park_count and state: per field of the parked genes'
    Lbfgsb1d (STATE_D, STATE_I) an array [G]."""
    return _rows_launch("du_rows_trace", route, y, sf, cell_of, Xc, alpha_hat, min_disp, max_disp, min_mu, coef, cell_mu,
                        genes, prior_var, prior_reg, const_mode, eval_cap, nll_const)


def alpha_wg(y, sf, cell_of, Xc, alpha_hat, min_disp, max_disp, min_mu, coef, eval_cap, genes=None, prior_var=1.0,
             prior_reg=False, const_mode=CONST_STORE, nll_const=None):
    """rows_trace("rows", ..., eval_cap >= 1) with the constants stored (or loaded), then k_alpha_wg on the parked
    states.  The dict of rows_trace for the row launch, and wg_alpha, wg_conv, wg_nfev, wg_grid_list [G], wg_grid,
    wg_grid_count: what k_alpha_wg wrote."""
    return _rows_launch("du_alpha_wg", "rows", y, sf, cell_of, Xc, alpha_hat, min_disp, max_disp, min_mu, coef, None,
                        genes, prior_var, prior_reg, const_mode, eval_cap, nll_const)


# ------------------------------------------------------------------------------- dsq_trend_grid.h, dsq_k_trend.hip
FIT_FIELDS = ("a0", "a1", "ok", "n_outer", "n_kept")
# the record of one (workgroup, point) of k_probe (devunit_trend.hip)
PROBE_TOT_LOAD, PROBE_KEPT0, PROBE_E0, PROBE_TOT_E0 = slice(0, 6), 6, slice(7, 10), slice(10, 16)
PROBE_KEPT1, PROBE_TOT_FILTER, PROBE_E1, PROBE_TOT_E1 = 16, slice(17, 23), slice(23, 26), slice(26, 32)


def trend_grid_blocks():
    return int(lib().du_trend_grid_blocks())


def trend_capacity(blocks):
    """genes the register path of `blocks` workgroups holds"""
    return blocks * int(lib().du_trend_threads()) * int(lib().du_trend_reg_genes())


def trend_fit_seq(cases, min_disp, max_disp, force_grid=0):
    """dsq::launch_trend_fit for every (disp, means) of `cases`, back to back on one TrendGridMem, one keep mask and one
    stream.  force_grid: -1 one workgroup, 0 the launcher's crossover, 1 the grid.  Returns out5 [len(cases)][5]
    (FIT_FIELDS), NaN where a launch wrote nothing."""
    d = np.ascontiguousarray(np.concatenate([np.asarray(c[0], np.float64).ravel() for c in cases]))
    m = np.ascontiguousarray(np.concatenate([np.asarray(c[1], np.float64).ravel() for c in cases]))
    off = np.zeros(len(cases) + 1, np.int32)
    off[1:] = np.cumsum([np.asarray(c[0]).size for c in cases])
    if d.size != m.size or any(np.asarray(c[0]).size != np.asarray(c[1]).size for c in cases):
        raise ValueError("disp and means of a case have one length")
    out = np.full((len(cases), 5), np.nan)
    fn = lib().du_trend_fit_seq
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.c_double, C.c_double,
                   C.c_int, C.POINTER(C.c_double)]
    fn.restype = C.c_int
    _check(fn(_p(d, C.c_double), _p(m, C.c_double), _p(off, C.c_int), len(cases), float(min_disp), float(max_disp),
              int(force_grid), _p(out, C.c_double)), f"du_trend_fit_seq(n={np.diff(off).tolist()}, grid={force_grid})")
    return out


def trend_fit(disp, means, min_disp, max_disp, force_grid=0, repeats=1):
    """`repeats` launches of one case (trend_fit_seq): out5 [repeats][5]"""
    return trend_fit_seq([(disp, means)] * repeats, min_disp, max_disp, force_grid)


def trend_glm(targets, cov, repeats=1):
    """dsq::launch_trend_glm, the raw one-fit mode: out5 [repeats][5]"""
    t, c = _d(targets).ravel(), _d(cov).ravel()
    if t.size != c.size:
        raise ValueError("targets and cov have one length")
    out = np.full((repeats, 5), np.nan)
    fn = lib().du_trend_glm
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double)]
    fn.restype = C.c_int
    _check(fn(_p(t, C.c_double), _p(c, C.c_double), t.size, int(repeats), _p(out, C.c_double)), f"du_trend_glm(n={t.size})")
    return out


def trend_probe(blocks, disp, means, min_disp, max_disp, points):
    """k_probe on 1 or trend_grid_blocks() workgroups: per point init_keep, eval, filter, eval and the six totals of
    every kind of pass, as EVERY workgroup's leader saw them.  Returns (records [blocks][points][32] - the PROBE_*
    slices -, the exchange's timeout flag)."""
    d, m = _d(disp).ravel(), _d(means).ravel()
    pts = _d(points).reshape(-1, 2)
    rec = int(lib().du_trend_probe_rec())
    out = np.full((blocks, pts.shape[0], rec), np.nan)
    to = C.c_uint(7)
    fn = lib().du_trend_probe
    fn.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double,
                   C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint)]
    fn.restype = C.c_int
    _check(fn(int(blocks), _p(d, C.c_double), _p(m, C.c_double), d.size, float(min_disp), float(max_disp),
              _p(pts, C.c_double), pts.shape[0], _p(out, C.c_double), C.byref(to)), f"du_trend_probe({blocks}, n={d.size})")
    return out, int(to.value)


def trend_loss_grad(cov, targets, a0, a1, keep=None):
    """dsq::launch_trend_loss_grad (k_trend) and the host's sum of its partials, in dsq_dev_trend_loss_grad's order:
    (loss, g0, g1, count) - all three sums are divided by the ONE count of NaN-free loss terms."""
    c, t = _d(cov).ravel(), _d(targets).ravel()
    k = np.ascontiguousarray(keep, dtype=np.uint8).ravel() if keep is not None else None
    nb = int(lib().du_trend_partials())
    part = np.full((nb, 4), np.nan)
    fn = lib().du_trend_loss_grad
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_int, C.c_double, C.c_double,
                   C.POINTER(C.c_double)]
    fn.restype = C.c_int
    _check(fn(_p(c, C.c_double), _p(t, C.c_double), _p(k, C.c_uint8), c.size, float(a0), float(a1), _p(part, C.c_double)),
           f"du_trend_loss_grad(n={c.size})")
    s = [0.0, 0.0, 0.0, 0.0]
    for row in part.tolist():
        for q in range(4):
            s[q] += row[q]
    cnt = s[3]
    with np.errstate(all="ignore"):
        return np.float64(s[0]) / cnt, -np.float64(s[1]) / cnt, -np.float64(s[2]) / cnt, cnt


# ------------------------------------------------------------------------------- dsq_shrink.h
SHRINK_WIDE_INST = ((16, 16), (32, 24), (32, 32), (48, 40), (48, 48))  # (PMAX, PB) as launch_shrink picks them


def shrink_rows(p, inst=None):
    """rows of Xt and entries of b / g per gene: p for shrink_fn<P>, PB for shrink_fn_wide<PMAX, PB>"""
    return p if inst is None else inst[1]


def shrink_pack(y, offset, X, b, inst=None):
    """The buffers of one shrink_fn call.  y / offset: [G][N], X: [G][N][p], b: [G][p] -> (y int32 [G][N], offset [G][N],
    Xt [G][rows][N], b [G][rows], g [G][lanes][rows] is the caller's): rows and entries at index >= p hold NaN, so a read
    beyond p poisons the result and never leaves the buffers."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    off, X, b = _d(offset), _d(X), _d(b)
    G, N = y.shape
    p = X.shape[2]
    rows = shrink_rows(p, inst)
    if off.shape != (G, N) or X.shape != (G, N, p) or b.shape != (G, p) or rows < p:
        raise ValueError("y / offset must be [G][N], X [G][N][p], b [G][p], p <= PB")
    Xt = np.full((G, rows, N), np.nan)
    Xt[:, :p] = X.transpose(0, 2, 1)
    bp = np.full((G, rows), np.nan)
    bp[:, :p] = b
    return y, off, np.ascontiguousarray(Xt), bp


def shrink_fn(y, offset, X, size, sigma0, sigma, sidx, b, inst=None):
    """shrink_fn<DeviceWave, p> (inst None, p <= 12: four genes per 256-thread block) or shrink_fn_wide<DeviceWave, *inst>
    at the run-time p (one gene per 64-thread block), every gene with its own rows (shrink_pack).  Returns (f0 [G][64]:
    the loss-only call, f1 [G][64]: the call with a gradient, g [G][64][rows]): what every lane holds; g is NaN before
    the call."""
    y, off, Xt, bp = shrink_pack(y, offset, X, b, inst)
    G, N = y.shape
    p, rows = X.shape[2], Xt.shape[1]
    sz, s0, s = (_d(np.broadcast_to(v, (G,))) for v in (size, sigma0, sigma))
    si = np.ascontiguousarray(np.broadcast_to(sidx, (G,)), dtype=np.int32)
    f0, f1, g = np.full((G, 64), np.nan), np.full((G, 64), np.nan), np.full((G, 64, rows), np.nan)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tail = [pi, pd, pd, C.c_int, C.c_int, C.c_int, pd, pd, pd, pi, pd, pd, pd, pd]
    args = (_p(y, C.c_int32), _p(off, C.c_double), _p(Xt, C.c_double), N, N, G, _p(sz, C.c_double), _p(s0, C.c_double),
            _p(s, C.c_double), _p(si, C.c_int32), _p(bp, C.c_double), _p(f0, C.c_double), _p(f1, C.c_double),
            _p(g, C.c_double))
    if inst is None:
        fn = lib().du_shrink_fn
        fn.argtypes, fn.restype = [C.c_int] + tail, C.c_int
        _check(fn(p, *args), f"du_shrink_fn(P={p}, N={N}, G={G})")
    else:
        fn = lib().du_shrink_fn_wide
        fn.argtypes, fn.restype = [C.c_int] * 3 + tail, C.c_int
        _check(fn(inst[0], inst[1], p, *args), f"du_shrink_fn_wide({inst}, p={p}, N={N}, G={G})")
    return f0, f1, g
