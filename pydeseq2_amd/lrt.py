"""Likelihood-ratio test of a nested reduced design (DESeq2's nbinomLRT), post hoc: the reduced fit by the IRLS launcher
of the LFC stage, the statistic by k_lrt (csrc/dsq_lrt.h).  ``DeseqPipeline.lrt`` delegates here."""
import ctypes as C
import os

import numpy as np

from ._design import DesignPack
from ._lib import DeviceScope, DsqCells, gather_rows_i32

_vp, c_double = C.c_void_p, C.c_double


def check_reduced_design(X, reduced_design):
    """The reduced design of a likelihood-ratio test against the full design X, as a float matrix - or a ValueError that
    names what is wrong with it.  Host only."""
    X = np.asarray(X, dtype=np.float64)
    Xr = np.asarray(reduced_design, dtype=np.float64)
    N, P = X.shape
    if Xr.ndim != 2:
        raise ValueError("The reduced design must be a samples x columns matrix.")
    if Xr.shape[0] != N:
        raise ValueError(f"The reduced design has {Xr.shape[0]} rows; the data set has {N} samples.")
    if not 1 <= Xr.shape[1] <= P - 1:
        raise ValueError(f"The reduced design must have between 1 and {P - 1} columns (fewer than the full design's "
                         f"{P}); it has {Xr.shape[1]}.")
    if np.isnan(Xr).any():
        raise ValueError("NaNs are not allowed in the reduced design.")
    if np.linalg.matrix_rank(Xr) != Xr.shape[1]:
        raise ValueError("The reduced design is rank deficient (its columns are linearly dependent).")
    if np.linalg.matrix_rank(np.hstack([Xr, X])) != np.linalg.matrix_rank(X):
        raise ValueError("The reduced design is not nested in the full design: its columns must lie in the span of the "
                         "full design's columns.")
    return np.ascontiguousarray(Xr)


def lrt(pipe, res, reduced_design):
    """Likelihood-ratio test of a nested reduced design (DESeq2's nbinomLRT) on the dispersions / LFCs of ``res``,
    post hoc like wald().  The reduced design is fitted by the IRLS launcher of the LFC stage (dsq_dev_lfc_fit2
    without epilogue, the reduced design's own DesignPack and cells) with the final dispersions, size factors and
    settings of fit_LFC, on the counts the final LFC was fitted on - the replaced counts of the last pass for the
    refitted genes - and k_lrt scores the two fits (csrc/dsq_lrt.h).
    Returns (pvalue, stat, reduced_LFC [G x P_reduced, natural log], reduced_converged); NaN for all-zero genes;
    genes whose counts all became zero in the refit: stat 0, pvalue 1 (the Wald rule, ds.py:357-360) and reduced_LFC 0."""
    Xr = check_reduced_design(pipe.design.X, reduced_design)
    G, N, ctx = pipe.G, pipe.N, pipe.ctx
    Dr = DesignPack(Xr, pipe.min_replicates)
    Pr = Dr.P
    nz = np.asarray(res.non_zero, dtype=bool)
    nzi = np.nonzero(nz)[0]
    Gn = len(nzi)
    pv, stt = np.full(G, np.nan), np.full(G, np.nan)
    beta_r, conv_r = np.full((G, Pr), np.nan), np.full(G, np.nan)
    refitted = np.asarray(res.refitted, dtype=bool) if res.refitted is not None else np.zeros(G, dtype=bool)
    keep = pipe._replace_keep
    if refitted.any() and (keep is None or keep["naz"] is None):
        raise RuntimeError("lrt(): the replaced counts of this result's refit are gone (another pass has run since)")
    with DeviceScope(ctx) as s:
        d_sf = s.upload(res.size_factors, dtype=np.float64)
        d_Xr, d_pinv = s.upload(Dr.Xt), s.upload(Dr.pinvXt)
        cells = None
        if Dr.cell_path and not os.environ.get("DSQ_NO_CELL_PATH"):
            cells = DsqCells(s.upload(Dr.cell_of).ptr, s.upload(Dr.Xc).ptr, s.upload(Dr.XXc).ptr, int(Dr.n_design_cells))

        def run(d_y, idx):
            """Reduced fit + statistic of the rows of d_y, which are the genes idx -> host vectors."""
            Gs = len(idx)
            d_bf = s.upload(np.asarray(res.LFC, dtype=np.float64)[idx])
            d_disp = s.upload(np.asarray(res.dispersions, dtype=np.float64)[idx])
            d_br, d_cv = s.empty((Gs, Pr), np.float64), s.empty((Gs,), np.uint8)
            d_out = s.empty((2 * Gs,), np.float64)
            pipe._k("lrt_reduced_fit", Gs, "dsq_dev_lfc_fit2", _vp(d_y.ptr), pipe.ldn, _vp(d_sf.ptr), _vp(d_Xr.ptr),
                    _vp(d_pinv.ptr), Dr.ldx, N, Gs, Pr, int(Dr.full_rank), _vp(d_disp.ptr), c_double(pipe.min_mu),
                    c_double(pipe.beta_tol), c_double(-30.0), c_double(30.0), pipe.irls_maxiter, _vp(d_br.ptr), None,
                    None, _vp(d_cv.ptr), None, C.byref(cells) if cells is not None else None,
                    None, None, c_double(0.0), None, None, None, None, None,
                    None, None, c_double(0.0), 0, None, None, None, None, 0)
            pipe._k("lrt", Gs, "dsq_dev_lrt", _vp(d_y.ptr), pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr),
                    pipe.design.ldx, pipe.P, _vp(d_Xr.ptr), Dr.ldx, Pr, N, Gs, _vp(d_disp.ptr), _vp(d_bf.ptr),
                    _vp(d_br.ptr), _vp(d_out.ptr), _vp(d_out.ptr + 8 * Gs))
            o = d_out.to_host()
            return o[Gs:], o[:Gs], d_br.to_host(), d_cv.to_host().astype(float)

        if Gn > 0:
            d_y = pipe.d_y if Gn == G else gather_rows_i32(s, ctx, pipe.d_y.ptr, pipe.ldn, nzi, N)
            pv[nzi], stt[nzi], beta_r[nzi], conv_r[nzi] = run(d_y, nzi)
        if refitted.any():  # their final LFC was fitted on the replaced counts: so is their reduced model
            rows = np.nonzero(~keep["naz"])[0]
            gidx = (keep["rp"] if keep["nzi"] is None else keep["nzi"][keep["rp"]])[rows]
            if not np.array_equal(np.sort(gidx), np.nonzero(refitted)[0]):
                raise RuntimeError("lrt(): the kept replaced counts belong to another result")
            d_y2 = gather_rows_i32(s, ctx, pipe._replace_buf.ptr, pipe.ldn, rows, N)
            pv[gidx], stt[gidx], beta_r[gidx], conv_r[gidx] = run(d_y2, gidx)
    z = np.asarray(res.new_all_zeroes, dtype=bool) if res.new_all_zeroes is not None else np.zeros(G, dtype=bool)
    if z.any():  # ds.py:357-360, dds.py:1380-1383
        stt[z], pv[z], beta_r[z] = 0.0, 1.0, 0.0
    return pv, stt, beta_r, conv_r
