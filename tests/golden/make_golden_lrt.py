"""Known-answer vectors for the likelihood-ratio test of a reduced design -> kat_lrt.npz.

Run in the build container only (needs the reference; see make_golden.py, whose shim is reused):

    python tests/golden/make_golden_lrt.py

For each of six KAT inputs (at most 24 genes, dispersions clip(map_alpha) as the shrink fixtures use them) the
unmodified reference fits the full and a nested reduced design with utils.irls_solver, and the statistic is
2 (nb_nll_reduced - nb_nll_full) with utils.nb_nll on the unthresholded mu the solver returns, the p-value
scipy.stats.chi2.sf(stat, df).  The same statistic evaluated in np.longdouble is stored next to it, and
stat_ref_err = max |float64 - longdouble|: the reference's own cancellation error (a difference of two sums of 1e3-1e4).

| case | reduced design                                   | df  |
| p2   | ~1                                               | 1   |
| p4   | intercept + first non-intercept column           | 2   |
| p8m  | the five factor columns (three continuous dropped) | 3 |
| p16  | ~1                                               | 15  |
| p65  | the 64 subject columns (condition dropped)       | 1   |
| p128 | columns 0 ... 4                                  | 123 |

A gene whose reduced (or full) fit does not converge in the reference is dropped (flags are compared strictly by the
tests); at most 2 of 24 per case.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, _import_reference  # noqa: E402

CASES = {"p2": [0], "p4": [0, 1], "p8m": [0, 1, 2, 3, 4], "p16": [0], "p65": list(range(64)), "p128": [0, 1, 2, 3, 4]}
G_MAX = 24


def nll_longdouble(y, mu, alpha):
    """utils.nb_nll without its lgamma terms (they are those of the other model and cancel exactly), in long double."""
    from numpy import longdouble as L

    y, mu, r = y.astype(L), mu.astype(L), L(1.0) / L(alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        ylog = np.where(y > 0, y * np.log(mu), L(0.0))
    return ((y + r) * np.log(r + mu) - ylog).sum()


def main():
    from scipy.stats import chi2

    ut, _gs, _pp, _di = _import_reference()
    out = {}
    for case, cols in CASES.items():
        k = np.load(os.path.join(HERE, f"kat_{case}.npz"))
        counts, X, sf = k["counts"], k["X"], k["sf"]
        N = counts.shape[0]
        disp = np.clip(k["map_alpha"], 1e-8, max(10, N))
        Xr = np.ascontiguousarray(X[:, cols])
        df = X.shape[1] - Xr.shape[1]
        assert np.linalg.matrix_rank(np.hstack([Xr, X])) == np.linalg.matrix_rank(X) == X.shape[1]
        rows, dropped = [], 0
        for g in range(min(counts.shape[1], G_MAX)):
            y = counts[:, g]
            bf, muf, _, cf = ut.irls_solver(y, sf, X, disp[g], 0.5, 1e-8)
            br, mur, _, cr = ut.irls_solver(y, sf, Xr, disp[g], 0.5, 1e-8)
            if not (cf and cr):
                dropped += 1
                continue
            stat = 2.0 * (float(ut.nb_nll(y, mur, disp[g])) - float(ut.nb_nll(y, muf, disp[g])))
            stat_ld = 2.0 * (nll_longdouble(y, mur, disp[g]) - nll_longdouble(y, muf, disp[g]))
            rows.append((g, bf, br, cf, cr, stat, float(stat_ld), float(chi2.sf(stat, df)), float(chi2.sf(float(stat_ld), df))))
        assert dropped <= 2, (case, dropped)
        gi = np.array([r[0] for r in rows])
        stat, stat_ld = np.array([r[5] for r in rows]), np.array([r[6] for r in rows])
        out[f"{case}_genes"] = gi
        out[f"{case}_cols"] = np.array(cols)
        out[f"{case}_df"] = np.array(df)
        out[f"{case}_disp"] = disp[gi]
        out[f"{case}_beta_full"] = np.stack([r[1] for r in rows])
        out[f"{case}_beta_reduced"] = np.stack([r[2] for r in rows])
        out[f"{case}_conv_full"] = np.array([r[3] for r in rows], dtype=bool)
        out[f"{case}_conv_reduced"] = np.array([r[4] for r in rows], dtype=bool)
        out[f"{case}_stat"], out[f"{case}_stat_ld"] = stat, stat_ld
        out[f"{case}_p"] = np.array([r[7] for r in rows])
        out[f"{case}_p_ld"] = np.array([r[8] for r in rows])
        out[f"{case}_stat_ref_err"] = np.array(np.abs(stat - stat_ld).max())
        print(case, "genes", len(rows), "dropped", dropped, "df", df, "stat", stat.min(), stat.max(),
              "ref_err", float(out[f"{case}_stat_ref_err"]))
    np.savez_compressed(os.path.join(HERE, "kat_lrt.npz"), **out)


if __name__ == "__main__":
    main()
