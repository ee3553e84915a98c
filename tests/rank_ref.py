"""Reference of the rank-sum test for the tests: the statement in numpy, scipy.stats.rankdata per stratum,
Python integers for the tie term, mpmath for z and the p-value.  Shared by tests/test_rank_host.py and
tests/test_gpu_rank.py; also the error bounds both hold the code to."""
import math
from fractions import Fraction

import mpmath
import numpy as np
from scipy.stats import rankdata

mpmath.mp.dps = 50

U2 = 2.0 ** -52           # one rounding, counted in full (the headroom over 2^-53 pays for the second-order terms)
U = 2.0 ** -53
SUB = 2.0 ** -1074
TINY = 2.2250738585072014e-308
MAXLOG = 7.09782712893383996843e2  # dsq_math.h, norm_sf: flushed to 0 where cephes flushes
ALT_CODE = {None: 0, "greater": 3, "less": 4}


def normed(y_row, sf):
    """v = (double)y / sf, IEEE division: what the device stages and ranks."""
    return np.asarray(y_row, dtype=np.float64) / np.asarray(sf, dtype=np.float64)


def reference(y_row, sf, labels, strata, alt):
    """One gene, one comparison.  labels: 1 / 0 / -1 per sample; strata: ids per sample or None.
    Returns a dict: usum, ties (floats holding the exact values), stat, p (mpmath), and what the bounds need."""
    lab = np.asarray(labels)
    v = normed(y_row, sf)
    used = lab >= 0
    ids = np.zeros(len(lab), np.int64) if strata is None else np.asarray(strata)
    levels = np.unique(ids[used])
    S = len(levels)
    usum, ties, pairs = Fraction(0), 0, 0
    W, V, A, n_contrib = mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0), 0
    for lv in levels:
        m = used & (ids == lv)
        x, l = v[m], lab[m]
        n, n1 = int(m.sum()), int((l == 1).sum())
        n2 = n - n1
        if n1 * n2 == 0 or n < 2:
            continue
        r = rankdata(x, method="average")
        R = Fraction(float(r[l == 1].sum()))  # (a sum of half-integers below 2^53: exact in any order)
        Us = R - Fraction(n1 * (n1 + 1), 2)
        _, cnt = np.unique(x, return_counts=True)
        Ts = sum(int(t) ** 3 - int(t) for t in cnt)
        usum += Us
        ties += Ts
        pairs += n1 * n2
        n_contrib += 1
        w = mpmath.mpf(1) if S == 1 else mpmath.mpf(1) / (n + 1)
        D = mpmath.mpf(Us.numerator) / Us.denominator - mpmath.mpf(n1 * n2) / 2
        W += w * D
        A += abs(w * D)
        V += w * w * mpmath.mpf(n1 * n2 * ((n ** 3 - n) - Ts)) / (12 * n * (n - 1))
    out = dict(usum=float(usum), ties=float(ties), pairs=pairs, S=S, n_contrib=n_contrib)
    assert Fraction(out["usum"]) == usum and int(out["ties"]) == ties
    if V == 0:
        out.update(stat=mpmath.mpf(0), p=mpmath.mpf(1), stat_tol=0.0, degenerate=True, z_for_p=mpmath.mpf(0))
        return out
    sd = mpmath.sqrt(V)
    c = mpmath.mpf("0.5") if S == 1 else mpmath.mpf(0)
    if alt is None:
        z = max(abs(W) - c, mpmath.mpf(0)) / sd
        stat, zp = mpmath.sign(W) * z, z
        p = min(mpmath.mpf(1), mpmath.erfc(z / mpmath.sqrt(2)))
    elif alt == "greater":
        stat = (W - c) / sd
        zp = stat
        p = mpmath.erfc(zp / mpmath.sqrt(2)) / 2
    else:
        stat = (W + c) / sd
        zp = -stat
        p = mpmath.erfc(zp / mpmath.sqrt(2)) / 2
    # ---- the bound on |stat - reference|
    # S == 1: W and the numerator |W| -+ c are exact half-integers; V = (n1 n2 * B) / (12 N (N - 1)) is one product and
    #   one quotient of exact integers, then one square root and one quotient: 4 roundings, 4 * 2^-52 relative.
    # S > 1 (c = 0), over the C contributing strata: w_s = 1 / (N_s + 1) is one rounding and w_s * D_s another, the C - 1
    #   additions of W one each relative to a partial sum that A = sum |w_s D_s| bounds: |dW| <= (C + 1) u A.
    #   A term of V: w * w (two roundings of w and the product's: 3), n1 n2 * B and its quotient (2), their product (1);
    #   the terms are positive, so the C - 1 additions add one rounding each: dV / V <= (C + 5) u; the square root halves
    #   that and adds its own, the final quotient one more: |dstat| <= u ((C + 1) A / sd + |stat| ((C + 5) / 2 + 2)).
    #   (Fused multiply-adds only drop roundings from this count.)
    if S == 1:
        tol = 4 * U2 * abs(float(stat))
    else:
        C = n_contrib
        tol = U2 * ((C + 1) * float(A / sd) + abs(float(stat)) * ((C + 5) / 2 + 2))
    out.update(stat=stat, p=p, stat_tol=tol, degenerate=False, z_for_p=zp)
    return out


def p_tolerance(ref):
    """|p - reference| allowed, or None where the reference lies within 1e-9 of norm_sf's flush to zero (not decided
    here), or "zero" where the code must return exactly 0 (beyond the flush, as scipy.stats.norm.sf does).
    tests/test_devunit_math.py::test_norm_sf holds norm_sf(z) to (1e-13 + 2u |a| (2|a| + 1.13)) relative (+ one
    subnormal spacing), a = z / sqrt 2; an error dz of the argument moves log sf by |dz / sqrt 2| times the same
    derivative bound |erfc'(a) / erfc(a)| <= 2|a| + 1.13."""
    z = float(ref["z_for_p"])
    a = z * 0.70710678118654752440
    if a > 0 and a * a > MAXLOG * (1 + 1e-9):
        return "zero"
    if a > 0 and a * a > MAXLOG * (1 - 1e-9):
        return None
    p = float(ref["p"])
    rel = 1e-13 + (2 * U * abs(a) + ref["stat_tol"] / math.sqrt(2)) * (2 * abs(a) + 1.13)
    return rel * p + (SUB if p < TINY else 0.0)


def scipy_mwu(y_row, sf, labels, alt):
    """scipy.stats.mannwhitneyu of the tested against the reference samples (S == 1 only)."""
    from scipy.stats import mannwhitneyu

    lab = np.asarray(labels)
    v = normed(y_row, sf)
    r = mannwhitneyu(v[lab == 1], v[lab == 0], use_continuity=True, method="asymptotic",
                     alternative={None: "two-sided", "greater": "greater", "less": "less"}[alt])
    return float(r.statistic), float(r.pvalue)


# ------------------------------------------------------------------------------------------------ whole cases
_REF = {}


def case_reference(case, alt):
    """[K][G] references of a case of tests/rank_cases.py, computed once per process."""
    key = (case.name, alt)
    if key not in _REF:
        _REF[key] = [[reference(case.y[g, :case.N], case.sf, case.labels[k], case.strata, alt) for g in range(case.G)]
                     for k in range(case.K)]
    return _REF[key]


def scipy_tolerance(case, k, g, ref):
    """How far scipy.stats.mannwhitneyu's own p-value may lie from the exact one (S == 1, relative to p).  scipy forms
    s = sqrt(n1 n2 / 12 * ((n + 1) - T / (n (n - 1)))): the quotient q and the difference b = (n + 1) - q are one rounding
    each, relative to q + b = n + 1 where the difference cancels: db / b <= u (n + 1) / b; n1 n2 / 12, the product, the
    square root (which halves what precedes it) and the final quotient one each: dz / z <= u ((n + 1) / (2 b) + 3.5).
    Its norm.sf is held to the bound of norm_sf."""
    lab = case.labels[k]
    n = int((lab >= 0).sum())
    b = (n + 1) - ref["ties"] / (n * (n - 1))
    z = float(ref["z_for_p"])
    a = abs(z) * 0.70710678118654752440
    dz = U2 * ((n + 1) / (2 * b) + 3.5) * abs(z)
    return 1e-13 + (2 * U * a + dz / math.sqrt(2)) * (2 * a + 1.13)


def check_case(case, alt, got, what, scipy_extra=None):
    """got: dict of [K][G] arrays (stat, pvalue, usum, ties).  Asserts every bound of the statement; returns the worst
    figures: stat error / bound, p error / bound, and for S == 1 the worst relative deviation from scipy's p-value.
    scipy_extra: the relative deviation from scipy's p-value allowed on top of the p bound (the GPU tests: what the host
    build shows); None: this module's own bound on scipy's error (scipy_tolerance)."""
    refs = case_reference(case, alt)
    worst = dict(stat=0.0, p=0.0, scipy=0.0)
    for k in range(case.K):
        for g in range(case.G):
            r, tag = refs[k][g], f"{what} {case.name} alt={alt} k={k} g={g}"
            st, pv, us, ti = (float(got[n][k, g]) for n in ("stat", "pvalue", "usum", "ties"))
            assert np.float64(us).view(np.int64) == np.float64(r["usum"]).view(np.int64), (tag, us, r["usum"])
            assert np.float64(ti).view(np.int64) == np.float64(r["ties"]).view(np.int64), (tag, ti, r["ties"])
            if r["degenerate"]:
                assert st == 0.0 and pv == 1.0, (tag, st, pv)
                continue
            es = abs(st - float(r["stat"]))
            assert es <= r["stat_tol"], (tag, st, float(r["stat"]), es, r["stat_tol"])
            if r["stat_tol"] > 0:
                worst["stat"] = max(worst["stat"], es / r["stat_tol"])
            tol = p_tolerance(r)
            if tol == "zero":
                assert pv == 0.0, (tag, pv)
            elif tol is not None:
                ep = abs(pv - float(r["p"]))
                assert ep <= tol, (tag, pv, float(r["p"]), ep, tol)
                worst["p"] = max(worst["p"], ep / tol)
            if r["S"] == 1:
                u_sp, p_sp = scipy_mwu(case.y[g, :case.N], case.sf, case.labels[k], alt)
                assert u_sp == us, (tag, u_sp, us)
                if p_sp > 0 and tol not in ("zero", None):
                    dev = abs(pv - p_sp) / p_sp
                    extra = scipy_tolerance(case, k, g, r) if scipy_extra is None else scipy_extra
                    assert abs(pv - p_sp) <= extra * p_sp + tol, (tag, pv, p_sp, dev, extra, tol)
                    worst["scipy"] = max(worst["scipy"], dev)
                elif p_sp == 0:
                    assert pv == 0.0, (tag, pv)
    return worst
