"""Known-answer vectors for designs wider than 48 columns (the device-memory kernel family, up to 128 columns).

Run in the build container only (needs the reference; see make_golden.py, whose shim and case writer are reused):

    python tests/golden/make_golden_widest.py

* p65:  paired design, intercept + 63 subject indicators + condition, 64 subjects x 2 (every row distinct: IRLS mu_hat);
* p72:  one 72-level factor x 4 replicates (72 distinct rows = p: the linear-model mu_hat, more than 64 cells);
* p128: a 2-level and a 4-level factor + 123 continuous covariates (multiples of 1/64), N = 512 (the family of
  wider_cases).

Each case keeps 24 expressed genes, filtered as wider_cases filters them: the widths are what is tested here, the
rescue's behaviour on flat likelihoods is pinned by kat_hard.npz.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, kat_case, synth  # noqa: E402


def paired_design(n_subjects):
    N = 2 * n_subjects
    i = np.arange(N)
    subj, cond = i // 2, i % 2
    cols = [np.ones(N)] + [(subj == s) for s in range(1, n_subjects)] + [cond == 1]
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


def factor_design(levels, reps):
    N = levels * reps
    lv = np.arange(N) // reps
    cols = [np.ones(N)] + [(lv == k) for k in range(1, levels)]
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


def mixed_design(pw, N):
    rng = np.random.default_rng(100 + pw)
    a, b = np.arange(N) % 2, (np.arange(N) // 2) % 4
    cols = [np.ones(N), (a == 1)] + [(b == k) for k in (1, 2, 3)]
    while len(cols) < pw:  # multiples of 1/64: the fixture stays under 1 MB
        cols.append(np.round(rng.normal(0, 0.6, N) * 64) / 64)
    return np.column_stack([np.asarray(v, dtype=float) for v in cols])


def expressed(X, seed, n=24):
    for G in (80, 160, 320, 640):
        c = synth(G, X.shape[0], X, seed, eff=0.3)
        c = c[:, c.mean(0) >= 40][:, :n]
        if c.shape[1] == n:
            return c
    raise RuntimeError("not enough expressed genes")


def main():
    ut, gs, pp, di = _import_reference()
    cases = {"p65": (paired_design(64), 65), "p72": (factor_design(72, 4), 72), "p128": (mixed_design(128, 512), 128)}
    which = sys.argv[1:] or list(cases)
    for name in which:
        X, seed = cases[name]
        kat_case(name, expressed(X, seed), X, ut, gs, pp, di)


if __name__ == "__main__":
    main()
