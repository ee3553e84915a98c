"""dsq_dev_ranksum on a cohort-sized matrix (60 000 genes x 1000 samples, two groups of 500):

    python tools/probes/rank_probe.py [--genes 60000] [--samples 1000] [--reps 5] [--scipy-genes 60000] [--json out.json]

Device time (dsq_timer_start/stop around the entry point, counts and size factors resident, after a warm-up) for S = 1 and
S = 4 strata, K = 1 and K = 8 comparisons (K = 8: the same two groups with other samples left out per comparison); medians
and the spread (min ... max).  Then scipy.stats.mannwhitneyu(axis=1, method="asymptotic") over the same normalised
matrix on this machine's host (wall time; --scipy-genes rows of it, scaled to all genes when fewer), and the largest
difference of the p-values of the K = 1, S = 1 run from scipy's."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydeseq2_amd import ranktest as rt  # noqa: E402
from pydeseq2_amd._lib import Context, DeviceArray, _vp  # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-genes", type=int, default=60000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    G, N = a.genes, a.samples
    rng = np.random.default_rng(1)
    sf = np.exp(rng.normal(0, 0.25, N))
    mean = np.exp(rng.normal(2.0, 2.0, G))  # most genes of a cohort are low: heavily tied rows
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mean[:, None] * sf[None, :])).astype(np.int32)
    group = (np.arange(N) % 2).astype(np.int8)
    strata4 = (np.arange(N) // 2) % 4
    ctx = Context(0)
    d_y, d_sf = DeviceArray.from_host(ctx, y), DeviceArray.from_host(ctx, sf)
    out = {"genes": G, "samples": N, "reps": a.reps, "runs": {}}
    p_first = None
    for S in (1, 4):
        for K in (1, 8):
            labels = np.tile(group, (K, 1))
            for k in range(1, K):  # other comparisons: 10 % of the samples left out, different ones each
                labels[k, rng.random(N) < 0.1] = -1
            ids = None if S == 1 else strata4
            P = rt.pack_layouts([rt.build_layout(labels[k], ids) for k in range(K)], labels)
            held = [DeviceArray.from_host(ctx, np.ascontiguousarray(x)) for x in
                    (P.order, P.seg, P.pad, P.nstrata, P.labels)]
            d_out = DeviceArray(ctx, (4 * K * G,), np.float64)
            o = d_out.ptr

            def call():
                ctx.call("dsq_dev_ranksum", _vp(d_y.ptr), N, _vp(d_sf.ptr), N, G, K, _vp(held[0].ptr), P.ldo,
                         _vp(held[1].ptr), _vp(held[2].ptr), P.lds, _vp(held[3].ptr), _vp(held[4].ptr), P.ldl, 0, _vp(o),
                         _vp(o + 8 * K * G), _vp(o + 16 * K * G), _vp(o + 24 * K * G), G)

            call()
            ctx.sync()
            t = []
            for _ in range(a.reps):
                ctx.timer_start()
                call()
                t.append(ctx.timer_stop())
            r = stats(t)
            r["L"] = int(P.pad.max())
            out["runs"][f"S{S}_K{K}"] = r
            print(f"S = {S}  K = {K}  L = {r['L']}: device ms {r['median']:.2f} [{r['min']:.2f} ... {r['max']:.2f}]", flush=True)
            if S == 1 and K == 1:
                p_first = d_out.to_host()[G:2 * G].copy()
            for d in held + [d_out]:
                d.free()
    from scipy.stats import mannwhitneyu

    n = min(G, a.scipy_genes)
    v = y[:n].astype(np.float64) / sf[None, :]
    t0 = time.perf_counter()
    res = mannwhitneyu(v[:, group == 1], v[:, group == 0], axis=1, use_continuity=True, method="asymptotic")
    wall = time.perf_counter() - t0
    ok = np.isfinite(res.pvalue)
    out["scipy"] = dict(genes=n, wall_s=wall, wall_s_all_genes=wall * G / n,
                        max_rel_p_diff=float(np.max(np.abs(p_first[:n][ok] - res.pvalue[ok]) / res.pvalue[ok])))
    print(f"scipy.stats.mannwhitneyu(axis=1) on {n} genes: {wall:.2f} s on the host ({wall * G / n:.2f} s for {G}); largest "
          f"relative difference of the p-values {out['scipy']['max_rel_p_diff']:.3g}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
