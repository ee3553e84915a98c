"""dsq_dev_ash on 60 000 genes, K in {1, 8, 28} contrasts drawn as the plain sets of tests/ash_cases are:

    python tools/probes/ash_probe.py [--genes 60000] [--reps 7] [--json out.json]

Device time (dsq_timer_start/stop around the entry point, inputs resident, after a warm-up): one call for K contrasts
against K single-contrast calls, alternating within one process; medians and the spread (min ... max).  For the first
contrast also the numpy restatement on the host (tests/ash_ref: the dense n x M matrix, stopped at the same 1e-8 rule)
with its wall time and the largest difference of the posterior means, and the host wall time of pydeseq2_amd.ash.ash
(grid, upload, the call, download, s-values)."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydeseq2_amd._lib import Context, DeviceArray  # noqa: E402
from pydeseq2_amd.ash import ash, mixsd_grid  # noqa: E402
from tests import ash_ref  # noqa: E402

_vp = C.c_void_p


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def draw(G, seed):
    rng = np.random.default_rng(seed)
    s = np.exp(rng.normal(-1.5, 0.6, G))
    eff = np.where(rng.random(G) < 0.3, rng.normal(0, 1.0, G), 0.0)
    return eff + s * rng.normal(size=G), s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    G = a.genes
    ctx = Context(0)
    out = {"genes": G, "reps": a.reps, "K": {}}
    for K in (1, 8, 28):
        bs = [draw(G, 100 + k) for k in range(K)]
        b, s = np.stack([x[0] for x in bs]), np.stack([x[1] for x in bs])
        grids = [mixsd_grid(b[k], s[k]) for k in range(K)]
        mk = np.array([len(g) for g in grids], np.int32)
        ldm = int(mk.max())
        sd = np.zeros((K, ldm))
        for k in range(K):
            sd[k, :mk[k]] = grids[k]
        d_b, d_s, d_sd, d_m = (DeviceArray.from_host(ctx, x) for x in (b, s, sd, mk))
        d_pi, d_o = DeviceArray(ctx, (K * ldm,), np.float64), DeviceArray(ctx, (3 * K * G + 2 * K,), np.float64)
        d_it, d_cv = DeviceArray(ctx, (K,), np.int32), DeviceArray(ctx, (K,), np.uint8)

        def call(k0, kn):
            o = d_o.ptr
            ctx.call("dsq_dev_ash", _vp(d_b.ptr + 8 * k0 * G), _vp(d_s.ptr + 8 * k0 * G), G, G, kn, _vp(d_sd.ptr + 8 * k0 * ldm),
                     _vp(d_m.ptr + 4 * k0), ldm, 100, _vp(d_pi.ptr + 8 * k0 * ldm), _vp(o + 8 * k0 * G),
                     _vp(o + 8 * (K + k0) * G), _vp(o + 8 * (2 * K + k0) * G), _vp(d_it.ptr + 4 * k0), _vp(d_cv.ptr + k0),
                     _vp(o + 8 * (3 * K * G + k0)), _vp(o + 8 * (3 * K * G + K + k0)))

        def multi():
            call(0, K)

        def singles():
            for k in range(K):
                call(k, 1)

        def dev_ms(f):
            ctx.timer_start()
            f()
            return ctx.timer_stop()

        for f in (multi, singles):
            f()
        ctx.sync()
        t = {"multi_dev": [], "singles_dev": []}
        for _ in range(a.reps):
            t["multi_dev"].append(dev_ms(multi))
            t["singles_dev"].append(dev_ms(singles))
        r = {k: stats(v) for k, v in t.items()}
        it, cv = d_it.to_host(), d_cv.to_host()
        r.update(M=mk.tolist(), n_iter=it.tolist(), converged=bool(cv.all()))
        pm0 = d_o.to_host()[:G]
        t0 = time.perf_counter()
        res = ash(ctx, b, s)
        r["ash_wall_ms"] = (time.perf_counter() - t0) * 1e3
        r["facade_equals_raw_call"] = bool(np.array_equal(res.post_mean[0], pm0))
        if K == 1:
            t0 = time.perf_counter()
            L, _ = ash_ref.lik(b[0], s[0], grids[0])
            x, n_it, _ = ash_ref.fit(L, 1e-8)
            e = ash_ref.posterior(b[0], s[0], grids[0], x / x.sum())
            r["numpy_wall_ms"] = (time.perf_counter() - t0) * 1e3
            r["numpy_iterations"] = int(n_it)
            r["post_mean_max_diff_vs_numpy"] = float(np.abs(pm0 - e[0]).max())
        out["K"][K] = r
        print(f"K = {K:2d}  M {mk.min()}-{mk.max()}  iterations {it.min()}-{it.max()}  device ms: one call "
              f"{r['multi_dev']['median']:.3f} [{r['multi_dev']['min']:.3f} ... {r['multi_dev']['max']:.3f}]  {K} x single "
              f"{r['singles_dev']['median']:.3f} [{r['singles_dev']['min']:.3f} ... {r['singles_dev']['max']:.3f}]  "
              f"ash() wall {r['ash_wall_ms']:.1f} ms  converged {r['converged']}", flush=True)
        if K == 1:
            print(f"        numpy restatement: {r['numpy_wall_ms']:.0f} ms, {n_it} iterations; largest |posterior mean "
                  f"difference| {r['post_mean_max_diff_vs_numpy']:.3g}", flush=True)
        for d in (d_b, d_s, d_sd, d_m, d_pi, d_o, d_it, d_cv):
            d.free()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
