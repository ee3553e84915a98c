"""One dsq_dev_wald_multi launch against K launches of dsq_dev_wald on the benchmark's c4 shape (60 000 genes x 500 samples,
the three-factor design, p = 8), K in {1, 8, 28}:

    python tools/probes/wald_multi_probe.py [--genes 60000] [--samples 500] [--reps 15] [--json out.json]

Device time (dsq_timer_start/stop around the entry points, inputs resident: what the call costs on the stream, the small
ridge / contrast uploads of dsq_dev_wald included) and host wall time of DeseqPipeline.wald_multi against K x
DeseqPipeline.wald (uploads, launch, download).  After a warm-up the two variants alternate within one process; medians
and the spread (min ... max) of each are printed, for K = 1 also the run-to-run spread of the single launch."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydeseq2_amd import DeseqPipeline  # noqa: E402
from pydeseq2_amd._lib import DeviceArray  # noqa: E402
from pydeseq2_amd.synth import synth_counts  # noqa: E402

_vp = C.c_void_p


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    counts, X = synth_counts(a.genes, a.samples, "3factor", 3)
    pipe = DeseqPipeline(counts, X, device=0)
    res = pipe.deseq2()
    ctx, G, N, P = pipe.ctx, pipe.G, pipe.N, pipe.P
    up = lambda v: DeviceArray.from_host(ctx, np.ascontiguousarray(v, dtype=np.float64))  # noqa: E731
    d_sf, d_beta, d_disp = up(res.size_factors), up(res.LFC), up(res.dispersions)
    ridge = np.ascontiguousarray(np.diag(np.repeat(1e-6, P)))
    out = {"genes": G, "samples": N, "P": P, "reps": a.reps, "K": {}}
    for K in (1, 8, 28):
        cons = np.ascontiguousarray(np.random.default_rng(K).normal(size=(K, P)))
        d_con = up(cons)
        d_m, d_s = DeviceArray(ctx, (3 * G * K,), np.float64), DeviceArray(ctx, (3 * G,), np.float64)

        def multi():
            ctx.call("dsq_dev_wald_multi", None, pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr), pipe.design.ldx, N, G, P,
                     _vp(d_disp.ptr), _vp(d_beta.ptr), _vp(ridge.ctypes.data), _vp(d_con.ptr), K, C.c_double(0.0), 0,
                     _vp(d_m.ptr), _vp(d_m.ptr + 8 * G * K), _vp(d_m.ptr + 16 * G * K))

        def singles():
            for k in range(K):
                ctx.call("dsq_dev_wald", None, pipe.ldn, _vp(d_sf.ptr), _vp(pipe.d_Xt.ptr), pipe.design.ldx, N, G, P,
                         _vp(d_disp.ptr), _vp(d_beta.ptr), _vp(ridge.ctypes.data), _vp(cons[k].ctypes.data),
                         C.c_double(0.0), 0, _vp(d_s.ptr), _vp(d_s.ptr + 8 * G), _vp(d_s.ptr + 16 * G))

        def dev_ms(f):
            ctx.timer_start()
            f()
            return ctx.timer_stop()

        def wall_ms(f):
            ctx.sync()
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3

        host_multi = lambda: pipe.wald_multi(res, cons)  # noqa: E731
        host_singles = lambda: [pipe.wald(res, c) for c in cons]  # noqa: E731
        for f in (multi, singles, host_multi, host_singles):  # warm-up: code objects, allocations
            f()
            f()
        ctx.sync()
        t = {"multi_dev": [], "singles_dev": [], "multi_wall": [], "singles_wall": []}
        for _ in range(a.reps):  # alternating
            t["multi_dev"].append(dev_ms(multi))
            t["singles_dev"].append(dev_ms(singles))
            t["multi_wall"].append(wall_ms(host_multi))
            t["singles_wall"].append(wall_ms(host_singles))
        r = {k: stats(v) for k, v in t.items()}
        r["dev_ratio_singles_over_multi"] = r["singles_dev"]["median"] / r["multi_dev"]["median"]
        r["wall_ratio_singles_over_multi"] = r["singles_wall"]["median"] / r["multi_wall"]["median"]
        # same numbers from both routes (the first contrast)
        pm, p1 = pipe.wald_multi(res, cons)[0][0], pipe.wald(res, cons[0])[0]
        r["first_contrast_bits_equal"] = bool(np.array_equal(pm, p1, equal_nan=True))
        out["K"][K] = r
        print(f"K = {K:2d}  device ms: multi {r['multi_dev']['median']:.3f} [{r['multi_dev']['min']:.3f} ... "
              f"{r['multi_dev']['max']:.3f}]  {K} x single {r['singles_dev']['median']:.3f} [{r['singles_dev']['min']:.3f} ... "
              f"{r['singles_dev']['max']:.3f}]  ratio {r['dev_ratio_singles_over_multi']:.2f}", flush=True)
        print(f"        host wall ms: wald_multi {r['multi_wall']['median']:.2f} [{r['multi_wall']['min']:.2f} ... "
              f"{r['multi_wall']['max']:.2f}]  {K} x wald {r['singles_wall']['median']:.2f} [{r['singles_wall']['min']:.2f} ... "
              f"{r['singles_wall']['max']:.2f}]  ratio {r['wall_ratio_singles_over_multi']:.2f}  "
              f"bits equal: {r['first_contrast_bits_equal']}", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    pipe.close()


if __name__ == "__main__":
    main()
