"""The hidden-batch entry points on a cohort-sized matrix (60 000 genes x 1000 samples):

    python tools/probes/ruv_probe.py [--genes 60000] [--samples 1000] [--k 2] [--controls-g 10000] [--reps 5] [--json out.json]

Device time (dsq_timer_start/stop around each C entry point, counts resident, after a warm-up; median [min ... max] of
--reps runs) of dsq_dev_log_counts, dsq_dev_nb_residuals (deviance, P = 2), dsq_dev_project_out (q = k; GB/s against the
algorithmic 16 N G bytes) and the Gram of the controls; then the whole of pydeseq2_amd.ruv.ruv (wall time, uploads and
downloads included) for RUVg over --controls-g control genes and RUVr over all genes, and numpy on the same inputs on this
machine's host: log, the same residual formula, the SVD of the control matrix, lstsq and the subtraction."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydeseq2_amd import pca as _pca  # noqa: E402
from pydeseq2_amd import ruv  # noqa: E402
from pydeseq2_amd._lib import GENE_MAJOR, Context, DeviceArray, DeviceScope, _vp  # noqa: E402


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median=float(np.median(v)), min=float(v[0]), max=float(v[-1]))


def timed(ctx, reps, call):
    call()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        t.append(ctx.timer_stop())
    return stats(t)


def wall(reps, call):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t)


def show(name, r, extra=""):
    print(f"{name}: {r['median']:.3f} ms [{r['min']:.3f} ... {r['max']:.3f}]{extra}", flush=True)


def np_deviance(y, mu, alpha):
    r = 1.0 / alpha[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(y > 0, y * np.log(y / mu), 0.0)
    D = 2.0 * (A - (y + r) * np.log((y + r) / (mu + r)))
    return np.sign(y - mu) * np.sqrt(np.maximum(D, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--controls-g", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    G, N, k = a.genes, a.samples, a.k
    rng = np.random.default_rng(1)
    sf = np.exp(rng.normal(0, 0.25, N))
    cond, batch = np.arange(N) % 2, (np.arange(N) // 2) % 2
    X = np.column_stack([np.ones(N), cond]).astype(np.float64)
    beta = np.column_stack([rng.normal(3.0, 1.5, G), rng.normal(0, 0.3, G)])
    alpha = np.exp(rng.uniform(np.log(0.01), np.log(1.0), G))
    eta = beta @ X.T + np.outer(rng.normal(0, 0.5, G), batch - 0.5)
    y = rng.negative_binomial(1 / alpha[:, None], 1 / (1 + alpha[:, None] * sf[None, :] * np.exp(eta))).astype(np.int32)  # G x N
    y[:, 0] += 1  # (every gene has counts)
    ctl = np.sort(rng.choice(G, min(a.controls_g, G), replace=False)).astype(np.int32)
    ctx = Context(0)
    d_y, d_sf = DeviceArray.from_host(ctx, y), DeviceArray.from_host(ctx, sf)
    d_Xt, d_b, d_a = (DeviceArray.from_host(ctx, np.ascontiguousarray(v)) for v in (X.T, beta, alpha))
    d_Y, d_R, d_O = (DeviceArray(ctx, (G, N), np.float64) for _ in range(3))
    W = np.linalg.qr(rng.normal(size=(N, k)))[0]
    d_Pt, d_Bt = DeviceArray.from_host(ctx, np.ascontiguousarray(W.T)), DeviceArray.from_host(ctx, np.ascontiguousarray(W.T))
    out = {"genes": G, "samples": N, "k": k, "reps": a.reps, "device_ms": {}, "wall_ms": {}, "numpy_ms": {}}
    dev = out["device_ms"]
    dev["log_counts"] = timed(ctx, a.reps, lambda: ctx.call("dsq_dev_log_counts", _vp(d_y.ptr), N, _vp(d_sf.ptr), N, G, 1,
                                                            C.c_double(1.0), _vp(d_Y.ptr), N))
    show("dsq_dev_log_counts", dev["log_counts"], f"  {12.0 * N * G / dev['log_counts']['median'] / 1e6:.0f} GB/s of 12 N G bytes")
    dev["nb_residuals"] = timed(ctx, a.reps, lambda: ctx.call("dsq_dev_nb_residuals", _vp(d_y.ptr), N, _vp(d_sf.ptr),
                                                              _vp(d_Xt.ptr), N, 2, N, G, _vp(d_a.ptr), _vp(d_b.ptr), 0,
                                                              _vp(d_R.ptr), N))
    show("dsq_dev_nb_residuals (deviance, P = 2)", dev["nb_residuals"])
    for post, name in ((0, "project_out"), (2, "project_out_round")):
        dev[name] = timed(ctx, a.reps, lambda: ctx.call("dsq_dev_project_out", _vp(d_Y.ptr), N, _vp(d_Pt.ptr), _vp(d_Bt.ptr), N,
                                                        k, N, G, post, C.c_double(1.0), _vp(d_O.ptr), N, None))
        dev[name]["GBps"] = 16.0 * N * G / dev[name]["median"] / 1e6
        show(f"dsq_dev_project_out (q = {k}, post {post})", dev[name], f"  {dev[name]['GBps']:.0f} GB/s of 16 N G bytes")
    for name, sel in (("gram_controls_g", ctl), ("gram_all_genes", None)):
        R = _pca._Resident(d_Y, GENE_MAJOR)

        def gram():
            with DeviceScope(ctx) as s:
                _pca._gram_on_device(ctx, s, R, sel, True)

        out["wall_ms"][name] = wall(a.reps, gram)
        show(f"centred Gram, {len(sel) if sel is not None else G} genes (row means + dsq_dev_sample_gram, wall)", out["wall_ms"][name])
    counts = np.ascontiguousarray(y.T)
    out["wall_ms"]["ruv_g"] = wall(a.reps, lambda: ruv.ruv(ctx, d_y, sf, k, ctl))
    show(f"ruv(method='g', k = {k}, {len(ctl)} controls), resident counts, wall", out["wall_ms"]["ruv_g"])
    fit = (X, beta, alpha, np.ones(G, dtype=bool))
    out["wall_ms"]["ruv_r"] = wall(a.reps, lambda: ruv.ruv(ctx, d_y, sf, k, None, "r", fit=fit))
    show(f"ruv(method='r', k = {k}, {G} controls), resident counts, wall", out["wall_ms"]["ruv_r"])
    out["wall_ms"]["ruv_g_counts"] = wall(a.reps, lambda: ruv.ruv(ctx, d_y, sf, k, ctl, return_counts=True))
    show("... with the normalised counts downloaded (N x G doubles)", out["wall_ms"]["ruv_g_counts"])
    # numpy on the same inputs
    yf = counts.astype(np.float64)
    npm = out["numpy_ms"]
    npm["log_counts"] = wall(1, lambda: np.log(yf / sf[:, None] + 1.0))
    Y = np.log(yf / sf[:, None] + 1.0)
    mu = sf[:, None] * np.exp(X @ beta.T)
    npm["nb_residuals"] = wall(1, lambda: np_deviance(yf, mu, alpha))

    def np_ruvg():
        Yc = Y[:, ctl] - Y[:, ctl].mean(0)
        Wn = np.linalg.svd(Yc, full_matrices=False)[0][:, :k]
        return Y - Wn @ np.linalg.lstsq(Wn, Y, rcond=None)[0]

    npm["ruv_g"] = wall(1, np_ruvg)
    npm["project_out"] = wall(1, lambda: Y - W @ (W.T @ Y))
    for n_, r_ in npm.items():
        show(f"numpy {n_}", r_)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
