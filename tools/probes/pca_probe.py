"""Sample PCA / sample distances at the benchmark shapes:

    python tools/probes/pca_probe.py [--genes 60000] [--reps 3] [--json out.json]

60 000 x 30 and 60 000 x 1000 over all genes (the distances' shape) and the 500 most variable genes of 60 000 x 1000
(plotPCA's shape).  Device time with dsq_timer_start/stop around each entry point, input resident, after a warm-up:
dsq_dev_row_meanvar, dsq_dev_sample_gram (pack + Gram + reduction; the kernels one by one: run this under
`rocprofv3 --kernel-trace --stats`), dsq_dev_gram_dist; the Gram's FLOP/s as 2 K N (N + 1) / 2 over the entry's time.
Beside them the wall time of pydeseq2_amd.pca.pca / sample_distances from a host matrix (upload, device, eigh) and of the
same result from numpy on the host (var + X~ X~^T), with the largest difference between the two."""
import argparse
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydeseq2_amd import pca as P  # noqa: E402
from pydeseq2_amd._lib import SAMPLE_MAJOR, Context, DeviceArray  # noqa: E402

_vp = C.c_void_p


def timed(ctx, reps, name, *args):
    ctx.call(name, *args)  # warm-up
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        ctx.call(name, *args)
        ms.append(ctx.timer_stop())
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    G = a.genes
    ctx = Context(0)
    out = {"genes": G, "reps": a.reps, "shapes": []}
    for N, ntop in ((30, None), (1000, None), (1000, 500)):
        rng = np.random.default_rng([N, G])
        x = rng.uniform(4.0, 14.0, G) + rng.normal(0.0, 0.5, (N, G)) + np.outer(rng.normal(size=N), rng.normal(0, 0.3, G))
        t0 = time.perf_counter()
        d_x = DeviceArray.from_host(ctx, x)
        ctx.sync()
        t_up = time.perf_counter() - t0
        d_mv = DeviceArray(ctx, 2 * G, np.float64)
        r = dict(N=N, G=G, ntop=ntop, upload_s=t_up)
        r["row_meanvar_ms"] = timed(ctx, a.reps, "dsq_dev_row_meanvar", _vp(d_x.ptr), SAMPLE_MAJOR, N, G, G, _vp(d_mv.ptr),
                                    _vp(d_mv.ptr + 8 * G))
        rv = np.empty(G)
        ctx.d2h(rv, d_mv.ptr + 8 * G)
        sel = None if ntop is None else P.select_genes(rv, ntop)
        K = G if sel is None else len(sel)
        d_sel = DeviceArray.from_host(ctx, sel) if sel is not None else None
        nw = int(ctx.lib.dsq_sample_gram_work_doubles(N, K))
        d_w, d_S, d_D = DeviceArray(ctx, nw, np.float64), DeviceArray(ctx, N * N, np.float64), DeviceArray(ctx, N * N, np.float64)
        r["K"], r["work_mb"] = K, nw * 8 / 2 ** 20
        r["sample_gram_ms"] = timed(ctx, a.reps, "dsq_dev_sample_gram", _vp(d_x.ptr), SAMPLE_MAJOR, N, G, G,
                                    _vp(d_sel.ptr) if d_sel is not None else None, K, _vp(d_mv.ptr), _vp(d_w.ptr), _vp(d_S.ptr), N)
        r["gram_dist_ms"] = timed(ctx, a.reps, "dsq_dev_gram_dist", _vp(d_S.ptr), N, N, _vp(d_D.ptr), N)
        flop = 2.0 * K * N * (N + 1) / 2
        r["gram_tflops_of_entry"] = flop / (r["sample_gram_ms"]["median"] * 1e-3) / 1e12
        r["pack_bytes_mb"] = 8.0 * K * (N + ((N + 15) // 16 * 16)) / 2 ** 20  # read x once, write the panel once
        for d in (d_x, d_mv, d_sel, d_w, d_S, d_D):
            if d is not None:
                d.free()
        # end to end from the host matrix, and what a user does today
        t0 = time.perf_counter()
        if ntop is None:
            D = P.sample_distances(ctx, x)
        else:
            res = P.pca(ctx, x, ntop=ntop)
        r["end_to_end_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        v = x.var(0, ddof=1)
        xs = x if ntop is None else x[:, np.argsort(-v, kind="stable")[:ntop]]
        xc = xs - xs.mean(0)
        Sn = xc @ xc.T
        if ntop is None:
            dg = np.diag(Sn)
            Dn = np.sqrt(np.maximum(dg[:, None] + dg[None, :] - 2 * Sn, 0))
            np.fill_diagonal(Dn, 0.0)
            r["numpy_s"] = time.perf_counter() - t0
            r["max_rel_diff"] = float(np.max(np.abs(D - Dn)) / Dn.max())
        else:
            from scipy.linalg import eigh

            t1 = time.perf_counter()
            w = eigh(Sn, eigvals_only=True)[::-1]
            r["numpy_s"], r["eigh_s"] = time.perf_counter() - t0, time.perf_counter() - t1
            r["max_rel_diff"] = float(np.max(np.abs(res.variance[:10] * (N - 1) - w[:10]) / w[0]))
        print(json.dumps(r), flush=True)
        out["shapes"].append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
