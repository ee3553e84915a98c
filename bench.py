"""bench.py — genes/sec of the end-to-end deseq2() hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4] [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and nothing else: it generates the matrix, uploads it, warms up, times
the K steps, writes the outputs if asked to and prints the result line.  `--full` adds every other measurement and
check, each of which takes runs of its own (listed under "Prints" below); the figures of those are null in a plain line.

A "step" is one pass of the whole path (size factors -> MoM -> mu_hat -> genewise alpha ->
trend/prior -> MAP alpha -> IRLS LFC -> Cook's (+ refit) -> Wald) over one synthetic count
matrix that is already resident in HBM when the timed region starts (the upload and the
one-off int64 -> int32 gene-major transposition happen in DeseqPipeline.__init__, outside
it; the per-gene result vectors ARE copied back to the host inside it).

Multi-GPU (driver launches `python -m torch.distributed.run --nproc-per-node N bench.py
--gpus N ...`; by hand `python bench.py --gpus N` starts the N ranks itself): genes shard across ranks.
Default for N > 1 is `--scaling strong`: the NAMED configuration's genes are split over the ranks
(BASELINE configs[2]: "60k x 1k, 1 vs 8 MI355X gene-shard"; configs[4]: c5 = 60k x 5k over 8 GPUs - every
rank generates only its own gene shard and sample block, pydeseq2_amd.synth.synth_counts_block);
`--scaling weak`: every rank owns the configuration's gene count.  The two cross-gene steps are exchanged in
DistDeseqPipeline over RCCL (size-factor medians, trend/prior on all-gathered per-gene vectors).
The harness itself is torch-free: the RCCL unique id travels over a TCP socket
(pydeseq2_amd.distributed.exchange_unique_id), barriers and the max-over-ranks are RCCL all-gathers.

Prints ONE JSON line on rank 0: metric, value (genes/s), unit, higher_is_better, dtype, ms_per_step, the workload, and
  roofline     — dominant kernel (dispersion MLE/MAP, k_alpha): algorithmic bytes per launch
                 (12*N bytes per gene: int32 counts + fp64 mu_hat) / mean launch
                 duration measured with HIP events on the launch stream IN THE TIMED STEPS, vs 8 TB/s HBM peak
With `--full` also (options --no-cpu-baseline, --no-extras and --cpu-sample narrow it):
  kernel_ms_per_step, stage_wall_ms_profiled_step, collective_ms_per_step, evaluations per gene —
                 one more, untimed step that synchronises and reads HIP events after every stage
  cpu_baseline — the oracle (numpy/scipy restatement of the reference, joblib over host cores)
                 timed on a bounded gene sample of the same workload.
  parity       — the engine re-run on exactly the gene slice the oracle just computed, compared in-run
                 (north-star tolerance 1e-5 on LFC / dispersions / p-values); the speed-up is only
                 reported when it holds.
  h2d_ms / value_with_h2d — the upload of the host count matrix (int64 as the reference holds it) and the
                 one-off transposition, and the rate that includes them (a pipeline is built and closed first, so that
                 the timed upload does not pay the one-off allocations).
  summary_tail, lfc_shrink, plugin_path, other_configs, parity_c4 — the summary tail, apeGLM shrinkage, the drop-in path
                 and the other BASELINE configurations (c2, c4, c5 and one GPU's share of c5) with their own parity objects.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (genes, samples, design)            BASELINE.json configs[1..3]
    "c2": (20000, 200, "2level"),
    "c3": (60000, 1000, "2level"),
    "c4": (60000, 500, "3factor"),
    "c4b": (60000, 500, "2factor"),  # developer measurements: p = 4, 6 cells (not a BASELINE configuration)
    "c5": (60000, 5000, "mixed"),  # BASELINE configs[4]; tiled generator (a rank builds only its shard; ~1 min at 1 GPU)
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
FP64_VALU_PEAK_TFLOPS = 78.6  # MI355X fp64 vector peak (256 CU x 128 flop/clk x 2.4 GHz)


def synth_fast(G, N, design, seed):
    """SURVEY §8(d) generator (pydeseq2_amd/synth.py)."""
    from pydeseq2_amd.synth import synth_counts

    return synth_counts(G, N, design, seed)


SEEDS = {"c2": 1, "c3": 2, "c4": 3, "c5": 4, "c4b": 5}


def plan_rank_data(config, genes, scaling, rank, world):
    """The matrix (block) one rank works on: (counts [N x G_rank] int64, X, sample block or None, G_rank, G_total,
    generator name).  strong: the configuration's genes split into contiguous blocks, one per rank, plus the rank's block
    of samples over all genes (size factors with two collectives); weak: every rank its own matrix of the
    configuration's size.  c5 (60 000 x 5 000) always comes from the tiled generator: a rank generates its gene shard
    and its sample block only, never the whole matrix."""
    from pydeseq2_amd.distributed import sample_block
    from pydeseq2_amd.synth import synth_counts_block

    G_cfg, N, design = CONFIGS[config]
    G_cfg = genes or G_cfg
    seed0 = SEEDS[config]
    tiled = config == "c5"
    if scaling == "strong" and world > 1:
        cuts = np.linspace(0, G_cfg, world + 1).astype(int)
        g0, g1 = int(cuts[rank]), int(cuts[rank + 1])
        n0, n1 = sample_block(rank, world, N)
        if tiled:
            counts, X = synth_counts_block(G_cfg, N, design, seed0, genes=(g0, g1))
            samp, _ = synth_counts_block(G_cfg, N, design, seed0, samples=(n0, n1))
        else:  # one matrix for the whole job (the single-GPU run's), every rank keeps its blocks
            counts_all, X = synth_fast(G_cfg, N, design, seed=seed0)
            counts = np.ascontiguousarray(counts_all[:, g0:g1])
            samp = np.ascontiguousarray(counts_all[n0:n1])
        return counts, X, samp, g1 - g0, G_cfg, "tiled" if tiled else "synth_counts"
    if tiled:
        counts, X = synth_counts_block(G_cfg, N, design, 1000 * rank + seed0)
    else:
        counts, X = synth_fast(G_cfg, N, design, seed=1000 * rank + seed0)
    return counts, X, None, G_cfg, G_cfg * world, "tiled" if tiled else "synth_counts"


def launch_local_ranks(n, argv, script=None):
    """`python bench.py --gpus N` started by hand: one child process per GPU with the environment a launcher would set
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT); returns the worst exit code.  (The driver starts the
    ranks itself through torch.distributed.run and never gets here.)"""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
        if rc:  # a rank died: the others would wait for it in the control plane forever
            for q in procs:
                if q.poll() is None:
                    q.terminate()
    return rc


def cpu_baseline(counts, X, n_sample, n_jobs):
    """Oracle deseq2()+Wald on the first n_sample genes, all host cores (kind = 'port')."""
    from oracle import nbglm_oracle as orc

    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        orc.deseq2(np.ascontiguousarray(counts[:, : 2 * n_jobs]), X, n_jobs=n_jobs, keep_layers=False)  # warm the pool
        sub = np.ascontiguousarray(counts[:, :n_sample])
        t = time.perf_counter()
        ref = orc.deseq2(sub, X, n_jobs=n_jobs, keep_layers=False)
        dt = time.perf_counter() - t
    return sub.shape[1] / dt, dt, sub, ref


# north-star tolerance 1e-5.  A p-value is a function of its Wald statistic z with d log p / d log z ~ z^2 in the
# tail (p = 2 sf(|z|)), so a 1e-5 agreement of the statistic is a 1e-5 * max(1, z^2) agreement of the p-value:
# the p-value error is reported in that unit ("pvalue_per_z2") and the statistic itself at 1e-5
PARITY_TOL = {"dispersions": 1e-5, "LFC": 1e-5, "lfcSE": 1e-5, "stat": 1e-5, "pvalue_per_z2": 1e-5}
# Genes whose L-BFGS-B success flag differs between the two sides.  Floor: a ONE-ULP change of mu_hat flips 0.09-0.18 % of
# the reference's own fits per fit (tests/tools/flip_floor.py -> profiles/r03_flip_floor.json; two fits per gene here);
# measured engine vs reference 0.14-0.23 % over both fits.
PARITY_MAX_NOISE_FRAC = 0.0035
# RAW Wald p-values (north-star wording), asserted as a COUNT of genes beyond a raw 1e-5 and as a ceiling on the worst one.
# Both bounds are the REFERENCE'S OWN noise floor, measured (tests/tools/pvalue_floor.py -> profiles/r06_pvalue_floor_*.json):
# the reference run twice, once with mu_hat moved by ONE ULP, disagrees with itself on the raw p-value of 0.23-0.32 % of the
# genes at c2 (46-64 of 20 000), 0-0.33 % at c3 (0-26 of 8000), 0-0.15 % at c5 (0-3 of 2000) beyond 1e-5, worst gene
# 0.8e-5 ... 6.6e-5: a success-flag flip (~7 per 20 000 fits) moves the all-gene trend by ~1e-6, every MAP dispersion by
# ~1e-8 ... 1e-6 and a p-value by that times z^2 / 2.  Engine vs reference, measured: 0.025 % (c3, all
# 60 000 genes), 0.12 % (c2, all 20 000), worst gene 3.7e-5 ... 1.8e-4.
PARITY_RAW_P_BEYOND_FRAC = 4.0e-3
PARITY_RAW_P_CEILING = 3.0e-4


def parity_report(res, ref):
    """Engine vs oracle on the same matrix: max relative errors over the genes on which both L-BFGS-B runs
    agree about convergence; the genes on which they disagree (line search decided inside rounding noise:
    one side returns its iterate, the other the quantised grid value) are counted and reported separately."""
    def rel(a, b, floor):
        a, b = np.asarray(a, float), np.asarray(b, float)
        both_nan = np.isnan(a) & np.isnan(b)
        d = np.abs(a - b) / np.maximum(np.abs(b), floor)
        d[both_nan] = 0.0
        d[np.isnan(d)] = np.inf  # NaN on one side only
        return d

    nz = ref.non_zero
    with np.errstate(invalid="ignore"):
        noisy = (res.genewise_converged != ref.genewise_converged) | (res.MAP_converged != ref.MAP_converged)
    noisy &= nz
    noisy |= res.refitted != ref.refitted
    ok = ~noisy
    errs = {
        "dispersions": rel(res.dispersions, ref.dispersions, 1e-300),
        "LFC": rel(res.LFC, ref.LFC, 1e-3).max(axis=1),  # |LFC| floor 1e-3 (natural log): absolute 1e-8
        "lfcSE": rel(res.lfcSE, ref.lfcSE, 1e-300),
        "stat": rel(res.stat, ref.stat, 1e-3),
        "pvalue_per_z2": rel(res.pvalue, ref.pvalue, 1e-300) / np.maximum(1.0, np.nan_to_num(ref.stat) ** 2),
    }
    max_rel = {k: float(v[ok].max()) if ok.any() else 0.0 for k, v in errs.items()}
    max_noise = {k: float(v[noisy].max()) if noisy.any() else 0.0 for k, v in errs.items()}
    # the RAW p-value error (north-star wording: "1e-5 on Wald p-values"), reported next to the asserted per-z^2 quantity so
    # that the reader sees what the relaxation covers: how many genes exceed a raw 1e-5 and how far out in the tail they sit
    p_raw = rel(res.pvalue, ref.pvalue, 1e-300)
    absz = np.abs(np.nan_to_num(np.asarray(ref.stat, float)))
    beyond = ok & (p_raw > 1e-5)
    # (the two raw bounds are asserted where the floor was measured - slices of 2000 genes and more - and on any slice without a
    # flag flip: ONE flip among G genes moves the all-gene trend, and with it every p-value, by ~2e-3 / G times z^2 / 2, which
    # on a 300-gene slice puts a tenth of the genes beyond a raw 1e-5)
    raw_asserted = bool(len(nz) >= 2000 or noisy.sum() == 0)
    pv_raw = {"pvalue": float(f"{(p_raw[ok].max() if ok.any() else 0.0):.3e}"),
              "n_genes_pvalue_beyond_1e-5": int(beyond.sum()),
              "abs_z_range_of_those_genes": [round(float(absz[beyond].min()), 2), round(float(absz[beyond].max()), 2)]
              if beyond.any() else None,
              "max_abs_z": round(float(absz[ok].max()), 2) if ok.any() else 0.0,
              "asserted": ({"n_genes_pvalue_beyond_1e-5_at_most": int(max(3, PARITY_RAW_P_BEYOND_FRAC * len(nz))),
                            "pvalue_at_most": PARITY_RAW_P_CEILING} if raw_asserted else
                           "not on this slice: fewer than 2000 genes with a flag flip among them (the flip moves the trend)")}
    untouched = nz & ~res.refitted & ~ref.refitted
    both = untouched & (((res.genewise_converged == 0) & (ref.genewise_converged == 0))
                        | ((res.MAP_converged == 0) & (ref.MAP_converged == 0)))
    G = len(nz)
    good = (all(max_rel[k] <= PARITY_TOL[k] for k in PARITY_TOL)
            and noisy.sum() <= max(2, PARITY_MAX_NOISE_FRAC * G)
            and (not raw_asserted
                 or (int(beyond.sum()) <= max(3, PARITY_RAW_P_BEYOND_FRAC * G) and pv_raw["pvalue"] <= PARITY_RAW_P_CEILING))
            and float(np.max(np.abs(res.size_factors - ref.size_factors) / ref.size_factors)) < 1e-12
            and bool((res.cooks_outlier[ok] == ref.cooks_outlier[ok]).all()))
    return {"genes": int(G), "tolerance": PARITY_TOL, "max_rel": {k: float(f"{v:.3e}") for k, v in max_rel.items()},
            "raw_pvalue": pv_raw,
            "n_noise_genes": int(noisy.sum()), "frac_noise": round(float(noisy.sum()) / G, 6),
            "max_rel_noise": {k: float(f"{v:.3e}") for k, v in max_noise.items()},
            "n_grid_on_both_sides": int(both.sum()),
            "size_factors_max_rel": float(f"{np.max(np.abs(res.size_factors - ref.size_factors) / ref.size_factors):.3e}"),
            "trend_coeffs_max_rel": (float(f"{np.max(np.abs(np.asarray(res.trend_coeffs) - ref.trend_coeffs) / np.abs(ref.trend_coeffs)):.3e}")
                                     if (res.trend_coeffs is not None and ref.trend_coeffs is not None) else None),
            "ok": bool(good)}


def _read_profile_json(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    try:
        return json.load(open(path))
    except Exception:  # noqa: BLE001
        return None


def stage_roofline(cfg, genes_full, N, full_ms):
    """Roofline object of ONE dispersion-stage launch group (main launch + continuation) of `cfg`:
      hbm        algorithmic bytes (12 N + 17 per gene) / the HIP-event stage time, vs 8 TB/s;
      traffic    HBM bytes of the same kernels from the FETCH_SIZE / WRITE_SIZE counter passes (profiles/traffic_<cfg>.json,
                 gfx950 x2 correction of the guide; rescaled per gene when the counters were collected at another size);
      companion  the fp64 vector-ALU bound from the MEASURED instruction mix (profiles/flops_<cfg>.json: SQ_INSTS_VALU_
                 {ADD,MUL,FMA,TRANS}_F64 of the stage's kernels, tools/pmc_flops.sh) / the same stage time, vs 78.6 TFLOP/s -
                 nothing assumed: flop = 64 x (ADD + MUL + 2 FMA + TRANS) wave instructions."""
    alg = genes_full * (12.0 * N + 17.0)
    ach = alg / (full_ms * 1e-3) / 1e9
    out = {"bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": None, "traffic_ratio": None,
           "algorithmic_bytes_per_launch": int(alg), "full_launch_ms": round(full_ms, 4), "companion": None}
    tj = _read_profile_json(f"traffic_{cfg}.json")
    if tj and tj.get("k_alpha_hbm_bytes_per_launch"):
        tr = float(tj["k_alpha_hbm_bytes_per_launch"])
        src = tj.get("source", "")
        if tj.get("genes_per_launch") and tj["genes_per_launch"] != genes_full:
            tr *= genes_full / tj["genes_per_launch"]
            src += f" - rescaled from a launch of {tj['genes_per_launch']} genes"
        out["traffic"], out["traffic_source"] = int(tr), src
        out["traffic_ratio"] = round(tr / alg, 3)
    fj = _read_profile_json(f"flops_{cfg}.json")
    if fj and fj.get("kernels") and fj.get("genes_per_launch"):
        ks = {k: v for k, v in fj["kernels"].items() if k.startswith("dsq::k_alpha")}
        if ks:
            scale = genes_full / float(fj["genes_per_launch"])
            flop = scale * sum(v["flop_per_launch"] for v in ks.values())
            valu = scale * sum(v["SQ_INSTS_VALU"] for v in ks.values())
            f64 = scale * sum(v["f64_wave_instructions"] for v in ks.values())
            tflops = flop / (full_ms * 1e-3) / 1e12
            # issue-side view: a wave64 fp64 instruction holds its SIMD for 4 cycles, any other VALU instruction for >= 1
            simd_cycles = 256 * 4 * 2.4e9 * full_ms * 1e-3
            out["companion"] = {
                "bound": "fp64_valu", "achieved": round(tflops, 2), "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(tflops / FP64_VALU_PEAK_TFLOPS, 4), "flop_per_launch": int(flop),
                "f64_wave_instructions": int(f64), "valu_wave_instructions": int(valu),
                "f64_issue_cycles_share": round(4.0 * f64 / simd_cycles, 4),
                "valu_issue_cycles_share_lower_bound": round((4.0 * f64 + (valu - f64)) / simd_cycles, 4),
                "kernels": sorted(ks), "source": f"profiles/flops_{cfg}.json ({fj.get('source', '')})",
                "note": "measured instruction mix (no assumed flop count): frac = 64 (ADD + MUL + 2 FMA + TRANS) / stage time / "
                        "peak; f64_issue_cycles_share = share of all SIMD cycles (256 CU x 4 SIMD x 2.4 GHz x stage time) "
                        "spent issuing fp64 instructions at 4 cycles each"}
    return out


def timed_steps(pipe, ctx, steps):
    """`steps` passes of the resident path, each timed twice: host wall clock around the call (it ends with the final
    synchronisation) and HIP events on the engine's stream around the same call - a host stall shows up in the first only,
    a device stall in both.  Returns (wall_ms list, gpu_ms list)."""
    wall, gpu = [], []
    for _ in range(steps):
        ctx.sync()
        ctx.timer_start()
        t0 = time.perf_counter()
        pipe.deseq2()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(float(ctx.timer_stop()))
    return wall, gpu


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(res, out_dir, G):
    """`--dump-outputs DIR`: the DeseqResult of the last timed step as DIR/<field>.npy (float64; flags as 0 / 1, scalars as
    0-d arrays), so that two builds can be compared output for output on the same seeded matrix.  Above 64 MB in all, a
    fixed seeded sample of the genes is written instead (DIR/gene_index.npy holds the sampled gene numbers)."""
    arrays = {}
    for name, v in vars(res).items():
        if isinstance(v, (dict, str)) or v is None:
            continue
        a = np.asarray(v)
        if a.dtype.kind not in "biuf":
            continue
        arrays[name] = np.array(a, dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        per_gene = sum(a.nbytes // G for a in arrays.values() if a.ndim and a.shape[0] == G) + 8  # (+ gene_index)
        fixed = total - (per_gene - 8) * G + 4096 * (len(arrays) + 1)  # (+ the .npy headers, with room to spare)
        keep = max(1, min(G, (DUMP_MAX_BYTES - fixed) // per_gene))
        idx = np.sort(np.random.default_rng(0).choice(G, size=keep, replace=False))
        arrays = {k: (a[idx] if a.ndim and a.shape[0] == G else a) for k, a in arrays.items()}
        arrays["gene_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    return sorted(arrays)


def _mmm(v):
    v = np.asarray(v, float)
    return {"min": round(float(v.min()), 3), "median": round(float(np.median(v)), 3), "max": round(float(v.max()), 3)}


def measure_other_config(name, genes, ctx, steps, warmup, parity_genes, n_jobs, shrink=True):
    """One more configuration on the same device (extras of the default run, so that the driver's record carries every
    BASELINE configuration, not only the headline one): ms per step of the resident path (MEDIAN of `steps` individually
    timed passes after `warmup` untimed ones, with min / max and the per-pass GPU time from HIP events beside the wall
    clock), the dispersion stage's launch time and HBM-roofline fraction (HIP events, as for the main line), the per-stage
    wall times of one profiled pass, and an in-run parity object against the oracle on a slice of the same matrix."""
    import warnings

    import pydeseq2_amd
    from oracle import nbglm_oracle as orc
    from pydeseq2_amd.synth import synth_counts_block

    G_cfg, N, design = CONFIGS[name]
    G = genes or G_cfg
    t_gen = time.perf_counter()
    if name == "c5":
        counts, X = synth_counts_block(G, N, design, SEEDS[name])
    else:
        counts, X = synth_fast(G, N, design, seed=SEEDS[name])
    t_gen = time.perf_counter() - t_gen
    pipe = pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx)
    for _ in range(warmup + 1):
        pipe.deseq2()
    pipe.kernel_log = {}
    ctx.sync()
    forks0 = pipe.lfc_forks
    t0 = time.perf_counter()
    wall, gpu = timed_steps(pipe, ctx, steps)
    loop_ms = (time.perf_counter() - t0) * 1e3 / steps
    lfc_forked = pipe.lfc_forks > forks0
    dt = float(np.median(wall)) * 1e-3
    big = [(ms, g) for ms, g in pipe.kernel_log.get("k_alpha", []) if g > 0.5 * G]
    full_ms = float(np.median([ms for ms, _ in big])) if big else None
    alg = G * (12.0 * N + 17.0)
    genes_full = float(np.median([g for _, g in big])) if big else float(G)
    out = {"workload": f"{name}: {G} genes x {N} samples, design {design} (p={X.shape[1]})"
                       + (" - one of eight GPUs' share of BASELINE configs[4]" if (name == "c5" and G < G_cfg) else ""),
           "ms_per_step": round(dt * 1e3, 3), "genes_per_s": round(G / dt, 1),
           "steps": steps, "warmup": warmup, "ms_per_step_wall": _mmm(wall), "ms_per_step_gpu_events": _mmm(gpu),
           "ms_per_step_loop_mean": round(loop_ms, 3),
           "timing_note": "ms_per_step = median wall time of the individually timed passes; gpu_events = HIP events on the "
                          "engine's stream around the same passes (a host stall widens wall only)",
           "generator_s": round(t_gen, 2),
           "lfc_fit_in_two_launches": bool(lfc_forked),
           "lfc_note": ("the LFC fit of the genes whose MAP dispersion is final starts under the MAP stage's tail (DESIGN 5): the "
                        "MAP launch's continuation shares the device with it, so full_launch_ms of that stage is 4-6 % longer "
                        "than alone (DSQ_LFC_OVERLAP=0) while the step is shorter") if lfc_forked else None,
           "dispersion_stage": None if full_ms is None else {
               "full_launch_ms": round(full_ms, 4), "algorithmic_bytes_per_launch": int(alg),
               "achieved_GBps": round(alg / (full_ms * 1e-3) / 1e9, 2),
               "frac": round(alg / (full_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)},
           "roofline": None if full_ms is None else stage_roofline(name, genes_full, N, full_ms)}
    try:
        rp = pipe.deseq2(profile=True)
        out["stage_wall_ms_profiled_step"] = {k: round(v * 1e3, 3) for k, v in rp.timings.items()}
    except Exception as e:  # noqa: BLE001
        out["stage_wall_error"] = repr(e)
    if shrink:
        try:  # apeGLM MAP LFC of the last coefficient, all genes (DeseqStats.lfc_shrink; not part of ms_per_step)
            from pydeseq2_amd.summary import lfc_shrink

            res = pipe.deseq2()
            lfc_shrink(pipe, res, X.shape[1] - 1)
            ctx.sync()
            t0 = time.perf_counter()
            shr = lfc_shrink(pipe, res, X.shape[1] - 1)
            ctx.sync()
            out["lfc_shrink"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3),
                                 "converged_fraction": round(float(np.nanmean(shr[2])), 6)}
        except Exception as e:  # noqa: BLE001
            out["lfc_shrink_error"] = repr(e)
    if parity_genes:
        try:
            whole = parity_genes >= G
            t_cpu = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sub = counts if whole else np.ascontiguousarray(counts[:, :parity_genes])
                ref = orc.deseq2(sub, X, n_jobs=n_jobs, keep_layers=False)
            t_cpu = time.perf_counter() - t_cpu
            if whole:  # the BENCHED pipeline's own result, every gene
                out["parity"] = parity_report(pipe.deseq2(), ref)
                out["parity"]["slice"] = f"all {G} genes of the benched matrix, the benched pipeline's own result"
            else:
                psub = pydeseq2_amd.DeseqPipeline(sub, X, ctx=ctx)
                out["parity"] = parity_report(psub.deseq2(), ref)
                out["parity"]["slice"] = f"first {parity_genes} genes of the benched matrix (a pipeline of their own: the trend is a fit over the genes it is given)"
                psub.close()
            out["parity"]["oracle_s"] = round(t_cpu, 1)
            out["parity"]["oracle_genes_per_s"] = round(sub.shape[1] / t_cpu, 1)
        except Exception as e:  # noqa: BLE001
            out["parity_error"] = repr(e)
    pipe.close()
    return out


def measure_plugin_path(counts, X, ctx, res, with_shrink=True):
    """The DROP-IN path: the eight `Inference` methods as the reference's DeseqDataSet.deseq2() / DeseqStats call them
    (dds.py:747-785, 901-911, 953-960, 1150-1157, 1240; ds.py:338-350, 400) - host numpy arrays in, host numpy arrays
    out, every call handed FRESH copies of the count / mu matrices as `self.X[:, self.non_zero_idx]` makes them.  Timed
    per call; `total_ms` = their sum in dds.py call order (the copies the reference itself makes are outside the timers).
    Two passes: `first` (nothing cached) and `repeat` (the second deseq2() on the same data)."""
    from pydeseq2_amd import HipInference

    inf = HipInference(ctx=ctx)
    nz = np.asarray(res.non_zero, bool)
    nzi = np.nonzero(nz)[0]
    N, G = counts.shape
    sf = np.asarray(res.size_factors, float)
    min_mu, min_disp, max_disp, beta_tol = 0.5, 1e-8, float(max(10.0, N)), 1e-8
    linear = len({tuple(r) for r in np.asarray(X)}) == X.shape[1]  # dds.py:747-750
    normed_layer = counts / sf[:, None]

    def one_pass():
        T = {}

        def tm(name, fn):
            t0 = time.perf_counter()
            o = fn()
            T[name] = T.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return o

        normed = normed_layer[:, nzi]  # dds.py:1149
        rde = tm("fit_rough_dispersions", lambda: inf.fit_rough_dispersions(normed, X))
        mde = tm("fit_moments_dispersions", lambda: inf.fit_moments_dispersions(normed, sf))
        mom = np.clip(np.minimum(rde, mde), min_disp, max_disp)
        y = counts[:, nzi]  # (the reference's own copy, `self.X[:, self.non_zero_idx]`: outside the timers, as all of them)
        if linear:
            mu_hat = tm("lin_reg_mu", lambda: inf.lin_reg_mu(y, sf, X, min_mu))
        else:
            mu_hat = tm("irls(mu_hat)", lambda: inf.irls(y, sf, X, mom, min_mu, beta_tol)[1])
        layer = np.full((N, G), np.nan)  # dds.py:770-771
        layer[:, nz] = mu_hat
        del mu_hat
        y, m = counts[:, nzi], layer[:, nzi]
        gw, _ = tm("alpha_mle(genewise)", lambda: inf.alpha_mle(y, X, m, mom, min_disp, max_disp))
        gw = np.clip(gw, min_disp, max_disp)
        # dds.py:1234-1262: the trend's outer loop (a GLM fit per pass, genes far off the curve dropped in between)
        cov, tgt = 1.0 / normed.mean(0), gw.copy()
        old_c, cf, n_trend = np.array([0.1, 0.1]), np.array([1.0, 1.0]), 0
        while (cf > 1e-10).all() and (np.log(np.abs(cf / old_c)) ** 2).sum() >= 1e-6 and n_trend < 20:
            old_c = cf
            cf, pred, okc = tm("dispersion_trend_gamma_glm", lambda: inf.dispersion_trend_gamma_glm(cov, tgt))
            n_trend += 1
            if not okc or (cf <= 1e-10).any():
                break
            ratio = tgt / pred
            keep = ~((ratio < 1e-4) | (ratio >= 15))
            cov, tgt = cov[keep], tgt[keep]
        T["trend_passes"] = n_trend
        fitted = np.asarray(res.fitted_dispersions, float)[nz]
        y, m = counts[:, nzi], layer[:, nzi]
        mp, _ = tm("alpha_mle(MAP)", lambda: inf.alpha_mle(y, X, m, fitted, min_disp, max_disp,
                                                          float(res.prior_disp_var), True, True))
        disp = np.asarray(res.dispersions, float)[nz]
        y = counts[:, nzi]
        beta, mu, hat, _ = tm("irls(LFC)", lambda: inf.irls(y, sf, X, disp, min_mu, beta_tol))
        mu_layer = np.full((N, G), np.nan)  # dds.py:972-974
        mu_layer[:, nz] = mu
        del mu, hat
        contrast = np.zeros(X.shape[1])
        contrast[-1] = 1.0
        m = mu_layer[:, nzi]
        tm("wald_test", lambda: inf.wald_test(X, disp, beta, m, np.diag(np.repeat(1e-6, X.shape[1])), contrast, 0.0))
        T["total_ms"] = float(sum(v for k, v in T.items() if k != "trend_passes"))
        if with_shrink:  # not part of deseq2() (ds.py:400); the eighth method, reported beside the total
            y = counts[:, nzi]
            tm("lfc_shrink_nbinom_glm", lambda: inf.lfc_shrink_nbinom_glm(X, y, 1.0 / disp, np.log(sf), 15.0, 1.0, "L-BFGS-B",
                                                                          X.shape[1] - 1))
        return {k: round(v, 3) for k, v in T.items()}

    first = one_pass()    # nothing cached, output layers pageable (staged, multi-threaded copy-out: csrc pc_download_rows)
    second = one_pass()   # device cache warm, output layers still pageable
    third = one_pass()    # this fit page-locks the three N x G output buffers (HipInference._layer)
    repeat = one_pass()   # steady state
    out = {"workload": f"{G} genes x {N} samples, p={X.shape[1]}: HipInference methods on host arrays in dds.py / ds.py call "
                       "order, fresh host copies per call", "first": first, "second": second, "third": third, "repeat": repeat,
           "total_ms": repeat["total_ms"], "total_ms_first": first["total_ms"], "total_ms_second": second["total_ms"],
           "total_ms_third": third["total_ms"],
           "note": "first: the only fit of a data set (uploads, pageable outputs); second: a caller that comes back (device "
                   "cache warm, outputs still pageable); third: the output layers are page-locked now (3 x hipHostMalloc of "
                   "N x G x 8 B, ~80 ms each at c3); repeat: every fit after that.  Floor of `repeat` at c3: 1.44 GB of N x G "
                   "outputs over PCIe (26 ms) + ten digests of 480 MB matrices at the host's memory bandwidth (2.4 ms each) + "
                   "the kernels (8 ms)"}
    stats = getattr(inf, "cache_stats", None)
    if stats is not None:
        out["cache"] = stats()
    return out


class _TimedComm:
    """Wraps a communicator for the profiled step: HIP-event time of every collective on the engine's stream."""

    def __init__(self, comm, ctx, log):
        self.comm, self.ctx, self.log = comm, ctx, log
        self.rank, self.world = comm.rank, comm.world

    def _timed(self, name, fn, *a):
        self.ctx.timer_start()
        out = fn(*a)
        self.log.append((name, self.ctx.timer_stop()))
        return out

    def allreduce_sum(self, darr):
        return self._timed("allreduce", self.comm.allreduce_sum, darr)

    def allgather(self, dsend, drecv):
        return self._timed("allgather", self.comm.allgather, dsend, drecv)


def main():
    # A run that hangs (a rendezvous, a device queue) must end with the Python stacks of all threads on stderr and a non-zero
    # exit code, not sit until the caller's limit: DSQ_BENCH_WATCHDOG_S seconds (default 40 min; a --full run takes about
    # two minutes, the largest configuration on one GPU a few minutes with its generator; 0 disables).
    import faulthandler

    wd = float(os.environ.get("DSQ_BENCH_WATCHDOG_S", "2400"))
    if wd > 0:
        faulthandler.dump_traceback_later(wd, exit=True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--genes", type=int, default=0, help="override the config's gene count")
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"],
                    help="strong (default for --gpus > 1): the configuration's genes are split over the ranks; "
                         "weak: every rank owns the configuration's gene count")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure: upload time, a profiled step, "
                         "CPU baseline and parity, summary tail, shrinkage, drop-in path, the other configurations")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity check")
    ap.add_argument("--cpu-sample", type=int, default=0, help="with --full: genes of the CPU baseline's sample")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the summary-tail / shrinkage / drop-in / other-configuration extras")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the result of the last timed step as DIR/<field>.npy (float64; per-rank DIR/rank<r>/ "
                         "when --gpus > 1)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:  # a plain run: nothing beside the headline figure
        args.no_cpu_baseline = args.no_extras = True

    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(launch_local_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.scaling is None:
        args.scaling = "strong"  # (one GPU: the named configuration, whole - the N = 1 point of the strong-scaling curve)
    N, design = CONFIGS[args.config][1:]
    counts, X, samp, G, G_total, generator = plan_rank_data(args.config, args.genes, args.scaling, rank, world)

    import pydeseq2_amd
    from pydeseq2_amd._lib import Context
    from pydeseq2_amd.distributed import DistDeseqPipeline, TcpControl, bring_up_comm

    # control plane of this harness (unique-id broadcast, barriers, max-over-ranks): a TCP star on rank 0;
    # the data-path collectives are RCCL calls the product makes through its C ABI
    control = TcpControl(rank, world, os.environ.get("MASTER_ADDR", "127.0.0.1"),
                         int(os.environ.get("MASTER_PORT", "29500")))
    # (DSQ_BENCH_SHARE_GPU=1: every rank on device 0 - exercises the multi-process path on a one-GPU box; RCCL refuses
    # two ranks on one device, so the job then runs on the host-staged fallback transport)
    ctx = Context(0 if os.environ.get("DSQ_BENCH_SHARE_GPU") else local_rank)
    info = ctx.device_info()
    transport = None
    comm = None
    if world > 1 or os.environ.get("DSQ_FORCE_DIST"):
        comm, transport = bring_up_comm(ctx, control)
        if transport != "rccl":
            print(f"[bench] rank {rank}: {transport}", file=sys.stderr)

    def make_pipe():
        if comm is not None:
            return DistDeseqPipeline(counts, X, comm=comm, ctx=ctx, keep_cooks=True, sample_shard=samp)
        return pydeseq2_amd.DeseqPipeline(counts, X, ctx=ctx, keep_cooks=True)

    def barrier():
        ctx.sync()  # hipStreamSynchronize on the engine's stream (it owns all device work)
        control.barrier()
        ctx.sync()

    # ---- upload (host int64 N x G -> HBM, narrowed to int32, + gene-major transposition): with --full timed on its own
    if args.full:
        make_pipe().close()  # first construction pays one-off allocations (pinned staging buffers, code objects)
    barrier()
    t_up = time.perf_counter()
    pipe = make_pipe()
    ctx.sync()
    h2d_s = control.max_float(time.perf_counter() - t_up) if args.full else None

    # the very first pass (kernel code objects, pool allocations) and a pass without the previous pass's non-zero mask
    # (what a single deseq2() call on a fresh pipeline pays: the host waits for the mask before it can compact)
    t_c = time.perf_counter()
    res = pipe.deseq2()
    ctx.sync()
    cold_first_ms = (time.perf_counter() - t_c) * 1e3
    pipe._nz_pred = None
    t_c = time.perf_counter()
    res = pipe.deseq2()
    ctx.sync()
    first_call_ms = (time.perf_counter() - t_c) * 1e3
    # the W warm-up steps of the steady-state path (the two passes above measure first-call latencies and are not counted:
    # with W = 2 they used to be the whole warm-up, and the first timed steps still ran 4 % slower than the rest; a plain
    # run keeps them too: they load the code objects and fill the pools, so the timed steps start from the same state)
    for _ in range(max(args.warmup, 0)):
        res = pipe.deseq2()
    # The timed region runs the production path (no per-stage synchronisation).  The dispersion
    # kernel's launch durations are still measured live in it: HIP events recorded on the engine's
    # stream around every k_alpha launch, read after the synchronisation the launch ends with anyway.
    pipe.time_kernels = False
    pipe.kernel_log = {}

    class _CountingComm:  # (collectives of the TIMED steps themselves, not only of the profiled one)
        def __init__(self, inner):
            self.inner, self.rank, self.world, self.n = inner, inner.rank, inner.world, 0

        def allreduce_sum(self, darr):
            self.n += 1
            return self.inner.allreduce_sum(darr)

        def allgather(self, dsend, drecv):
            self.n += 1
            return self.inner.allgather(dsend, drecv)

    counting = _CountingComm(comm) if comm is not None else None
    if counting is not None:
        pipe.comm = counting
    barrier()
    syncs0 = int(ctx.lib.dsq_host_sync_count())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = pipe.deseq2()
    ctx.sync()
    dt = control.max_float(time.perf_counter() - t0)
    host_syncs_per_step = (int(ctx.lib.dsq_host_sync_count()) - syncs0 - 1) / max(args.steps, 1)
    barrier()
    dumped = None
    if args.dump_outputs:  # (before the profiled step below runs the path once more)
        dump_dir = args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, f"rank{rank}")
        dumped = {"dir": os.path.abspath(dump_dir), "arrays": dump_outputs(res, dump_dir, G)}
    if counting is not None:
        pipe.comm = comm
    klog_timed = pipe.kernel_log
    # --full: one extra, untimed step with per-stage event timing (synchronises after every stage)
    coll_log, klog_prof, res_prof = [], {}, None
    if args.full:
        if comm is not None:
            pipe.comm = _TimedComm(comm, ctx, coll_log)
        pipe.time_kernels, pipe.collect_nfev, pipe.kernel_log = True, True, {}
        res_prof = pipe.deseq2(profile=True)
        klog_prof, pipe.time_kernels, pipe.collect_nfev = pipe.kernel_log, False, False
        if comm is not None:
            pipe.comm = comm
    # extras outside `value` (a failure here must not cost the bench line): summary tail (SURVEY 8(f)-1:
    # Cook's filter, independent filtering + BH) and apeGLM LFC shrinkage of the tested coefficient (8(f)-2)
    extras = {}
    if not args.no_extras:
        try:
            from pydeseq2_amd.summary import lfc_shrink
            from pydeseq2_amd.summary import summary as summary_tail

            cvec = np.zeros(X.shape[1])
            cvec[-1] = 1.0
            summary_tail(res_prof, cvec, ctx=ctx)
            ctx.sync()
            t_sum = time.perf_counter()
            for _ in range(3):
                sres = summary_tail(res_prof, cvec, ctx=ctx)
            ctx.sync()
            t_sum = (time.perf_counter() - t_sum) / 3
            extras["summary_tail"] = {"ms": round(t_sum * 1e3, 3),
                                      "rejections_at_0.05": int(np.nansum(sres["padj"] < 0.05)),
                                      "cutoff_index": int(sres["info"]["j"]),
                                      "note": "padj with independent filtering on the device (not part of value)"}
            lfc_shrink(pipe, res_prof, X.shape[1] - 1)
            ctx.sync()
            t_shr = time.perf_counter()
            shr = lfc_shrink(pipe, res_prof, X.shape[1] - 1)
            ctx.sync()
            t_shr = time.perf_counter() - t_shr
            extras["lfc_shrink"] = {"ms": round(t_shr * 1e3, 3), "prior_scale": round(float(shr[3]), 6),
                                    "converged_fraction": round(float(np.nanmean(shr[2])), 5),
                                    "note": "apeGLM MAP LFC of the last coefficient, all genes (not part of value)"}
        except Exception as e:  # noqa: BLE001
            extras["extras_error"] = repr(e)
        if world == 1 and not os.environ.get("DSQ_BENCH_NO_PLUGIN"):
            try:  # the drop-in path (HipInference under the reference's call sequence), host arrays in and out
                extras["plugin_path"] = measure_plugin_path(counts, X, ctx, res_prof)
            except Exception as e:  # noqa: BLE001
                extras["plugin_path_error"] = repr(e)
    barrier()

    if rank != 0:
        control.barrier()  # rank 0 finishes its CPU baseline before anybody tears the job down
        control.close()
        return

    ms_per_step = dt / args.steps * 1e3
    value = G_total / (dt / args.steps)

    # ---- roofline of the dominant kernel (both dispersion launches use k_alpha).  Algorithmic bytes, launch
    # duration and measured HBM traffic all refer to ONE FULL-SIZE launch (the two tiny launches on the genes
    # refitted after outlier replacement are listed separately, so that the rocprofv3 per-kernel average of the
    # same command, which mixes both, can still be reproduced from avg_launch_ms_all)
    klog = klog_timed
    launches = list(klog.get("k_alpha", []))
    stages = [nm for nm, _ in klog.get("k_alpha_stage", [])]
    big = [(ms, g) for ms, g in launches if g > 0.5 * G]
    # the genewise launches run alone; the MAP launches start while the robust-dispersion kernel of the side stream
    # is still finishing (it no longer waits behind the trend fit): both averages are reported, the roofline object
    # uses the one over ALL full-size launches, which is what rocprofv3's per-kernel average of this command shows
    solo = [ms for (ms, g), nm in zip(launches, stages) if g > 0.5 * G and nm == "alpha_mle"]
    maps = [ms for (ms, g), nm in zip(launches, stages) if g > 0.5 * G and nm == "alpha_map"]
    full_ms = float(np.mean([ms for ms, _ in big]))
    genes_full = float(np.mean([g for _, g in big]))
    alg_bytes = genes_full * (12.0 * N + 17.0)
    achieved = alg_bytes / (full_ms * 1e-3) / 1e9
    stage_ms = {k: round(float(np.sum([ms for ms, _ in v])), 3) for k, v in klog_prof.items()
                if k not in ("k_alpha", "k_alpha_stage", "grid_fallback_genes", "nfev")}
    # evaluations per gene of the full-size launches (counted by the kernel itself in the profiled step)
    nfev_full = [e for e, g in klog_prof.get("nfev", []) if g > 0.5 * G]
    evals = float(np.mean(nfev_full)) if nfev_full else None
    base_rf = stage_roofline(args.config, genes_full, N, full_ms)
    valu = base_rf["companion"]
    if valu is not None and evals:
        valu["evaluations_per_gene"] = round(evals / G, 2)
        valu["flop_per_sample_eval_measured"] = round(valu["flop_per_launch"] / (evals / G * genes_full * N), 1)
    n_fallback = float(np.sum([x for x, _ in klog.get("grid_fallback_genes", [])])) / args.steps
    roofline = {
        "bound": "hbm", "kernel": "dispersion MLE / MAP stage, full-size launches: k_alpha_rows (four genes per wavefront) "
                                  "+ k_alpha_wg (continuation of the parked fits) where the design takes them, else "
                                  "k_alpha (one gene per wavefront); HIP events around the stage's kernels",
        "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None, "traffic_ratio": None,
        "algorithmic_bytes_per_launch": int(alg_bytes), "full_launch_ms": round(full_ms, 4),
        "full_launches_timed": len(big),
        "full_launch_ms_genewise_only": round(float(np.mean(solo)), 4) if solo else None,
        "frac_genewise_only": round(alg_bytes / (float(np.mean(solo)) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if solo else None,
        "full_launch_ms_MAP_only": round(float(np.mean(maps)), 4) if maps else None,
        "overlap_note": "round 5: for the row-kernel designs (c2, c3) the MAP launch no longer starts beside the end of the "
                        "robust-dispersion kernel of the side stream (that kernel runs in two parts, under the tails of the "
                        "genewise and of the MAP stage), so genewise and MAP launches take the same time; for the other "
                        "designs the MAP launch still shares the machine with it - `achieved` / `frac` average over both, as "
                        "rocprofv3 does",
        "avg_launch_ms_all": round(float(np.mean([ms for ms, _ in launches])), 4), "launches_timed": len(launches),
        "pipeline_algorithmic_GBps": round(G * 104.0 * N / (dt / args.steps) / 1e9, 2),
        "kernel_ms_per_step": stage_ms if args.full else None, "grid_fallback_genes_per_step": n_fallback,
        "companion": valu,
    }
    for k in ("traffic", "traffic_source", "traffic_ratio"):
        if base_rf.get(k) is not None:
            roofline[k] = base_rf[k]

    # ---- CPU baseline + in-run parity.  For the headline configuration the oracle runs over EVERY gene of the benchmark
    # matrix (c3: 60 000 genes, ~40 s on the GPU box's 64 cores): its rate is the cpu_baseline, and the result the BENCHED
    # pipeline returned in the timed loop is compared with it gene by gene - no slice, no second pipeline.
    cpu, parity = None, None
    if not args.no_cpu_baseline:
        cores = os.cpu_count() or 1
        n_jobs = min(cores, 64)
        n_sample = args.cpu_sample or {"c2": 20000, "c3": 60000, "c4": 8000, "c4b": 8000, "c5": 2000}[args.config]
        n_sample = min(n_sample, G)
        try:
            v, secs, sub, ref = cpu_baseline(counts, X, n_sample, n_jobs)
            whole = n_sample >= G
            cpu = {"value": round(v, 1), "unit": "genes/s", "cores": n_jobs, "kind": "port",
                   "sample": f"oracle (numpy/scipy restatement of the reference incl. scipy L-BFGS-B per gene, "
                             f"joblib/loky workers warmed up) on "
                             + (f"ALL {G} genes" if whole else f"the first {n_sample} genes") + f" x {N} samples of the "
                             f"benchmark matrix, {secs:.1f} s",
                   "why_port": "the reference is a pure-Python package: under this build's rules it may be imported only in the "
                               "build container and may not travel to the GPU box in any form, so what runs here is the oracle - "
                               "bit-identical to the unmodified reference at the benchmark shapes (tests/golden/kat_e2e_*.npz, "
                               "made by the committed tests/golden/make_golden.py from the reference itself) and timed against "
                               "it on the same cores in the build container (reference_slice)"}
            ref_slice = os.path.join(ROOT, "profiles", "cpu_reference_slice.json")
            if os.path.exists(ref_slice):  # the unmodified reference kernels, timed on the build box (tools/)
                cpu["reference_slice"] = json.load(open(ref_slice)).get(args.config)
            if whole and world == 1:
                parity = parity_report(res, ref)
                parity["slice"] = f"all {G} genes of the benchmark matrix; engine side = the result of the timed steps themselves"
            else:
                psub = pydeseq2_amd.DeseqPipeline(sub, X, ctx=ctx)
                parity = parity_report(psub.deseq2(), ref)
                parity["slice"] = f"first {n_sample} genes of the benchmark matrix (the cpu_baseline sample)"
                psub.close()
            del ref, sub
            if not args.no_extras and args.config == "c3" and world == 1:
                # the other BASELINE configurations on the same device (configs[1], [3] at full size, configs[4] at full
                # size and as one GPU's share): each with its step time, the roofline object of its dispersion stage and an
                # in-run parity check ON THE BENCHED MATRIX - c2 over all its genes against the benched pipeline's own result,
                # c4 on its first 8000 genes, c5 on its first 2000 (the oracle takes ~1 ms per gene and core there)
                # (single-GPU runs only: in a multi-rank job the other ranks wait for rank 0 behind the control plane's
                # socket timeout, and the driver's N = 1 run records these)
                oc = {}
                for nm, gn, pg, st, wu in (("c2", 0, 20000, 20, 5), ("c4", 0, 8000, 20, 5), ("c5", 7500, 300, 20, 5),
                                           ("c5", 0, 2000, 8, 3)):
                    key = nm if gn == 0 else f"{nm}_shard"
                    if key == "c5" and os.environ.get("DSQ_BENCH_NO_C5_FULL"):
                        continue
                    try:
                        oc[key] = measure_other_config(nm, gn, ctx, st, wu, pg, n_jobs)
                    except Exception as e:  # noqa: BLE001
                        oc[key] = {"error": repr(e)}
                if oc:
                    extras["other_configs"] = oc
                    if "parity" in oc.get("c4", {}):
                        extras["parity_c4"] = oc["c4"]["parity"]
        except Exception as e:  # noqa: BLE001 - the GPU measurement above stands on its own
            print(f"[bench] cpu_baseline / parity failed: {e!r}", file=sys.stderr)
    parity_ok = bool(parity and parity["ok"]
                     and all(v.get("parity", {"ok": True})["ok"] for v in extras.get("other_configs", {}).values()))
    if parity is not None and not parity_ok:
        print("[bench] PARITY CHECK FAILED - no speed-up is reported", file=sys.stderr)

    coll_ms = round(float(sum(ms for _, ms in coll_log)), 3) if (comm is not None and args.full) else None
    rccl_nranks = None
    if transport == "rccl":
        try:
            rccl_nranks = comm.info()[0]  # what ncclCommCount says, not what the launcher's environment says
        except Exception as e:  # noqa: BLE001
            rccl_nranks = repr(e)
    out = {
        "metric": "genes/sec end-to-end deseq2() (size factors->dispersion->IRLS->Wald)",
        "value": round(value, 1), "unit": "genes/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic", "full": args.full,
        "genes_nonzero": int(genes_full),
        "config": {"workload": f"{args.config}: {G_total} genes x {N} samples in total"
                               + (f" ({G} per GPU, {args.scaling} scaling)" if world > 1 else "")
                               + f", design {design} (p={X.shape[1]}), NB counts (SURVEY 8d generator)",
                   "genes_per_gpu": G, "genes_total": G_total, "samples": N, "p": int(X.shape[1]),
                   "collectives": transport, "generator": generator,
                   "sample_block_rows": (None if samp is None else int(samp.shape[0])),
                   "rccl_nranks": rccl_nranks,
                   "device": info["name"] or f"{info['arch']} ({info['cu_count']} CUs)", "arch": info["arch"]},
        "first_call_ms": round(first_call_ms, 3), "cold_first_call_ms": round(cold_first_ms, 3),
        "first_call_note": "cold_first_call_ms: the very first deseq2() of the process on a fresh pipeline (code objects, "
                           "pool allocations; the non-zero mask and the row kernels' gene lists come from the upload); "
                           "first_call_ms: a pass that waits for the non-zero mask on the host before compacting (what "
                           "every first call did in round 2), pools warm",
        "h2d_ms": round(h2d_s * 1e3, 3) if args.full else None,
        "value_with_h2d": round(G_total / (dt / args.steps + h2d_s), 1) if args.full else None,
        "h2d_note": f"host int64 {N} x {G} ({counts.nbytes / 1e6:.0f} MB per GPU) -> int32 in HBM through pinned "
                    "staging chunks + gene-major transposition; value_with_h2d = genes / (one upload + one step)",
        "collective_ms_per_step": coll_ms,
        "collectives_per_step": (counting.n / max(args.steps, 1)) if counting is not None else None,
        "collectives_profiled_step": len(coll_log) if (comm is not None and args.full) else None,
        "host_syncs_per_step": round(host_syncs_per_step, 2),
        "roofline": roofline,
        "cpu_baseline": cpu,
        "parity": parity,
        "stage_wall_ms_profiled_step": {k: round(v * 1e3, 3) for k, v in res_prof.timings.items()} if args.full else None,
        "dumped_outputs": dumped,
        "speedup_vs_cpu_baseline": round(value / cpu["value"], 1) if (cpu and parity_ok) else None,
        "speedup_note": "value / cpu_baseline.value: GPU resident rate over the oracle ('port') on this box's host cores; the "
                        "oracle is bit-identical to the unmodified reference and runs at 0.77-1.18 x its speed on the same "
                        "cores (cpu_baseline.reference_slice, profiles/cpu_reference_slice.json; cpu_baseline.why_port)",
    }
    out.update(extras)
    print(json.dumps(out))
    control.barrier()
    control.close()


if __name__ == "__main__":
    main()
