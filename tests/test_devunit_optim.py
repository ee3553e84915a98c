"""The lane-parallel L-BFGS-B optimisers built for the device (tests/devunit/devunit_optim.hip): the wavefront-resident
inverse form of csrc/dsq_lbfgsb_wave.h, whose body only the device build has, and the compact form of csrc/dsq_lbfgsb.h
spread over 64 lanes (dsq_lbfgsb_par.h), whose read-barrier-write moves only a 64-lane policy compiles.

The converged coefficients of the shrinkage KATs cannot see a wrong but positive-definite quasi-Newton matrix, a pair
replayed from the wrong ring slot or a race that ends in refresh(): the minimum is the same, reached by other iterates.
These tests look at the iterates:
  1. the 8-, 16- and 32-lane group sums, exactly (a distinct power of two per lane) and within the bound of any order;
  2. lbfgsb_wave_direction on given pairs, exactly against fractions.Fraction and within a measured multiple of the error
     of a plain fp64 restatement against a 50-digit replay;
  3. lbfgsb_wave<P, R> against lbfgsb_nd<R, ., 10, OneLane> on the device, evaluation by evaluation, and its independence
     of the workspace's contents and of the wavefront it runs in;
  4. lbp::dpofa / dtrsl_upper / dtrsl_upper_t_own and the whole lbfgsb_nd with DeviceWave against OneLane, bit for bit.

The tests not marked `gpu` check the cases (tests/optim_cases.py)."""
import math

import numpy as np
import pytest

from tests import optim_cases as oc

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def du():
    from tests import devunit

    devunit.lib()
    return devunit


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_run(a, b):
    """every number of two traced runs has the same bits; else the first that differs"""
    for key in ("nev", "success", "nfev", "nit", "status"):
        if a[key] != b[key]:
            return f"{key}: {a[key]} != {b[key]}"
    for e in range(len(a["f"])):
        for key in ("x", "f", "g"):
            if not same_bits(a[key][e], b[key][e]):
                return f"evaluation {e}, {key}: {a[key][e]!r} != {b[key][e]!r}"
    for key in ("xfin", "ffin"):
        if not same_bits(a[key], b[key]):
            return f"{key}: {a[key]!r} != {b[key]!r}"
    return None


# ------------------------------------------------------------------------------------------------ 1. group sums
def test_groups_are_the_layouts_rows_and_columns():
    for R, (nrow, ncol) in {8: (8, 8), 16: (4, 16), 32: (2, 32)}.items():
        for lane in range(64):
            assert len(oc.group_members(R, "rowsum", lane)) == nrow and len(oc.group_members(R, "colsum", lane)) == ncol
            assert lane in oc.group_members(R, "rowsum", lane) and lane in oc.group_members(R, "colsum", lane)


@gpu
@pytest.mark.parametrize("which", ["rowsum", "colsum"])
@pytest.mark.parametrize("R", [8, 16, 32])
def test_group_sums_exactly(du, R, which):
    """A distinct power of two per lane.  64 of them do not fit 53 bits, so there are two passes: lanes 0 ... 31 carry
    2^lane and the others 0, then lanes 32 ... 63 carry 2^(lane - 32).  A lane left out of its group, counted twice or
    taken from another group changes the sum of the pass in which it is not 0, and every sum is an integer below 2^32:
    the result must have the bits of the sum over the group computed here."""
    lanes = np.arange(256) & 63
    rows = [np.where(lanes < 32, 2.0 ** (lanes & 31), 0.0), np.where(lanes >= 32, 2.0 ** (lanes & 31), 0.0)]
    for v in rows:
        v = v.copy()
        v[64:] = np.roll(v[64:], 5)  # (the other three wavefronts of the block hold other values)
        got = du.groupsum(R, which, v)
        for t in range(256):
            base = t & ~63
            ref = math.fsum(v[base + k] for k in oc.group_members(R, which, t & 63))
            assert bits(got[t]) == bits(ref), (R, which, t, got[t], ref)


@gpu
@pytest.mark.parametrize("which", ["rowsum", "colsum"])
@pytest.mark.parametrize("R", [8, 16, 32])
def test_group_sums_within_the_bound_of_any_order(du, R, which):
    """mixed signs, exponents over 40 binades, against math.fsum: (k - 1) u sum|v| for a group of k lanes"""
    v = oc.spread_doubles(np.random.default_rng(R + (which == "colsum")), 1024)
    got = du.groupsum(R, which, v)
    for t in range(v.size):
        grp = [v[(t & ~63) + k] for k in oc.group_members(R, which, t & 63)]
        ref = math.fsum(grp)
        assert abs(got[t] - ref) <= (len(grp) - 1) * oc.U * math.fsum(abs(x) for x in grp), (R, which, t, got[t], ref)


# ------------------------------------------------------------------------------------------------ 2. the direction
def exact_cases():
    rng = np.random.default_rng(21)
    return [oc.exact_direction_case(rng, R, p, col, head) for _, R, p in oc.DIR_SHAPES for col in oc.EXACT_COLS
            for head in oc.DIR_HEADS]


@pytest.fixture(scope="module")
def exact_refs():
    cases = exact_cases()
    return cases, [oc.direction_exact(c) for c in cases]  # (raises if a case leaves the exact numbers)


def rounding_cases():
    rng = np.random.default_rng(22)
    return [oc.random_direction_case(rng, R, p, 10, head) for _, R, p in oc.DIR_SHAPES for head in oc.DIR_HEADS]


def run_direction(du, cases):
    """the device's (d, z) per case, one launch per R"""
    out = [None] * len(cases)
    for R in (8, 16, 32):
        idx = [i for i, c in enumerate(cases) if c["R"] == R]
        sel = [cases[i] for i in idx]
        d, z = du.direction(R, [c["col"] for c in sel], [c["head"] for c in sel], [c["theta"] for c in sel],
                            [c["S"] for c in sel], [c["Y"] for c in sel], [c["RHO"] for c in sel], [c["g"] for c in sel],
                            [c["x"] for c in sel])
        for k, i in enumerate(idx):
            out[i] = (d[k], z[k])
    return out


def test_exact_direction_cases_are_exact(exact_refs):
    """every sum of the recurrence is exact in fp64 in any order (direction_exact's guard), so the plain fp64
    restatement gives the rational result; the cases cover every shape, the wrapping ring and NaN outside it"""
    cases, refs = exact_refs
    assert {(c["R"], c["p"]) for c in cases} == {(R, p) for _, R, p in oc.DIR_SHAPES}
    assert any(c["head"] + c["col"] > oc.M for c in cases)
    for c, (d, z) in zip(cases, refs):
        d64, z64 = oc.direction_fp64(c)
        assert np.array_equal(d, d64) and np.array_equal(z, z64)
        used = oc.ring(c["col"], c["head"])
        for slot in range(oc.M):
            assert np.isnan(c["S"][slot]).all() == (slot not in used) and np.isnan(c["RHO"][slot]) == (slot not in used)
            assert slot not in used or (c["S"][slot, c["p"]:] == 0).all() and (c["Y"][slot, c["p"]:] == 0).all()
    assert any(np.abs(z).max() > 0 for _, z in refs)


@gpu
def test_direction_exactly(du, exact_refs):
    """Small integers, theta and every rho a power of two, col <= 3: the device's d and z equal the recurrence in exact
    rationals (as numbers: a rational has no signed zero).  The slots outside the ring hold NaN, the padding components
    zero - a NaN in the output means a lane read what it must not."""
    cases, refs = exact_refs
    for c, (d, z), (dd, dz) in zip(cases, refs, run_direction(du, cases)):
        what = (c["R"], c["p"], c["col"], c["head"])
        assert not np.isnan(dd).any() and not np.isnan(dz).any(), what
        assert np.array_equal(dd, d) and np.array_equal(dz, z), (what, dd, d, dz, z)


@gpu
def test_direction_within_the_rounding_of_a_plain_restatement(du):
    """Random well-scaled pairs with y's > 0, col = 10 (heads 0, 3, 9: the ring wraps), against a 50-digit replay.  The
    bound is not fixed in advance: per case it is 8 x the error of the plain fp64 restatement of the recurrence
    (sequential sums, nothing fused) on the same inputs - the margin for the tree order of the lane sums and the fused
    multiply-adds - and at least 4 ulp of max|H| max|g|.

    Measured on an MI355X over the 30 cases: the fp64 restatement errs by 1.5e-16 ... 9.0e-16, the device by 1.4e-16 ...
    8.4e-16; ratio device / numpy 0.48 ... 3.24 (the largest at R = 32, p = 17); the device uses at most 0.40 of its bound."""
    cases = rounding_cases()
    worst = (0.0, None)
    for c, dev in zip(cases, run_direction(du, cases)):
        d, z, hmax = oc.direction_mp(c)
        e_np = oc.direction_error(oc.direction_fp64(c), (d, z))
        e_dev = oc.direction_error(dev, (d, z))
        floor = 4 * np.spacing(hmax * np.abs(c["g"]).max())
        bound = max(8 * e_np, floor)
        print(f"direction R={c['R']} p={c['p']} head={c['head']}: numpy {e_np:.3e} device {e_dev:.3e} "
              f"ratio {e_dev / e_np:.2f} floor {floor:.3e}")
        worst = max(worst, (e_dev / bound, (c["R"], c["p"], c["head"], e_dev, e_np, floor)))
        assert not np.isnan(dev[0]).any() and not np.isnan(dev[1]).any()
        assert np.array_equal(dev[0][c["p"]:], np.zeros(c["R"] - c["p"])) and \
            np.array_equal(dev[1][c["p"]:], np.zeros(c["R"] - c["p"]))
    assert worst[0] <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 3. wave vs compact
def settled(q, t0, ulps):
    return all((t["nit"], t["success"], t["status"]) == (t0["nit"], t0["success"], t0["status"])
               for t in (oc.host_trace(q, u) for u in ulps))


@pytest.fixture(scope="module")
def wave_host():
    """per problem of WAVE_PROBLEMS: (problem, host trace, E = the largest relative difference over the first five
    evaluations between the host run and itself with every gradient component moved by one ulp)"""
    out = []
    for entry in oc.WAVE_PROBLEMS:
        q = oc.wave_problem(entry)
        t0 = oc.host_trace(q)
        tp, tm = oc.host_trace(q, 1), oc.host_trace(q, -1)
        out.append((entry, q, t0, (tp, tm), max(oc.trace_distance(t0, tp), oc.trace_distance(t0, tm))))
    return out


def test_wave_problems_are_settled(wave_host):
    """The host run (compact form, one lane) of every problem keeps nit, flag and status when every gradient component
    moves by one ulp - and by 64; the list covers every shape, condition numbers 10 ... 10^4 and, per R, two problems of
    more than 12 iterations; no run needs more evaluations than the device trace holds."""
    for entry, q, t0, (tp, tm), E in wave_host:
        same = lambda t: (t["nit"], t["success"], t["status"]) == (t0["nit"], t0["success"], t0["status"])  # noqa: E731
        assert same(tp) and same(tm), entry
        assert settled(q, t0, (64, -64)), entry
        assert t0["success"] and t0["nfev"] <= 200, entry
        assert E > 0, entry
    assert {e[1] for e in oc.WAVE_PROBLEMS} == set(oc.DIR_SHAPES)
    assert {e[2] for e in oc.WAVE_PROBLEMS} == {10, 100, 1000, 10000}
    for R in (8, 16, 32):
        assert sum(t0["nit"] > 12 for entry, _, t0, _, _ in wave_host if entry[1][1] == R) >= 2


@gpu
@pytest.mark.parametrize("R", [8, 16, 32])
def test_wave_optimiser_follows_the_compact_form(du, wave_host, R):
    """lbfgsb_wave<P, R> against lbfgsb_nd<R, ., 10, OneLane>, both on the device on the same function bits: success,
    status and nit equal, the final x within 1e-7 max(1, |x|_inf), and the first five evaluations within 64 E (at least
    2^-40), E being what one ulp on the gradient does to the host run of the compact form: the inverse form rounds every
    entry of H, not one ulp of g.

    Measured on an MI355X over the 16 problems: E = 2.1e-15 ... 1.4e-12 (the largest at condition number 10^4), the
    device differs by 1.1e-15 ... 4.5e-13, at most 3.1 E and 0.026 of its bound; nit, nfev, flag and status equal on all."""
    for entry, q, t0, _, E in wave_host:
        P, R_, p = entry[1]
        if R_ != R:
            continue
        wave = du.optimise("wave", [q], P=P, R=R)[0]
        one = du.optimise("one", [q], R=R)[0]
        dist = oc.trace_distance(one, wave)
        bound = max(64 * E, 2.0 ** -40)
        print(f"wave {entry}: nit {wave['nit']} / {one['nit']} (host {t0['nit']}), nfev {wave['nfev']} / {one['nfev']}, "
              f"E {E:.3e}, device {dist:.3e}, bound {bound:.3e}")
        assert wave["nev"] == wave["nfev"] <= du.TRACE_CAP and one["nev"] == one["nfev"] <= du.TRACE_CAP, entry
        assert (wave["success"], wave["status"], wave["nit"]) == (one["success"], one["status"], one["nit"]), \
            (entry, wave["success"], wave["status"], wave["nit"], one["success"], one["status"], one["nit"])
        assert np.max(np.abs(wave["xfin"] - one["xfin"])) <= 1e-7 * max(1.0, np.max(np.abs(one["xfin"]))), entry
        assert same_bits(wave["x"][0], one["x"][0]) and same_bits(wave["f"][0], one["f"][0]), entry  # same function bits
        assert dist <= bound, (entry, dist, bound)


WAVE_INSTANCES = sorted({(P, R) for P, R, _ in oc.DIR_SHAPES})


@gpu
def test_wave_trace_does_not_depend_on_the_workspace(du):
    """zeros, NaN or 0xFF bytes in every word of the workspace before x0 goes in: the same bits of every evaluation"""
    for entry in oc.WAVE_PROBLEMS:
        P, R, p = entry[1]
        q = oc.wave_problem(entry)
        ref = du.optimise("wave", [q], P=P, R=R, pattern=du.ZERO_WORD)[0]
        assert ref["nit"] > 0
        for pattern in (du.NAN_WORD, du.FF_WORD):
            diff = same_run(ref, du.optimise("wave", [q], P=P, R=R, pattern=pattern)[0])
            assert diff is None, (entry, hex(pattern), diff)


@gpu
@pytest.mark.parametrize("P,R", WAVE_INSTANCES)
def test_wave_trace_does_not_depend_on_the_wavefront(du, P, R):
    """four problems in the four wavefronts of one 256-thread block against each alone in a 64-thread block"""
    p = P if P < R else R - 3
    qs = [oc.make_problem(seed, p, 100) for seed in (11, 12, 13, 14)]
    together = du.optimise("wave", qs, P=P, R=R, block=256)
    for q, t in zip(qs, together):
        alone = du.optimise("wave", [q], P=P, R=R, block=64)[0]
        assert alone["nit"] > 5
        diff = same_run(alone, t)
        assert diff is None, (P, R, q["seed"], diff)


# ------------------------------------------------------------------------------------------------ 4. 64 lanes vs one
def lbp_arrays(rng, lda, n, pivot=None):
    """an SPD matrix in the upper triangle of an lda x lda array (A(i, j) = a[j - 1][i - 1]), everything else random; pivot
    k: A(k, k) lowered so that the k-th pivot of the factorisation is <= 0 (k = 1: exactly 0; else by 1e-6 or 0.5, far
    beyond the rounding of the sum of squares it is compared with)"""
    B = rng.normal(size=(n + 2, n))
    A = B.T @ B / n + np.eye(n)
    if pivot is not None:
        Rf = np.linalg.cholesky(A).T
        A[pivot - 1, pivot - 1] = (Rf[:pivot - 1, pivot - 1] ** 2).sum() - (0.0 if pivot == 1 else (1e-6, 0.5)[pivot % 2])
    a = rng.normal(size=(lda, lda))
    for j in range(n):
        a[j, :j + 1] = A[:j + 1, j]
    return a, A


LBP_SHAPES = [(20, n) for n in range(1, 21)] + [(10, n) for n in range(1, 11)]


@gpu
def test_lbp_dpofa_64_lanes_equal_one(du):
    """random SPD matrices for n = 1 ... 20 (lda 20) and 1 ... 10 (lda 10), and matrices whose first, a middle or last
    pivot is not positive: the same return value in every lane and the same bits of the whole array - the strict lower
    triangle, which stays as it was, and sacc included"""
    rng = np.random.default_rng(41)
    for lda in (20, 10):
        ns, arrs, mats, want = [], [], [], []
        for _, n in [s for s in LBP_SHAPES if s[0] == lda]:
            for pivot in [None] + sorted({1, (n + 1) // 2, n}):
                a, A = lbp_arrays(rng, lda, n, pivot)
                ns.append(n); arrs.append(a); mats.append(A); want.append(pivot or 0)
        one = du.lbp(False, "dpofa", lda, ns, arrs)
        lanes = du.lbp(True, "dpofa", lda, ns, arrs)
        for k, (n, a0, A) in enumerate(zip(ns, arrs, mats)):
            assert (one[3][k] == want[k]).all() and (lanes[3][k] == want[k]).all(), (lda, n, want[k], one[3][k], lanes[3][k])
            for o, l in zip(one[:3], lanes[:3]):
                assert same_bits(o[k], l[k]), (lda, n, want[k])
            low = np.triu(np.ones((lda, lda), bool), 1)  # a[j][i] with i > j: A(i, j) below the diagonal
            assert same_bits(lanes[0][k][low], a0[low]) and same_bits(lanes[0][k][n:], a0[n:])
            if want[k] == 0:  # and it is the factor: |R'R - A| <= gamma_(n + 1) |R'| |R| (Higham, Theorem 10.3)
                Rf = np.triu(lanes[0][k][:n, :n].T)
                gamma = (n + 1) * oc.U / (1 - (n + 1) * oc.U)
                assert (np.abs(Rf.T @ Rf - A) <= gamma * (np.abs(Rf).T @ np.abs(Rf))).all(), (lda, n)


@gpu
@pytest.mark.parametrize("op", ["dtrsl01", "dtrsl11", "batch11"])
def test_lbp_solves_64_lanes_equal_one(du, op):
    """triangular factors of random SPD matrices, random right-hand sides; dtrsl also with a zero on the diagonal
    (first, middle, last: it returns that index and leaves b alone).  Same return values, same bits of a, b and sacc."""
    rng = np.random.default_rng(42)
    for lda in (20, 10):
        ns, arrs, bs, want = [], [], [], []
        for _, n in [s for s in LBP_SHAPES if s[0] == lda]:
            if op == "batch11" and 2 * n > lda:
                continue
            for zero in [None] + (sorted({1, (n + 1) // 2, n}) if op != "batch11" else []):
                a, A = lbp_arrays(rng, lda, n)
                Rf = np.linalg.cholesky(A).T
                for j in range(n):
                    a[j, :j + 1] = Rf[:j + 1, j]
                if zero is not None:
                    a[zero - 1, zero - 1] = 0.0
                ns.append(n); arrs.append(a); bs.append(rng.normal(size=lda)); want.append(zero or 0)
        one = du.lbp(False, op, lda, ns, arrs, bs)
        lanes = du.lbp(True, op, lda, ns, arrs, bs)
        for k, n in enumerate(ns):
            assert (one[3][k] == want[k]).all() and (lanes[3][k] == want[k]).all(), (op, lda, n, want[k])
            for o, l in zip(one[:3], lanes[:3]):
                assert same_bits(o[k], l[k]), (op, lda, n, want[k])
            if want[k]:
                assert same_bits(lanes[1][k], bs[k])
            else:  # the solution, against numpy's solve of the same triangle: a factor of condition < 10, n <= 20 - both
                # are within cond gamma_n = 2e-14 of the true solution, relative to its largest component
                T = np.triu(arrs[k][:n, :n].T)
                if op == "batch11":
                    got, ref = lanes[0][k][n:2 * n, :n].T, np.linalg.solve(T.T, arrs[k][n:2 * n, :n].T)
                else:
                    got, ref = lanes[1][k][:n], np.linalg.solve(T if op == "dtrsl01" else T.T, bs[k][:n])
                assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref))), (op, lda, n)


@pytest.fixture(scope="module")
def lanes_host():
    return [(entry, oc.lanes_problem(entry)) for entry in oc.LANES_PROBLEMS]


def test_lanes_problems_have_their_properties(lanes_host):
    """per n of {5, 16} (NMAX 16) and {33, 40, 48} (NMAX 48): an unbounded problem of at least 14 iterations (more than
    m = 10 pairs: both moves ran), a box with some but not all bounds active at the solution, a half-bounded problem"""
    seen = {}
    for entry, q in lanes_host:
        _, nmax, n, _, kind = entry
        t = oc.host_trace(q)
        assert t["success"] and t["nfev"] <= 200, entry
        x, b = t["xfin"], q["bounds"]
        if kind == "none":
            assert b is None and t["nit"] >= 14, entry
        else:
            active = sum((lo is not None and x[i] == lo) or (hi is not None and x[i] == hi) for i, (lo, hi) in enumerate(b))
            if kind == "box":
                assert all(lo is not None and hi is not None for lo, hi in b) and 0 < active < n, (entry, active)
            else:
                assert {(lo is None, hi is None) for lo, hi in b} == {(False, True), (True, True)}, entry
                assert t["nit"] >= 14, entry
        seen.setdefault((nmax, n), set()).add(kind)
    assert seen == {(nmax, n): {"none", "box", "half"} for nmax, n in ((16, 5), (16, 16), (48, 33), (48, 40), (48, 48))}


@gpu
@pytest.mark.parametrize("nmax", [16, 48])
def test_compact_form_64_lanes_equal_one(du, lanes_host, nmax):
    """lbfgsb_nd<NMAX, ., 10, DeviceWave> against OneLane: every x, f, g of every evaluation and the result, bit for bit"""
    for entry, q in lanes_host:
        if entry[1] != nmax:
            continue
        one = du.optimise("one", [q], R=nmax)[0]
        lanes = du.optimise("lanes", [q], R=nmax)[0]
        assert one["nev"] == one["nfev"] <= du.TRACE_CAP and one["success"], entry
        if entry[4] == "none":
            assert one["nit"] >= 14, entry
        diff = same_run(one, lanes)
        assert diff is None, (entry, diff)
