"""CPU: the "camera resection" contract (include/mocap_core.h) as tests/resection_reference.py states it -- the three symbols, the
refusals that need no device, the statement alone on the four inputs the GPU test uses (planted pose and exactly the planted mask),
the analytic Jacobian against 50-digit central differences, the kernels' arithmetic header compiled for the host
(tests/native/resect_check.cpp, once more under ASan + UBSan) against the statement, and the re-gauge for camera 0."""
import math
import os
import re
import shutil
import struct
import subprocess

import mpmath
import numpy as np
import pytest

import resection_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "low-cost-mocap_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mocap_core.h")
SYMBOLS = ("mocap_resect_camera", "mocap_resect_camera_dev", "mocap_resect_hypotheses")
NAMES = list(rr.CASES)


# ---------------------------------------------------------------- the symbols
def test_the_three_symbols_are_declared_exported_and_bound():
    from mocap_core import capi, helpers
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert re.search(r"\sT\s+%s\b" % name, exported), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None, name
        args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(capi.SIGNATURES[name][1]) == len(args.split(",")), name
    for name, mine, theirs in (("MAX_POINTS", rr.MAX_POINTS, capi.RESECT_MAX_POINTS), ("MAX_HYP", rr.MAX_HYP, capi.RESECT_MAX_HYP),
                               ("INFO", rr.INFO, capi.RESECT_INFO)):
        assert mine == theirs and re.search(r"#define\s+MOCAP_RESECT_%s\s+%d\b" % (name, mine), text), name
    for name, mine, theirs in (("OK", rr.OK, capi.RESECT_OK), ("TOO_FEW", rr.TOO_FEW, capi.RESECT_TOO_FEW),
                               ("NO_MODEL", rr.NO_MODEL, capi.RESECT_NO_MODEL)):
        assert mine == theirs and re.search(r"MOCAP_RESECT_%s\s*=\s*%d\b" % (name, mine), text), name
    assert capi.MocapCore.RESECT_INFO_KEYS == rr.INFO_KEYS and len(rr.INFO_KEYS) == rr.INFO
    for method in ("resect_camera", "resect_camera_dev", "resect_hypotheses"):
        assert callable(getattr(capi.MocapCore, method))
    assert callable(helpers.reseat_camera) and callable(helpers.camera_health)


def test_refusals_that_need_no_device():
    from mocap_core import capi, helpers
    lib = capi.load_library()
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.mocap_resect_camera(None, 1, p, p, p, p, p, 2.0, 1, 0, 4, 1, p, p, p, p) == capi.MOCAP_E_ARG
    assert lib.mocap_resect_camera_dev(None, 1, p, p, p, p, p, 2.0, 1, 0, 4, 1, p, p, p, p) == capi.MOCAP_E_ARG
    assert lib.mocap_resect_hypotheses(None, 1, p, p, p, p, p, 2.0, 1, 0, p, p, p, p) == capi.MOCAP_E_ARG
    assert not buf.any()
    # the wrapper, on an object that has no context: what it refuses itself never reaches the library
    core = object.__new__(capi.MocapCore)
    core.lib, core._h, core.C = lib, None, 0
    c = rr.planted_case(8)
    skew = c["K"].copy()
    skew[0, 1] = 0.5
    prior = (c["R"], c["t"])
    for kw in (dict(K=skew), dict(threshold_px=0.0), dict(threshold_px=-2.0), dict(threshold_px=float("nan")),
               dict(threshold_px=float("inf")), dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=rr.MAX_HYP + 1), dict(min_inliers=3),
               dict(max_iter=-1), dict(X=np.zeros((0, 3)), obs=np.zeros((0, 2))), dict(X=c["X"][:5])):
        args = dict(X=c["X"], obs=c["obs"], K=c["K"])
        args.update(kw)
        with pytest.raises(capi.MocapError) as e:
            core.resect_camera(**args)
        assert e.value.code == capi.MOCAP_E_ARG, kw
    with pytest.raises(capi.MocapError) as e:
        core.resect_hypotheses(c["X"], c["obs"], c["K"], prior=prior, n_hyp=0)      # the probe has no evaluate-only mode
    assert e.value.code == capi.MOCAP_E_ARG
    core._h = None
    # the seam: fewer than three cameras cannot give points without one of them
    helpers.set_camera_params([{"intrinsic_matrix": rr.K_TEST.tolist()}] * 2)
    poses = [{"R": np.eye(3).tolist(), "t": [0, 0, 0]}, {"R": np.eye(3).tolist(), "t": [1, 0, 0]}]
    with pytest.raises(ValueError):
        helpers.reseat_camera([[[1, 2], [3, 4]]], poses, 1)
    with pytest.raises(ValueError):
        helpers.camera_health([[[1, 2], [3, 4]]], poses)


# ---------------------------------------------------------------- the statement alone
def test_the_sampler_is_a_pure_function_with_three_distinct_rows():
    assert rr.mix(0) == 0xe220a8397b1dcdaf                        # splitmix64's first output for the state 0
    seen = set()
    for n in (3, 4, 5, 67, 1031, rr.MAX_POINTS):
        for h in range(300):
            i = rr.sample(rr.SEED, h, n)
            assert len(set(i)) == 3 and all(0 <= k < n for k in i) and i == rr.sample(rr.SEED, h, n)
            seen.add((n, i))
    assert sum(1 for n, _ in seen if n == 3) == 6                  # every order of three rows turns up
    for n in (67, 1031, rr.MAX_POINTS):                            # other counters, other rows: 300 draws of >= 287 430 triples
        assert sum(1 for m, _ in seen if m == n) >= 295
    hits = np.zeros(5)
    for h in range(5000):
        for k in rr.sample(1, h, 5):
            hits[k] += 1
    assert hits.min() > 2700 and hits.max() < 3300                 # 3000 each if uniform


@pytest.mark.parametrize("name", NAMES)
def test_the_statement_recovers_the_planted_pose_and_exactly_the_planted_mask(name):
    c = rr.case(name)
    R, t, mask, info = c["solve"]
    assert info["status"] == rr.OK and info["valid"] == int((np.isfinite(c["X"]).all(axis=1) & np.isfinite(c["obs"]).all(axis=1)).sum())
    assert np.array_equal(mask, c["mask"])                         # the condition the GPU test relies on
    assert info["inliers"] == int(c["mask"].sum()) and info["accepted"] >= 1
    dR, dt = np.abs(R - c["R"]).max(), np.linalg.norm(t - c["t"])
    print(f"{name}: |R - planted| {dR:.2e}, |t - planted| {dt:.2e}, rms winner {info['rms_winner']:.3g} -> final {info['rms_final']:.3g} px, "
          f"{info['accepted']} steps, {info['linearisations']} linearisations")
    if name == "exact6":
        assert dR < 1e-9 and dt < 1e-9
    else:
        assert dR < 2e-3 and dt < 1e-2 and info["rms_final"] < info["rms_winner"]
        rows, idx = c["table"]["rows"], c["table"]["idx"]
        k4 = rr.k4_of(c["K"])
        assert rr.mp_cost(rr.pose_of(R, t), k4, rows, mask[idx]) <= rr.mp_cost(rr.pose_of(c["R"], c["t"]), k4, rows, mask[idx])
    if c["prior"] is not None:
        assert info["rms_prior"] > info["rms_final"] and c["table"]["n_sol"][0] == 1
        assert np.array_equal(c["table"]["poses"][0, 0], rr.pose_of(*c["prior"])) and (c["table"]["sample"][0] == -1).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_statements_solutions_fit_their_samples_and_few_are_ill_conditioned(name):
    c = rr.case(name)
    tab, k4 = c["table"], rr.k4_of(c["K"])
    worst_px = worst_orth = 0.0
    total = ill = 0
    for h in range(tab["poses"].shape[0]):
        if tab["sample"][h, 0] < 0:
            continue
        pick = [int(np.nonzero(tab["idx"] == i)[0][0]) for i in tab["sample"][h]]
        for s in range(int(tab["n_sol"][h])):
            px, orth = rr.mp_sample_error(list(tab["poses"][h, s]), k4, tab["rows"][pick])
            worst_px, worst_orth = max(worst_px, px), max(worst_orth, orth)
            total += 1
            ill += not (tab["cond"][h][s][0] > 1e-6 and tab["cond"][h][s][1] > 1e-6)
    print(f"{name}: {total} solutions ({total / tab['poses'].shape[0]:.2f} per hypothesis), worst sample reprojection {worst_px:.2e} px, "
          f"|R^T R - I| {worst_orth:.2e}, ill-conditioned {ill}")
    assert total >= tab["poses"].shape[0] and worst_px < 1e-5 and worst_orth < 1e-13
    assert ill <= 0.05 * total                                     # a condition on the inputs: the GPU test leaves these out
    # the winner's rule
    h, s, cnt = rr.winner(tab["counts"], tab["n_sol"])
    assert cnt == tab["counts"].max() and (h, s) == min((a, b) for a, b in zip(*np.nonzero(tab["counts"] == cnt)) if b < tab["n_sol"][a])


def test_too_few_no_model_and_evaluate_only():
    c = rr.planted_case(40, outliers=0.2, noise=0.3, prior_off=(3.0, 0.03), seed=5)
    X = c["X"].copy()
    X[3:] = np.nan
    R, t, mask, info = rr.resect(X, c["obs"], c["K"], None, 2.0, 16, 1, 4, 10)
    assert info["status"] == rr.TOO_FEW and info["valid"] == 3 and np.isnan(R).all() and np.isnan(t).all() and not mask.any()
    R, t, mask, info = rr.resect(X, c["obs"], c["K"], c["prior"], 2.0, 16, 1, 4, 10)
    assert info["status"] == rr.TOO_FEW and np.array_equal(R, c["prior"][0]) and np.array_equal(t, c["prior"][1])
    rng = np.random.default_rng(11)
    scrambled = np.stack([rng.uniform(0, 320, 67), rng.uniform(0, 240, 67)], axis=1)
    big = rr.planted_case(67, seed=5)
    R, t, mask, info = rr.resect(big["X"], scrambled, big["K"], None, 2.0, 64, 1, 8, 10)
    assert info["status"] == rr.NO_MODEL and info["winner_inliers"] < 8 and np.isnan(R).all() and info["accepted"] == 0
    # evaluate only: the prior's bits, its mask, its rms
    for n_hyp, max_iter in ((0, 0), (0, 5)):
        R, t, mask, info = rr.resect(c["X"], c["obs"], c["K"], c["prior"], 30.0, n_hyp, 1, 4, max_iter)
        assert info["status"] == rr.OK and (info["winner_hypothesis"], info["winner_solution"]) == (0, 0)
        if max_iter == 0:
            assert np.array_equal(R, c["prior"][0]) and np.array_equal(t, c["prior"][1]) and info["accepted"] == 0
            assert info["rms_prior"] == info["rms_final"] == info["rms_winner"] and 0 < info["inliers"] == mask.sum()
        else:
            assert info["accepted"] >= 1 and info["rms_final"] < info["rms_prior"]


def test_the_analytic_rows_agree_with_50_digit_central_differences():
    c = rr.case("noisy67")
    rows, k4 = c["table"]["rows"], rr.k4_of(c["K"])
    pose = rr.pose_of(*c["solve"][:2])
    worst_mp = worst_f = 0.0
    for row in rows[:12]:
        fd, an = rr.mp_jacobian_fd(pose, k4, row)
        P, x, xn, yn, _, _, _ = rr.view(pose, k4, row)
        Jf = rr.jacobian(P, x, xn, yn, k4)
        for r in range(2):
            scale = max(abs(v) for v in an[r])
            for i in range(6):
                worst_mp = max(worst_mp, float(abs(fd[r][i] - an[r][i]) / scale))
                worst_f = max(worst_f, float(abs(mpmath.mpf(Jf[r][i]) - an[r][i]) / scale))
    print(f"analytic rows: {worst_mp:.2e} from 50-digit central differences (step 1e-20), the double rows {worst_f:.2e} from the 50-digit rows")
    assert worst_mp < 1e-30          # the truncation error of a central difference at h = 1e-20 is O(h^2)
    assert worst_f < 1e-13           # the doubles: a handful of roundings, and R orthonormal to 1e-16 only


def test_the_regauge_leaves_world_coordinates_where_they_were():
    from mocap_core import synth
    rig = synth.ring_rig(4)
    rng = np.random.default_rng(3)
    R0 = np.array(rr.apply_step(rr.pose_of(np.eye(3), np.zeros(3)), list(rng.normal(size=3) * 0.05) + [0.0] * 3)[:9]).reshape(3, 3)
    t0 = rng.normal(size=3) * 0.03
    Rn, tn, M = rr.regauge(rig["R"], rig["t"], R0, t0)
    assert np.array_equal(Rn[0], np.eye(3)) and not tn[0].any()
    X = rng.uniform(-1, 1, (20, 3))                   # points in the old frame; X' = R0 X + t0 in the new one
    Xn = X @ R0.T + t0
    for c in range(1, 4):                             # every other camera sees them where it did
        assert np.abs((X @ rig["R"][c].T + rig["t"][c]) - (Xn @ Rn[c].T + tn[c])).max() < 1e-14
    D = np.diag([-1.0, -1.0, 1.0])
    W = np.eye(4)
    W[:3, :3] = np.array(rr.apply_step(rr.pose_of(np.eye(3), np.zeros(3)), [0.3, -0.2, 0.1, 0, 0, 0])[:9]).reshape(3, 3) * 1.7
    W[:3, 3] = [0.4, -1.0, 2.0]
    world = lambda W, X: (np.c_[X @ D, np.ones(len(X))] @ W.T)[:, :3]    # noqa: E731  the live loop: W (D X, 1)
    assert np.abs(world(W, X) - world(W @ M, Xn)).max() < 1e-14


# ---------------------------------------------------------------- the kernels' arithmetic on the host
def _hex(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _words(vals):
    return " ".join(_hex(v) for v in vals)


def _build(tmp_path, *flags):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "resect_check")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, *flags,
                           os.path.join(ROOT, "tests", "native", "resect_check.cpp"), "-o", exe])
    return exe


def _unhex(w):
    return struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0]


def _run_and_compare(exe):
    steps = checked_solutions = 0
    for name in NAMES:
        c = rr.case(name)
        tab, k4 = c["table"], rr.k4_of(c["K"])
        rows, n = tab["rows"], len(tab["idx"])
        H = tab["poses"].shape[0]
        cands = [(h, s) for h in range(H) for s in range(int(tab["n_sol"][h]))][:40]
        win = rr.winner(tab["counts"], tab["n_sol"])
        wpose = [float(v) for v in tab["poses"][win[0], win[1]]]
        sampled = [h for h in range(H) if tab["sample"][h, 0] >= 0][:40]
        picks = {h: [int(np.nonzero(tab["idx"] == i)[0][0]) for i in tab["sample"][h]] for h in sampled}
        lines = [_words(k4 + [rr.THRESHOLD]), str(n)] + [_words(r) for r in rows]
        lines += ["sample %d %d %d" % (rr.SEED, h, n) for h in sampled]
        lines += ["score " + _words(tab["poses"][h, s]) for h, s in cands]
        lines += ["row %d %s" % (i, _words(wpose)) for i in range(min(n, 20))]
        lines += ["refine %d %s" % (rr.MAX_ITER, _words(wpose))]
        lines += ["p3p %d %d %d" % tuple(picks[h]) for h in sampled]
        lines += ["end"]
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        out = res.stdout.split("\n")
        assert out[len(lines) - 2 - n - 1] == "resect checks done"
        it = iter(out)
        for h in sampled:                                         # the sampler
            assert [int(v) for v in next(it).split()] == picks[h], (name, h)
        for h, s in cands:                                        # scoring: counts and masks
            count, bits = next(it).split()
            want = rr.classify(list(tab["poses"][h, s]), k4, rows, rr.THRESHOLD)
            assert int(count) == tab["counts"][h, s] == want.sum() and bits == "".join("1" if b else "0" for b in want), (name, h, s)
        for i in range(min(n, 20)):                               # the rows of a linearisation, bit for bit
            assert next(it).split() == [_hex(v) for v in rr.row_sums(wpose, k4, rows[i])], (name, i)
        got = next(it).split()                                    # the two rounds: the same folds in the same order, bit for bit
        pose, accepted, lins = rr.refine(wpose, k4, rows, rr.THRESHOLD, rr.MAX_ITER)
        assert got[:12] == [_hex(v) for v in pose] and [int(got[12]), int(got[13])] == [accepted, lins], name
        assert [_unhex(w) for w in got[:12]] == rr.pose_of(*c["solve"][:2])
        steps += accepted
        for h in sampled:                                         # the three-point solver, by residual
            got = next(it).split()
            ns = int(got[0])
            assert ns == tab["n_sol"][h], (name, h)
            for s in range(ns):
                pose = [_unhex(w) for w in got[1 + 12 * s:13 + 12 * s]]
                px, orth = rr.mp_sample_error(pose, k4, rows[picks[h]])
                assert px < 1e-5 and orth < 1e-13, (name, h, s, px, orth)
                if min(tab["cond"][h][s]) > 1e-6:
                    assert np.abs(np.array(pose) - tab["poses"][h, s]).max() < 1e-6, (name, h, s)
                checked_solutions += 1
    assert steps >= 8 and checked_solutions > 100                 # steps were taken, solutions were compared


def test_host_build_of_the_kernels_arithmetic_equals_the_statement(tmp_path):
    _run_and_compare(_build(tmp_path, "-O2"))


def test_host_build_under_asan_and_ubsan(tmp_path):
    _run_and_compare(_build(tmp_path, "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan"))


def test_the_step_is_the_cholesky_solution():
    c = rr.case("noisy67")
    rows, k4 = c["table"]["rows"], rr.k4_of(c["K"])
    pose = [float(v) for v in c["table"]["poses"][c["solve"][3]["winner_hypothesis"], c["solve"][3]["winner_solution"]]]
    s = rr.linearise(pose, k4, rows, rr.classify(pose, k4, rows, rr.THRESHOLD))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s[:21]
    H = H + np.triu(H, 1).T
    for lam in (0.0, 1e-3, 10.0):
        d = rr.lm_step(s, lam)
        want = np.linalg.solve(H + lam * np.diag(np.diag(H)), -np.array(s[21:27]))
        assert np.abs(np.array(d) - want).max() <= 1e-9 * np.abs(want).max()
    assert rr.lm_step([0.0] * 31, 1e-3) is None and math.isnan(rr.resect(np.zeros((1, 3)), np.zeros((1, 2)), rr.K_TEST)[0][0, 0])
