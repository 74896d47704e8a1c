"""CPU: the "point refinement" contract (include/mocap_core.h) as tests/point_refine_reference.py states it -- against SciPy's
converged Levenberg-Marquardt optimum, the cases it must leave alone, the kernel's arithmetic header compiled for the host
(tests/native/refine_check.cpp) bit for bit against the statement, and the five symbols."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import point_refine_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "low-cost-mocap_amd", "csrc")
SYMBOLS = ("mocap_set_point_refinement", "mocap_refine_points", "mocap_refine_points_dev", "mocap_triangulate_refined",
           "mocap_triangulate_refined_dev")
N_GROUPS = 60


def _rig(name):
    from mocap_core import synth
    return {"ring8": lambda: synth.ring_rig(8), "ring2": lambda: synth.ring_rig(2),
            "calib8": lambda: synth.calibrated_ring_rig(8, seed=0)}[name]()


_cache = {}


def _cases(name, integer):
    """Groups of 2 .. C views at 0.3 px noise with their DLT starts and the statement's result at iters = 4: computed once."""
    key = (name, integer)
    if key not in _cache:
        rig = _rig(name)
        rng = np.random.default_rng([len(name), int(integer), 77])
        obs, truth = pr.random_groups(rig, N_GROUPS, rng, noise=0.3, integer=integer)
        P = pr.camera_table(rig["K"], rig["R"], rig["t"])
        views = [pr.obs_views(o)[0] for o in obs]
        starts = np.array([pr.dlt_start(rig["K"], rig["R"], rig["t"], v) for v in views])
        got = [pr.refine(P, v, s, 4) for v, s in zip(views, starts)]
        _cache[key] = dict(rig=rig, P=P, obs=obs, truth=truth, views=views, starts=starts, got=got)
    return _cache[key]


def _residuals(P, views, X):
    out = []
    for c, u, v in views:
        p = np.array(P[c]).reshape(3, 4)
        h = p[:, :3] @ X + p[:, 3]
        out += [h[0] / h[2] - u, h[1] / h[2] - v]
    return np.array(out)


# ---------------------------------------------------------------- against SciPy
@pytest.mark.parametrize("integer", [False, True], ids=["noise", "integer"])
@pytest.mark.parametrize("name", ["ring8", "ring2", "calib8"])
def test_four_steps_reach_scipys_optimum(name, integer):
    from scipy.optimize import least_squares
    cs = _cases(name, integer)
    worst = 0.0
    for views, start, got in zip(cs["views"], cs["starts"], cs["got"]):
        assert got is not None
        sol = least_squares(lambda X: _residuals(cs["P"], views, X), start, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        rel = np.abs(np.array(got[0]) - sol.x).max() / np.abs(sol.x).max()
        worst = max(worst, rel)
    print(f"{name} integer={integer}: worst relative distance to SciPy's optimum {worst:.2e}")
    assert worst < 1e-5


@pytest.mark.parametrize("integer", [False, True], ids=["noise", "integer"])
@pytest.mark.parametrize("name", ["ring8", "ring2", "calib8"])
def test_the_cost_never_rises_over_the_start(name, integer):
    cs = _cases(name, integer)
    for views, start, got in zip(cs["views"], cs["starts"], cs["got"]):
        c0 = pr.evaluate(cs["P"], views, [float(v) for v in start], False)[0]
        assert got[1] <= c0
        for iters in (1, 2, 16):
            assert pr.refine(cs["P"], views, start, iters)[1] <= c0
    # no step at all: the start and its cost
    X, cost, acc = pr.refine(cs["P"], cs["views"][0], cs["starts"][0], 0)
    assert X == [float(v) for v in cs["starts"][0]] and acc == 0 and cost == pr.evaluate(cs["P"], cs["views"][0], X, False)[0]


def test_refined_points_are_closer_to_the_truth_on_the_calibrated_rig():
    cs = _cases("calib8", False)
    refined = np.array([g[0] for g in cs["got"]])
    rms = lambda a: float(np.sqrt(((a - cs["truth"]) ** 2).sum(axis=1).mean()))    # noqa: E731
    before, after = rms(cs["starts"]), rms(refined)
    print(f"calibrated rig: rms distance to the truth {before * 1e3:.2f} mm at the DLT start, {after * 1e3:.2f} mm refined: factor {before / after:.1f}")
    assert after < before


# ---------------------------------------------------------------- what is left alone
def test_parallel_rays_keep_the_start_without_a_step():
    from mocap_core import synth
    rig = synth.ring_rig(2)
    K, R, t = rig["K"], np.array([rig["R"][0], rig["R"][0]]), np.array([rig["t"][0], rig["t"][0]])   # the same pose twice
    P = pr.camera_table(K, R, t)
    # one ray seen twice: the pixel is the start's own projection in the statement's arithmetic, so the start's cost is exactly 0,
    # every point of the ray is a minimum and no trial is strictly better
    for start in ([0.1, -0.2, 3.0], [0.3, 0.1, 2.0]):
        p = P[0]
        w = p[8] * start[0] + p[9] * start[1] + p[10] * start[2] + p[11]
        u = (p[0] * start[0] + p[1] * start[1] + p[2] * start[2] + p[3]) / w
        v = (p[4] * start[0] + p[5] * start[1] + p[6] * start[2] + p[7]) / w
        views = [(0, u, v), (1, u, v)]
        for iters in (1, 4, 16):
            got, cost, acc = pr.refine(P, views, start, iters)
            assert got == start and acc == 0 and cost == 0.0
        assert pr.refine_views(P, views, start, 4) == (start, 0.0, pr.RF_REFINED)       # refined, with 0 accepted steps
    # two different pixels from one pose: the rays meet in the camera centre alone, where no depth is > 0
    assert pr.refine(P, [(0, u, v), (1, u + 1.0, v)], [0.0, 0.0, 0.0], 4) is None


def test_a_start_behind_a_camera_and_a_nan_observation_are_left_untouched():
    cs = _cases("ring8", False)
    P, views = cs["P"], next(v for v in cs["views"] if v[0][0] == 0)       # a group that camera 0 sees
    assert pr.refine(P, views, [0.0, 0.0, -1.0], 4) is None                # behind camera 0
    assert pr.refine(P, views, [np.nan, 0.0, 3.0], 4) is None
    assert pr.refine(P, views, [np.inf, 0.0, 3.0], 4) is None
    assert pr.refine_views(P, views, [0.0, 0.0, -1.0], 4) == (None, None, pr.RF_BAD_START)
    # frame-path form: a NaN blob, an index beyond counts, one view, no view -- xyz and err stay, info says why
    C, M = 8, 4
    blobs = np.zeros((1, C, M, 2), dtype=np.float32)
    counts = np.full((1, C), 3, dtype=np.int32)
    for c, u, v in cs["views"][1]:
        blobs[0, c, 0] = (u, v)
    good = np.full(C, -1, dtype=np.int16)
    good[[c for c, _, _ in cs["views"][1]]] = 0
    blobs[0, :, 1] = np.nan
    rows = np.full((1, 6, C), -1, dtype=np.int16)
    rows[0, 0] = good
    rows[0, 1] = good
    rows[0, 1, np.nonzero(good == 0)[0][0]] = 1            # the NaN blob
    rows[0, 2] = good
    rows[0, 2, np.nonzero(good == 0)[0][0]] = 3            # >= counts
    rows[0, 3, 2] = 0                                      # one view
    rows[0, 5] = good                                      # beyond n_pts
    xyz = np.arange(18, dtype=np.float64).reshape(1, 6, 3) + 100.0
    err = np.arange(6, dtype=np.float64).reshape(1, 6) + 50.0
    start_of = lambda v: pr.dlt_start(cs["rig"]["K"], cs["rig"]["R"], cs["rig"]["t"], v)   # noqa: E731
    out = pr.refine_frames(P, blobs, counts, xyz, err, rows, [5], None, start_of, 4)
    assert out["info"][0].tolist()[1:] == [pr.RF_BAD_OBS, pr.RF_BAD_INDEX, pr.RF_FEW_VIEWS, pr.RF_FEW_VIEWS, 0]
    assert out["info"][0, 0] & pr.RF_REFINED and out["info"][0, 0] >> pr.RF_STEPS_SHIFT >= 1
    assert np.array_equal(out["xyz"][0, 1:], xyz[0, 1:]) and np.array_equal(out["err"][0, 1:], err[0, 1:])
    assert not np.array_equal(out["xyz"][0, 0], xyz[0, 0]) and out["err"][0, 0] < 1.0
    for st, n in ((1, 5), (2, 5), (4, 5), (0, -1), (0, 7)):
        skipped = pr.refine_frames(P, blobs, counts, xyz, err, rows, [n], [st], start_of, 4)
        assert not skipped["info"].any() and np.array_equal(skipped["xyz"], xyz) and np.array_equal(skipped["err"], err)
    # observation form: an infinite coordinate, one view
    obs = np.full((3, C, 2), np.nan)
    obs[0] = pr.views_to_obs(cs["views"][1], C)
    obs[1] = obs[0]
    obs[1, cs["views"][1][0][0], 0] = np.inf
    obs[2, 0] = (1.0, 2.0)
    starts = np.array([start_of(cs["views"][1])] * 3)
    x, e, info = pr.triangulate_refined(P, obs, starts, 4)
    assert info[0] & pr.RF_REFINED and info[1:].tolist() == [pr.RF_BAD_OBS, pr.RF_FEW_VIEWS]
    assert np.isnan(x[1:]).all() and np.isnan(e[1:]).all() and np.isfinite(x[0]).all()


# ---------------------------------------------------------------- the kernel's arithmetic on the host
def _hex(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _host_input(P, cases):
    lines = [str(len(P)), " ".join(_hex(v) for row in P for v in row), str(len(cases))]
    for iters, views, start in cases:
        lines.append("%d %d %s" % (iters, len(views), " ".join(_hex(v) for v in start)))
        lines += ["%d %s %s" % (c, _hex(u), _hex(v)) for c, u, v in views]
    return "\n".join(lines) + "\n"


def _host_cases():
    """Per rig: every group at 1, 4 and 16 steps, and the cases without a step or without a result."""
    out = []
    for name, integer in (("ring8", False), ("calib8", True), ("ring2", False)):
        cs = _cases(name, integer)
        cases = [(iters, v, s) for v, s in zip(cs["views"], cs["starts"]) for iters in (1, 4, 16)]
        cases.append((4, cs["views"][0], [0.0, 0.0, -1.0]))
        cases.append((4, cs["views"][0], [np.nan, 0.0, 3.0]))
        cases.append((0, cs["views"][0], cs["starts"][0]))
        cases.append((16, cs["views"][0][:1], cs["starts"][0]))                           # one view: H is singular
        out.append((cs["P"], cases))
    return out


def _build(tmp_path, *flags):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "refine_check")
    subprocess.check_call([cxx, "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, *flags,
                           os.path.join(ROOT, "tests", "native", "refine_check.cpp"), "-o", exe])
    return exe


def _run_and_compare(exe):
    steps = 0
    for P, cases in _host_cases():
        res = subprocess.run([exe], input=_host_input(P, cases), capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        lines = res.stdout.split("\n")
        assert lines[len(cases)] == "refine checks done"
        for (iters, views, start), line in zip(cases, lines):
            want = pr.refine(P, views, start, iters)
            if want is None:
                assert line == "0", (line, iters, start)
                continue
            X, cost, acc = want
            assert line == "1 %s %s %s %s %d" % (_hex(X[0]), _hex(X[1]), _hex(X[2]), _hex(cost / float(2 * len(views))), acc), (iters, views)
            steps += acc
    assert steps > 300                                    # steps were taken: the comparison is of arithmetic, not of starts


def test_host_build_of_the_kernels_arithmetic_equals_the_statement_bit_for_bit(tmp_path):
    _run_and_compare(_build(tmp_path, "-O2"))


def test_host_build_under_asan_and_ubsan(tmp_path):
    _run_and_compare(_build(tmp_path, "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan"))


# ---------------------------------------------------------------- the symbols
def test_the_five_symbols_are_declared_exported_and_bound():
    from mocap_core import capi, helpers
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert re.search(r"\sT\s+%s\b" % name, exported), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None, name
        args = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(capi.SIGNATURES[name][1]) == len(args.split(",")), name
    assert re.search(r"#define\s+MOCAP_REFINE_MAX_ITERS\s+16\b", text) and capi.REFINE_MAX_ITERS == pr.MAX_ITERS == 16
    for name, mine, theirs in (("REFINED", pr.RF_REFINED, capi.RF_REFINED), ("FEW_VIEWS", pr.RF_FEW_VIEWS, capi.RF_FEW_VIEWS),
                               ("BAD_INDEX", pr.RF_BAD_INDEX, capi.RF_BAD_INDEX), ("BAD_OBS", pr.RF_BAD_OBS, capi.RF_BAD_OBS),
                               ("BAD_START", pr.RF_BAD_START, capi.RF_BAD_START)):
        assert mine == theirs and re.search(r"MOCAP_RF_%s\s*=\s*%d\b" % (name, mine), text), name
    assert re.search(r"#define\s+MOCAP_RF_STEPS_SHIFT\s+8\b", text) and capi.RF_STEPS_SHIFT == pr.RF_STEPS_SHIFT == 8
    for method in ("set_point_refinement", "refine_points", "refine_points_dev", "triangulate_refined", "triangulate_refined_dev"):
        assert callable(getattr(capi.MocapCore, method))
    assert callable(helpers.set_point_refinement) and callable(helpers.triangulate_points_refined) and helpers._state["refine"] == 0
    with pytest.raises(ValueError):
        helpers.set_point_refinement(17)
    assert helpers._state["refine"] == 0
