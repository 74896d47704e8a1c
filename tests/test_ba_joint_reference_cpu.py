"""Joint bundle adjustment without a GPU (include/mocap_core.h, "joint bundle adjustment"): the symbols are declared, exported and
bound; the refusals that need no device; and the plain statement of the contract, tests/ba_joint_reference.py, checked on its own:
its Jacobian blocks against 50-digit central differences, its integer algebra against mpmath run end to end, and the loop on the
inputs the device tests use (exact data, the Huber input, the noisy 8-camera rig)."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import ba_joint_reference as bj
from conftest import ROOT

np.seterr(all="ignore")
HEADER = os.path.join(ROOT, "include", "mocap_core.h")
CAP = 1e-9   # pose error on exact data: six orders above what the loop reaches (1e-15), seven below the start (2e-2)


def test_the_section_is_declared_exported_and_bound():
    from mocap_core import capi, helpers
    text = open(HEADER).read()
    lib = capi.load_library()
    for name in ("mocap_ba_joint_normal_eq", "mocap_ba_joint_solve"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None
    for name, mine in (("MAX_CAMERAS", bj.MAX_CAMERAS), ("MAX_POINTS", bj.MAX_POINTS), ("INFO", 12)):
        assert re.search(r"#define\s+MOCAP_BAJ_%s\s+%d\b" % (name, mine), text) and getattr(capi, "BAJ_" + name) == mine
    assert re.search(r"#define\s+MOCAP_BAJ_FOCAL\s+1u", text) and capi.BAJ_FOCAL == 1
    for name in ("CAMERA_UNSEEN", "NO_POINTS", "SINGULAR", "POINT_SINGULAR", "LAMBDA", "MAX_ITER", "BAD_DEPTH"):
        mine = getattr(bj, "ST_" + name)
        assert getattr(capi, "BAJ_ST_" + name) == mine and re.search(r"MOCAP_BAJ_ST_%s\s*=\s*%d\b" % (name, mine), text), name
    assert callable(capi.MocapCore.ba_joint_normal_eq) and callable(capi.MocapCore.ba_joint_solve)
    assert callable(helpers.bundle_adjustment_joint)
    assert helpers.DEFAULT_BA_MODE == "scipy"   # the seam is beside bundle_adjustment: its default has not moved


def test_refusals_that_need_no_device():
    from mocap_core import capi, helpers
    lib = capi.load_library()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    # the library: a null context is refused before anything is read
    assert lib.mocap_ba_joint_normal_eq(None, 1, p, p, p, p, p, 0, 0.0, 0.0, p, p, p, p) == capi.MOCAP_E_ARG
    assert lib.mocap_ba_joint_solve(None, 1, p, p, p, p, p, 0, 0.0, 0.0, 1, p) == capi.MOCAP_E_ARG
    assert not buf.any()
    # the wrapper, on an object that has no context: what it refuses itself never reaches the library
    core = object.__new__(capi.MocapCore)
    core.lib, core._h, core.C = lib, None, 2
    obs, R, t = np.zeros((3, 2, 2)), np.stack([np.eye(3)] * 2), np.zeros((2, 3))
    for kw in (dict(refine_focal=True), dict(huber_px=-1.0), dict(huber_px=float("nan")), dict(ftol=-1e-3), dict(ftol=float("inf")),
               dict(max_iter=0)):
        with pytest.raises(capi.MocapError) as e:
            core.ba_joint_solve(obs, R, t, **kw)
        assert e.value.code == capi.MOCAP_E_ARG, kw
    with pytest.raises(capi.MocapError) as e:
        core.ba_joint_normal_eq(obs, R, t, np.zeros((3, 3)), refine_focal=True)
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        core.ba_joint_solve(obs, R[:1], t)       # poses of another camera count
    assert e.value.code == capi.MOCAP_E_ARG
    core._h = None
    # the seam
    poses = [{"R": np.eye(3).tolist(), "t": [0, 0, 0]}, {"R": np.eye(3).tolist(), "t": [1, 0, 0]}]
    for kw in (dict(refine_focal=True), dict(huber_px=-2.0), dict(max_iter=0), dict(ftol=float("nan"))):
        with pytest.raises(ValueError):
            helpers.bundle_adjustment_joint([[[1, 2], [3, 4]]], poses, **kw)
    # the reference states the same rules
    K = np.array([[[300.0, 0, 160], [0, 300, 160], [0, 0, 1]]] * 3)
    assert bj.check_args(3, 5, K, True) is None and bj.check_args(2, 5, K[:2], False) is None
    skew = K.copy()
    skew[1, 0, 1] = 0.5
    for bad in (bj.check_args(1, 5, K[:1], False), bj.check_args(17, 5, np.repeat(K[:1], 17, 0), False), bj.check_args(2, 0, K[:2], False),
                bj.check_args(2, bj.MAX_POINTS + 1, K[:2], False), bj.check_args(3, 5, skew, False), bj.check_args(2, 5, K[:2], True),
                bj.check_args(3, 5, K, False, huber_px=-1.0), bj.check_args(3, 5, K, False, ftol=float("nan")),
                bj.check_args(3, 5, K, False, max_iter=0), bj.check_args(3, 5, K, False, lam=-1.0)):
        assert bad is not None


# ------------------------------------------------------------------------------------------------- the Jacobian blocks, 50 digits
def _mp_residual(R, t, K, s, X, uv, w, dt, ds, dX):
    """r at the camera moved by (w, dt, ds) and the point moved by dX, all mpmath."""
    mp = mpmath
    th = mp.sqrt(sum(v * v for v in w))
    Wx = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = mp.eye(3) if th == 0 else mp.eye(3) + (mp.sin(th) / th) * Wx + ((1 - mp.cos(th)) / th ** 2) * (Wx * Wx)
    Rm = E * mp.matrix(R.tolist())
    Y = Rm * mp.matrix([mp.mpf(float(X[k])) + dX[k] for k in range(3)]) + mp.matrix([mp.mpf(float(t[k])) + dt[k] for k in range(3)])
    f = mp.mpf(float(s)) * (1 + ds)
    return [mp.mpf(float(K[0, 0])) * f * Y[0] / Y[2] + mp.mpf(float(K[0, 2])) - mp.mpf(float(uv[0])),
            mp.mpf(float(K[1, 1])) * f * Y[1] / Y[2] + mp.mpf(float(K[1, 2])) - mp.mpf(float(uv[1]))]


def test_analytic_blocks_agree_with_50_digit_central_differences():
    rig, obs, X0, start = bj.planted_case(4, 12, noise_px=0.3, calibrated=True)
    h = mpmath.mpf(10) ** -20
    worst_f = worst_mp = 0.0
    with mpmath.workdps(bj.DPS):
        for c in (1, 3):
            s = 1.0 + 0.01 * c
            for p in range(12):
                if np.isnan(obs[p, c, 0]):
                    continue
                R, t, K, X, uv = start["R"][c], start["t"][c], rig["K"][c], X0[p] + 0.01, obs[p, c]
                cd = []
                for k in range(10):      # w 3, t 3, focal scale, X 3
                    d = [mpmath.mpf(0)] * 10
                    d[k] = h
                    rp = _mp_residual(R, t, K, s, X, uv, d[0:3], d[3:6], d[6], d[7:10])
                    d[k] = -h
                    rm = _mp_residual(R, t, K, s, X, uv, d[0:3], d[3:6], d[6], d[7:10])
                    cd.append([(a - b) / (2 * h) for a, b in zip(rp, rm)])
                for F in (bj.FLOAT, bj.MP):
                    lift = (lambda v: float(v)) if F is bj.FLOAT else (lambda v: mpmath.mpf(float(v)))
                    v = bj.view_terms(F, [[lift(x) for x in row] for row in R], [lift(x) for x in t], lift(K[0, 0]) * lift(s),
                                      lift(K[1, 1]) * lift(s), lift(K[0, 2]), lift(K[1, 2]), [F.lift([x]) for x in X],
                                      F.lift([uv[0]]), F.lift([uv[1]]), 0.0)
                    rows = [[a[0] for a in v["Au"]] + [a[0] for a in v["Bu"]], [a[0] for a in v["Av"]] + [a[0] for a in v["Bv"]]]
                    for r in range(2):
                        scale = max(abs(x[r]) for x in cd)
                        err = max(abs(mpmath.mpf(rows[r][k]) - cd[k][r]) for k in range(10)) / scale
                        if F is bj.FLOAT:
                            worst_f = max(worst_f, float(err))
                        else:
                            worst_mp = max(worst_mp, float(err))
    print(f"analytic rows against 50-digit central differences (h = 1e-20): doubles {worst_f:.2e}, mpmath {worst_mp:.2e} of the row's largest entry")
    # the difference of two 50-digit residuals of up to 1e3 px carries 1e-46 px, over 2 h = 2e-20: 5e-27 per entry, relative to a
    # row whose largest entry is at least 1; the truncation, O(h^2) = 1e-40, is far below.  A wrong term shows at O(1).
    assert worst_mp < 1e-25
    assert worst_f < 1e-13       # plain doubles: a few ulp through ~20 operations


def test_huber_rows_are_the_plain_rows_times_sqrt_w():
    with mpmath.workdps(bj.DPS):
        R = [[mpmath.mpf(x) for x in row] for row in np.eye(3).tolist()]
        t = [mpmath.mpf(0)] * 3
        X = [bj.MP.lift([0.1]), bj.MP.lift([-0.2]), bj.MP.lift([2.0])]
        args = (bj.MP, R, t, mpmath.mpf(300), mpmath.mpf(310), mpmath.mpf(160), mpmath.mpf(150), X, bj.MP.lift([170.0]), bj.MP.lift([126.0]))
        plain, hub = bj.view_terms(*args, 0.0), bj.view_terms(*args, 2.0)
        s = mpmath.sqrt(plain["rho"][0])
        assert s > 2 and hub["down"][0] and not plain["down"][0]
        sw = mpmath.sqrt(2 / s)
        assert abs(hub["rho"][0] - (4 * s - 4)) < 1e-40
        for k in ("ru", "rv"):
            assert abs(hub[k][0] - sw * plain[k][0]) < 1e-40
        for k in ("Au", "Av", "Bu", "Bv"):
            for a, b in zip(hub[k], plain[k]):
                assert abs(a[0] - sw * b[0]) < 1e-40


def test_the_integer_algebra_is_mpmath_to_45_digits():
    rig, obs, _, start = bj.planted_case(3, 5, noise_px=0.3, calibrated=True)
    X = bj.dlt_start(obs, start["R"], start["t"], rig["K"])
    fs = np.array([1.0, 1.01, 0.99])
    a = bj.linearise_mp(obs, start["R"], start["t"], rig["K"], X, fs, True, 2.0, 1e-3)
    b = bj.linearise_mp(obs, start["R"], start["t"], rig["K"], X, fs, True, 2.0, 1e-3, algebra=bj.MP)
    with mpmath.workdps(bj.DPS):
        for k in ("S", "rhs"):
            scale = max(abs(v) for v in b[k].ravel())
            assert max(abs(x - y) for x, y in zip(a[k].ravel(), b[k].ravel())) < scale * mpmath.mpf(10) ** -45
        assert a["cost"] == b["cost"]
    d = bj.linearise(obs, start["R"], start["t"], rig["K"], X, fs, True, 2.0, 1e-3)
    assert max(bj.rel_errors(d, a)) < 1e-13


# ----------------------------------------------------------------------------------------------------------------------- loop
@pytest.mark.parametrize("C,N", [(2, 67), (3, 5), (4, 200)])
def test_reference_recovers_planted_poses_on_exact_data(C, N):
    rig, obs, X0, start = bj.planted_case(C, N)
    assert bj.pose_errors(start["R"], start["t"], rig)[0] > 1e-2
    R, t, _, X, info = bj.solve(obs, start["R"], start["t"], rig["K"])
    rot, tr = bj.pose_errors(R, t, rig)
    print(f"C={C} N={N}: rotation {rot:.2e} rad, translation {tr:.2e} |t1|, {info['accepted']} accepted of {info['passes']} passes")
    assert rot <= CAP and tr <= CAP
    part = ~np.isnan(X[:, 0])
    assert part.sum() == info["participating"] and info["excluded"] == N - part.sum()
    assert np.array_equal(part, (~np.isnan(obs[..., 0])).sum(axis=1) >= 2)
    k = np.linalg.norm(rig["t"][1]) / np.linalg.norm(t[1])
    assert np.abs(X[part] * k - X0[part]).max() <= CAP * np.linalg.norm(rig["t"][1])
    assert np.array_equal(R[0], start["R"][0]) and np.array_equal(t[0], start["t"][0])
    assert abs(np.linalg.norm(t[1]) - np.linalg.norm(start["t"][1])) <= 4 * np.spacing(np.linalg.norm(start["t"][1]))


def test_reference_huber_condition():
    rig, clean, bad, moved, start = bj.outlier_case()
    e_clean = bj.pose_errors(*bj.solve(clean, start["R"], start["t"], rig["K"], max_iter=50)[:2], rig)
    off = bj.solve(bad, start["R"], start["t"], rig["K"], huber=0.0, max_iter=50)
    on = bj.solve(bad, start["R"], start["t"], rig["K"], huber=2.0, max_iter=50)
    e_off, e_on = bj.pose_errors(off[0], off[1], rig), bj.pose_errors(on[0], on[1], rig)
    print(f"clean {e_clean[0] * 1e3:.2f} mrad / {e_clean[1]:.2e}; {moved} outliers, Huber off {e_off[0] * 1e3:.2f} mrad / {e_off[1]:.2e}, "
          f"at 2 px {e_on[0] * 1e3:.2f} mrad / {e_on[1]:.2e}; down-weighted {on[4]['down_weighted']}")
    assert e_on[0] <= 0.25 * e_off[0] and e_on[1] <= 0.25 * e_off[1]
    assert on[4]["down_weighted"] >= moved


def test_reference_is_monotone_on_the_noisy_rig():
    # (the device test starts from the poses mocap_ba_solve returns; without a GPU the start is perturb_rig's)
    rig, obs, _, start = bj.planted_case(8, 257, noise_px=0.3)
    costs = []
    _, _, _, _, info = bj.solve(obs, start["R"], start["t"], rig["K"], progress=lambda R, t, c: costs.append(c))
    assert info["cost"] <= info["cost0"] and len(costs) == info["accepted"] >= 1
    assert all(b < a for a, b in zip([info["cost0"]] + costs, costs))
    assert costs[-1] == info["cost"]
