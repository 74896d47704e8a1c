"""Lens calibration without a GPU (include/mocap_core.h, "lens calibration"): the symbols are declared, exported and bound; the
refusals that need no device; and the plain statement of the contract, tests/ba_lens_reference.py, checked on its own: all 14 columns
of A and the 3 of B against 50-digit central differences, its integer algebra against mpmath run end to end, the Newton inverse of
the lens, and the loop on exact and on noisy captures that fill the images."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import ba_joint_reference as bj
import ba_lens_reference as bl
from conftest import ROOT

np.seterr(all="ignore")
HEADER = os.path.join(ROOT, "include", "mocap_core.h")
CAP = 1e-9   # pose and lens error on exact data: six orders above what the loop reaches (1e-15), seven below the start (2e-2)


def test_the_section_is_declared_exported_and_bound():
    from mocap_core import capi, helpers
    text = open(HEADER).read()
    lib = capi.load_library()
    for name in ("mocap_ba_lens_normal_eq", "mocap_ba_lens_solve", "mocap_undistort_points", "mocap_undistort_points_dev"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and getattr(lib, name) is not None
    for name, mine in (("BAL_MAX_CAMERAS", bl.MAX_CAMERAS), ("BAL_MAX_POINTS", bl.MAX_POINTS), ("BAL_INFO", 12), ("UNDISTORT_NEWTON", bl.NEWTON),
                       ("UNDISTORT_MAX_POINTS", 1 << 20)):
        assert re.search(r"#define\s+MOCAP_%s\s+%d\b" % (name, mine), text) and getattr(capi, name) == mine, name
    for name in ("FOCAL", "CENTRE", "RADIAL", "TANGENTIAL"):
        mine = getattr(bl, name)
        assert re.search(r"#define\s+MOCAP_BAL_%s\s+%du" % (name, mine), text) and getattr(capi, "BAL_" + name) == mine
        assert capi.BAL_REFINE[name.lower()] == mine
    for name in ("CAMERA_UNSEEN", "NO_POINTS", "SINGULAR", "POINT_SINGULAR", "LAMBDA", "MAX_ITER", "BAD_DEPTH"):
        mine = getattr(bl, "ST_" + name)
        assert getattr(capi, "BAL_ST_" + name) == mine == getattr(capi, "BAJ_ST_" + name)
        assert re.search(r"MOCAP_BAL_ST_%s\s*=\s*%d\b" % (name, mine), text), name
    for fn in ("ba_lens_normal_eq", "ba_lens_solve", "undistort_points", "undistort_points_dev"):
        assert callable(getattr(capi.MocapCore, fn))
    assert callable(helpers.calibrate_lenses) and callable(helpers.undistort_image_points)
    assert "fill" in helpers.calibrate_lenses.__doc__.lower() and "distortion_coef = 0" in helpers.calibrate_lenses.__doc__


def test_refusals_that_need_no_device():
    from mocap_core import capi, helpers
    lib = capi.load_library()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    # the library: a null context is refused before anything is read
    assert lib.mocap_ba_lens_normal_eq(None, 3, 1, p, p, p, p, p, p, 0, 0.0, 0.0, p, p, p, p) == capi.MOCAP_E_ARG
    assert lib.mocap_ba_lens_solve(None, 3, 1, p, p, p, p, p, p, 0, 0.0, 0.0, 1, p) == capi.MOCAP_E_ARG
    assert lib.mocap_undistort_points(None, 3, 1, p, p, p, p) == capi.MOCAP_E_ARG
    assert lib.mocap_undistort_points_dev(None, 3, 1, p, p, p, p) == capi.MOCAP_E_ARG
    assert not buf.any()
    # the wrapper, on an object that has no context: what it refuses itself never reaches the library
    core = object.__new__(capi.MocapCore)
    core.lib, core._h, core.C = lib, None, 0
    K3 = np.array([[[300.0, 0, 160], [0, 300, 160], [0, 0, 1]]] * 3)
    d3 = np.zeros((3, 5))
    obs, R, t = np.zeros((4, 3, 2)), np.stack([np.eye(3)] * 3), np.zeros((3, 3))
    skew, neg, nand = K3.copy(), K3.copy(), d3.copy()
    skew[1, 0, 1] = 0.5
    neg[2, 1, 1] = -300.0
    nand[0, 3] = np.nan
    for kw in (dict(huber_px=-1.0), dict(huber_px=float("nan")), dict(ftol=-1e-3), dict(ftol=float("inf")), dict(max_iter=0),
               dict(refine=("focal", "skew")), dict(refine=16), dict(K=skew), dict(K=neg), dict(dist=nand), dict(K=K3[:2]),
               dict(obs=np.zeros((4, 2, 2)))):
        a = dict(obs=obs, R=R, t=t, K=K3, dist=d3)
        a.update(kw)
        with pytest.raises(capi.MocapError) as e:
            core.ba_lens_solve(**a)
        assert e.value.code == capi.MOCAP_E_ARG, kw
    with pytest.raises(capi.MocapError) as e:
        core.ba_lens_solve(obs[:, :2], R[:2], t[:2], K3[:2], d3[:2], refine=("focal",))      # any flag needs three cameras
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        core.ba_lens_normal_eq(obs, R, t, K3, d3, np.zeros((4, 3)), lam=-1.0)
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        core.undistort_points(np.zeros((4, 3, 2)), K3[:2], d3)
    assert e.value.code == capi.MOCAP_E_ARG
    # the seam
    poses = [{"R": np.eye(3).tolist(), "t": [float(c), 0, 0]} for c in range(3)]
    helpers.set_camera_params([{"intrinsic_matrix": K3[c].tolist()} for c in range(3)])
    pts = [[[1, 2], [3, 4], [5, 6]]]
    for kw in (dict(refine=("wide",)), dict(refine=16), dict(huber_px=-2.0), dict(max_iter=0), dict(ftol=float("nan"))):
        with pytest.raises(ValueError):
            helpers.calibrate_lenses(pts, poses, **kw)
    with pytest.raises(ValueError):
        helpers.calibrate_lenses([[[1, 2], [3, 4]]], poses[:2])
    # the reference states the same rules
    assert bl.check_args(3, 5, K3, d3, bl.ALL) is None and bl.check_args(2, 5, K3[:2], d3[:2], 0) is None
    for bad in (bl.check_args(1, 5, K3[:1], d3[:1], 0), bl.check_args(17, 5, np.repeat(K3[:1], 17, 0), np.zeros((17, 5)), 0),
                bl.check_args(3, 0, K3, d3, 0), bl.check_args(3, bl.MAX_POINTS + 1, K3, d3, 0), bl.check_args(3, 5, skew, d3, 0),
                bl.check_args(3, 5, neg, d3, 0), bl.check_args(3, 5, K3, nand, 0), bl.check_args(2, 5, K3[:2], d3[:2], bl.CENTRE),
                bl.check_args(3, 5, K3, d3, 16), bl.check_args(3, 5, K3, d3, 0, huber_px=-1.0), bl.check_args(3, 5, K3, d3, 0, ftol=float("nan")),
                bl.check_args(3, 5, K3, d3, 0, max_iter=0), bl.check_args(3, 5, K3, d3, 0, lam=-1.0)):
        assert bad is not None
    assert [bl.n_cam_params(16, bl.ALL), bl.n_cam_params(3, 0), bl.n_cam_params(3, bl.RADIAL)] == [218, 12, 18]
    assert bl.columns(3, 0, bl.CENTRE | bl.TANGENTIAL) == [-1] * 8 + [12, 13, -1, -1, 14, 15]
    assert bl.columns(3, 2, bl.ALL)[:7] == [6, 7, 8, 9, 10, 11, 12 + 16]


# ------------------------------------------------------------------------------------------------- the Jacobian blocks, 50 digits
def _mp_residual(R, t, a, X, uv, d):
    """r at the camera moved by d[0:14] (w, dt, fx and fy scaled by 1 + d, the other intrinsics + d) and the point by d[14:17]."""
    mp = mpmath
    w = d[0:3]
    th = mp.sqrt(sum(v * v for v in w))
    Wx = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = mp.eye(3) if th == 0 else mp.eye(3) + (mp.sin(th) / th) * Wx + ((1 - mp.cos(th)) / th ** 2) * (Wx * Wx)
    Y = E * mp.matrix(R.tolist()) * mp.matrix([mp.mpf(float(X[k])) + d[14 + k] for k in range(3)]) + \
        mp.matrix([mp.mpf(float(t[k])) + d[3 + k] for k in range(3)])
    fx, fy = mp.mpf(float(a[0])) * (1 + d[6]), mp.mpf(float(a[1])) * (1 + d[7])
    cx, cy = mp.mpf(float(a[2])) + d[8], mp.mpf(float(a[3])) + d[9]
    k1, k2, p1, p2 = (mp.mpf(float(a[4 + i])) + d[10 + i] for i in range(4))
    k3 = mp.mpf(float(a[8]))
    x, y = Y[0] / Y[2], Y[1] / Y[2]
    r2 = x * x + y * y
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3        # the textbook form, not the reference's nesting
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return [fx * xd + cx - mp.mpf(float(uv[0])), fy * yd + cy - mp.mpf(float(uv[1]))]


def test_analytic_blocks_agree_with_50_digit_central_differences():
    rig, obs, X0, start = bl.planted_case(4, 12, noise_px=0.3)
    a = bl.intrinsics(rig["K"], rig["dist"])
    a[:, 8] = -0.2                                     # k3 is in the model
    h = mpmath.mpf(10) ** -20
    worst_f = worst_mp = 0.0
    checked = 0
    with mpmath.workdps(bl.DPS):
        for c in (1, 3):
            for p in range(12):
                if np.isnan(obs[p, c, 0]):
                    continue
                checked += 1
                R, t, X, uv = start["R"][c], start["t"][c], X0[p] + 0.01, obs[p, c]
                cd = []
                for k in range(17):      # w 3, t 3, fx fy cx cy k1 k2 p1 p2, X 3
                    d = [mpmath.mpf(0)] * 17
                    d[k] = h
                    rp = _mp_residual(R, t, a[c], X, uv, d)
                    d[k] = -h
                    rm = _mp_residual(R, t, a[c], X, uv, d)
                    cd.append([(x - y) / (2 * h) for x, y in zip(rp, rm)])
                for F in (bl.FLOAT, bl.MP):
                    lift = (lambda v: float(v)) if F is bl.FLOAT else (lambda v: mpmath.mpf(float(v)))
                    v = bl.view_terms(F, [[lift(x) for x in row] for row in R], [lift(x) for x in t], [lift(x) for x in a[c]],
                                      [F.lift([x]) for x in X], F.lift([uv[0]]), F.lift([uv[1]]), 0.0)
                    rows = [[x[0] for x in v["Au"]] + [x[0] for x in v["Bu"]], [x[0] for x in v["Av"]] + [x[0] for x in v["Bv"]]]
                    for r in range(2):
                        scale = max(abs(x[r]) for x in cd)
                        err = max(abs(mpmath.mpf(rows[r][k]) - cd[k][r]) for k in range(17)) / scale
                        if F is bl.FLOAT:
                            worst_f = max(worst_f, float(err))
                        else:
                            worst_mp = max(worst_mp, float(err))
    print(f"{checked} views, 17 columns each, against 50-digit central differences (h = 1e-20): doubles {worst_f:.2e}, mpmath "
          f"{worst_mp:.2e} of the row's largest entry")
    assert checked >= 12
    # as in the joint bundle adjustment's test: two 50-digit residuals of up to 1e3 px carry 1e-46 px, over 2 h = 2e-20: 5e-27 per
    # entry, relative to a row whose largest entry is at least 1; the truncation, O(h^2) = 1e-40, is far below.  A wrong term shows
    # at O(1).
    assert worst_mp < 1e-25
    assert worst_f < 1e-13       # plain doubles: a few ulp through ~40 operations


def test_flags_zero_and_no_lens_is_the_joint_bundle_adjustment():
    """With zero coefficients and no intrinsic unknown the section's S, rhs and cost are the joint bundle adjustment's, to rounding
    (Jxx = Jyy = 1, Jxy = 0: the same terms, a few more operations)."""
    rig, obs, _, start = bj.planted_case(3, 20, noise_px=0.3, calibrated=True)
    X = bj.dlt_start(obs, start["R"], start["t"], rig["K"])
    a = bl.linearise(obs, start["R"], start["t"], rig["K"], np.zeros((3, 5)), X, 0, 2.0, 1e-3)
    b = bj.linearise(obs, start["R"], start["t"], rig["K"], X, None, False, 2.0, 1e-3)
    assert np.abs(a["S"] - b["S"]).max() <= 1e-12 * np.abs(b["S"]).max() and np.abs(a["rhs"] - b["rhs"]).max() <= 1e-12 * np.abs(b["rhs"]).max()
    assert a["cost"] == b["cost"] and a["down"] == b["down"]


def test_the_integer_algebra_is_mpmath_to_45_digits():
    rig, obs, _, start = bl.planted_case(3, 5, noise_px=0.3)
    X = bj.dlt_start(obs, start["R"], start["t"], rig["K"])
    args = (obs, start["R"], start["t"], rig["K"], rig["dist"], X, bl.ALL, 2.0, 1e-3)
    a = bl.linearise_mp(*args)
    b = bl.linearise_mp(*args, algebra=bl.MP)
    with mpmath.workdps(bl.DPS):
        for k in ("S", "rhs"):
            scale = max(abs(v) for v in b[k].ravel())
            assert max(abs(x - y) for x, y in zip(a[k].ravel(), b[k].ravel())) < scale * mpmath.mpf(10) ** -45
        assert a["cost"] == b["cost"]
    d = bl.linearise(*args)
    assert d["S"].shape == (12 + 24, 12 + 24) and max(bl.rel_errors(d, a)) < 1e-12


# ----------------------------------------------------------------------------------------------------------------- undistortion
def test_reference_undistortion_inverts_the_lens_over_the_whole_picture():
    from mocap_core import synth
    K = np.array(synth.DEFAULT_K)
    u, v = np.meshgrid(np.arange(320.0), np.arange(320.0))
    raw = np.stack(synth.distort_pixels(u.ravel(), v.ravel(), K, synth.REFERENCE_DISTORTION), axis=1)[:, None, :]
    back = bl.undistort(raw, K[None], np.array([synth.REFERENCE_DISTORTION]))
    err = np.abs(back[:, 0] - np.stack([u.ravel(), v.ravel()], axis=1)).max()
    print(f"round trip over 320 x 320 at REFERENCE_DISTORTION, {bl.NEWTON} Newton steps: {err:.2e} px")
    assert err < 1e-10          # 3e-13 px measured; a pixel coordinate of 320 carries 6e-14
    raw[7, 0, 1] = np.nan
    assert np.isnan(bl.undistort(raw, K[None], np.array([synth.REFERENCE_DISTORTION]))[7]).all()
    same = bl.undistort(raw, K[None], np.zeros((1, 5)))
    assert same[:7].tobytes() == raw[:7].tobytes() and same[8:].tobytes() == raw[8:].tobytes()


# ----------------------------------------------------------------------------------------------------------------------- loop
def test_reference_recovers_planted_lenses_and_poses_on_exact_data():
    rig, obs, X0, start = bl.planted_case(4, 200)
    assert bl.pose_errors(start["R"], start["t"], rig)[0] > 1e-2 and bl.lens_errors(start["K"], start["dist"], rig)[1] > 5.0
    R, t, K, d, X, info = bl.solve(obs, start["R"], start["t"], start["K"], start["dist"], flags=bl.ALL)
    rot, tr = bl.pose_errors(R, t, rig)
    f, c, k1 = bl.lens_errors(K, d, rig)
    print(f"rotation {rot:.2e} rad, translation {tr:.2e} |t1|, focal {f:.2e}, centre {c:.2e} px, k1 {k1:.2e}, all of dist "
          f"{np.abs(d - rig['dist']).max():.2e}; {info['accepted']} accepted of {info['passes']} passes")
    assert rot <= CAP and tr <= CAP and f <= CAP and c <= CAP * 320 and np.abs(d - rig["dist"]).max() <= CAP
    part = ~np.isnan(X[:, 0])
    assert part.sum() == info["participating"] and np.array_equal(part, (~np.isnan(obs[..., 0])).sum(axis=1) >= 2)
    k = np.linalg.norm(rig["t"][1]) / np.linalg.norm(t[1])
    assert np.abs(X[part] * k - X0[part]).max() <= CAP * np.linalg.norm(rig["t"][1])
    assert np.array_equal(R[0], start["R"][0]) and np.array_equal(t[0], start["t"][0])
    assert abs(np.linalg.norm(t[1]) - np.linalg.norm(start["t"][1])) <= 4 * np.spacing(np.linalg.norm(start["t"][1]))
    assert (d[:, 4] == 0).all()


def test_reference_on_a_noisy_capture_for_the_record():
    """0.3 px noise, 300 points that fill the images: what the full model is worth against poses alone with no lens in the model."""
    rig, obs, _, start = bl.planted_case(4, 300, noise_px=0.3)
    full = bl.solve(obs, start["R"], start["t"], start["K"], start["dist"], flags=bl.ALL)
    none = bl.solve(obs, start["R"], start["t"], start["K"], start["dist"], flags=0)
    e_full, e_none = bl.pose_errors(full[0], full[1], rig), bl.pose_errors(none[0], none[1], rig)
    f, c, k1 = bl.lens_errors(full[2], full[3], rig)
    print(f"all flags: rotation {e_full[0] * 1e3:.1f} mrad, focal {f * 100:.2f} %, centre {c:.2f} px, k1 {k1:.3f}; no lens in the model: "
          f"rotation {e_none[0] * 1e3:.1f} mrad; cost {full[5]['cost0']:.0f} -> {full[5]['cost']:.1f} against {none[5]['cost']:.1f}")
    assert full[5]["cost"] < none[5]["cost"] < full[5]["cost0"]
    assert all(b < a for a, b in zip([full[5]["cost0"]] + full[5]["costs"], full[5]["costs"]))
    assert e_full[0] < e_none[0]
