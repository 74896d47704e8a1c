"""The statement of "predicted precision" (tests/precision_reference.py, the NumPy text the GPU results are compared with bit for
bit) checked on the CPU: against a 50-digit evaluation with an exact eigen-decomposition, against the textbook stereo case in closed
form, against what a least-squares triangulation actually scatters under pixel noise, and under a change of the caller's
coordinates; the rules of refusal; and the seven symbols' declaration, export and binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import precision_reference as pr
from conftest import ROOT
from mocap_core import synth

INF, NAN = float("inf"), float("nan")

# Measured on the cases of test_statement_against_50_digits (the largest relative error over all OK points; cov relative to the
# point's largest covariance entry, axis absolute on a unit vector):  sig 9.1e-16, cov 2.6e-15, axis 5.2e-14 over 305 points -- the
# axis of a nearly round ellipsoid (two close eigenvalues) is the least determined.  The assertion stands at 100 x the measured figure.
MEASURED = {"sig": 9.1e-16, "cov": 2.6e-15, "axis": 5.2e-14}


def _errors(Pp, x, res):
    e = {"sig": 0.0, "cov": 0.0, "axis": 0.0}
    n = 0
    for i in np.nonzero(res["info"] == pr.OK)[0]:
        views = [c for c in range(Pp.shape[0]) if (int(res["seen"][i]) >> c) & 1]
        sig, axis, cov = pr.exact(Pp, x[i], views, 0.5)
        e["sig"] = max(e["sig"], max(abs(float((res["sig"][i, k] - sig[k]) / sig[k])) for k in range(3)))
        top = max(abs(c) for c in cov)
        e["cov"] = max(e["cov"], max(abs(float((res["cov"][i, k] - cov[k]) / top)) for k in range(6)))
        e["axis"] = max(e["axis"], max(abs(float(res["axis"][i, k] - axis[k])) for k in range(3)))
        n += 1
    return e, n


def test_statement_against_50_digits():
    worst = {"sig": 0.0, "cov": 0.0, "axis": 0.0}
    total = 0
    for C, N in ((2, 70), (3, 70), (8, 60)):
        rig = synth.calibrated_ring_rig(C, seed=3)
        P = pr.camera_table(rig["K"], rig["R"], rig["t"])
        rng = np.random.default_rng(20 + C)
        x = rig["centre"][None] + rng.uniform(-0.8, 0.8, (N, 3))
        seen = np.full(N, (1 << C) - 1, dtype=np.uint64)
        if C == 8:
            seen[::2] = rng.integers(3, 256, len(seen[::2]), dtype=np.uint64) | np.uint64(3)
        res = pr.point_precision(P, x, seen=seen, sigma_px=0.5)
        e, n = _errors(P, x, res)
        assert n == N
        total += n
        worst = {k: max(worst[k], e[k]) for k in worst}
    rig = synth.calibrated_ring_rig(8, seed=3)
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    step = np.array([0.4, 0.4, 0.5])
    grid = (rig["centre"] - step * [3, 2, 1], [step[0], 0, 0], [0, step[1], 0], [0, 0, step[2]])
    x = pr.grid_points((7, 5, 3), *grid)
    res = pr.evaluate(P, x, 0.5, vis=(*rig["image_size"], 0.1, 10.0))
    e, n = _errors(P, x, res)
    assert n >= 90
    total += n
    worst = {k: max(worst[k], e[k]) for k in worst}
    print("predicted precision, statement against 50 digits over %d points: %s" % (total, worst))
    assert total >= 290
    for k in worst:
        assert worst[k] <= min(100.0 * MEASURED[k], 1e-8), (k, worst[k])


def test_textbook_stereo_case_in_closed_form():
    for f, b, z, sigma in ((500.0, 0.6, 3.0, 1.0), (1234.5, 0.25, 7.5, 0.3), (320.0, 2.0, 1.5, 2.0)):
        K = np.repeat(np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]])[None], 2, axis=0)
        R = np.stack([np.eye(3), np.eye(3)])
        t = np.array([[b / 2, 0, 0], [-b / 2, 0, 0]])          # centres at (-b/2, 0, 0) and (+b/2, 0, 0)
        res = pr.point_precision(pr.camera_table(K, R, t), np.array([[0.0, 0.0, z]]), seen=np.array([3], dtype=np.uint64), sigma_px=sigma)
        assert res["info"][0] == pr.OK and res["n_views"][0] == 2
        lateral, depth = sigma * z / (f * np.sqrt(2.0)), sigma * np.sqrt(2.0) * z * z / (f * b)
        assert np.allclose(res["sig"][0], [lateral, lateral, depth], rtol=1e-12, atol=0)
        assert np.allclose(res["axis"][0], [0.0, 0.0, 1.0], rtol=0, atol=1e-12)
        assert np.allclose(res["cov"][0], [lateral ** 2, 0, 0, lateral ** 2, 0, depth ** 2], rtol=1e-12, atol=1e-12 * depth ** 2)


def _gauss_newton(P, obs, X0, steps=8):
    """An independent least-squares triangulation: obs [S][C][2], all cameras, S samples at once."""
    X = np.repeat(X0[None], obs.shape[0], axis=0)
    for _ in range(steps):
        h = np.einsum("cij,sj->sci", P[:, :, :3], X) + P[None, :, :, 3]            # [S][C][3]
        proj = h[:, :, :2] / h[:, :, 2:3]
        r = (proj - obs).reshape(obs.shape[0], -1)                                   # [S][2C]
        J = (P[None, :, :2, :3] - proj[:, :, :, None] * P[None, :, 2:3, :3]) / h[:, :, 2:3, None]   # [S][C][2][3]
        J = J.reshape(obs.shape[0], -1, 3)
        X = X - np.linalg.solve(np.einsum("ski,skj->sij", J, J), np.einsum("ski,sk->si", J, r)[..., None])[..., 0]
    return X


def test_the_prediction_is_a_prediction():
    rig = synth.calibrated_ring_rig(8, seed=5)
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    X0 = rig["centre"] + np.array([0.3, -0.2, 0.25])
    sigma, S = 0.5, 20000
    res = pr.point_precision(P, X0[None], seen=np.array([255], dtype=np.uint64), sigma_px=sigma)
    assert res["info"][0] == pr.OK
    h = np.einsum("cij,j->ci", P[:, :, :3], X0) + P[:, :, 3]
    assert res["sig"][0, 2] / h[:, 2].min() < 1e-2            # the linearisation's own bias is far below the tolerance
    rng = np.random.default_rng(12345)
    obs = (h[:, :2] / h[:, 2:3])[None] + sigma * rng.standard_normal((S, 8, 2))
    X = _gauss_newton(P, obs, X0)
    c = res["cov"][0]
    cov = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    lam, vec = np.linalg.eigh(cov)
    assert np.allclose(np.sqrt(lam), res["sig"][0], rtol=1e-9)
    assert abs(abs(vec[:, 2] @ res["axis"][0]) - 1.0) < 1e-9
    d = X - X.mean(axis=0)
    for k in range(3):
        ratio = np.var(d @ vec[:, k], ddof=1) / lam[k]
        print("principal axis %d: sample variance / predicted = %.4f" % (k, ratio))
        assert abs(ratio - 1.0) <= 0.06                      # six standard deviations of sqrt(2 / (S - 1))


def test_frame_folding():
    rig = synth.calibrated_ring_rig(3, seed=3)
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    rng = np.random.default_rng(8)
    X = rig["centre"][None] + rng.uniform(-0.7, 0.7, (50, 3))
    seen = np.full(50, 7, dtype=np.uint64)
    plain = pr.point_precision(P, X, seen=seen, sigma_px=0.8)
    for scale in (1.0, 0.001, 39.37):
        Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        a = rng.standard_normal(3)
        frame = np.concatenate([scale * Q, a[:, None]], axis=1)            # X = scale Q x + a
        x = (X - a) @ Q / scale
        res = pr.point_precision(P, x, seen=seen, sigma_px=0.8, frame=frame)
        assert (res["info"] == pr.OK).all()
        print("frame folding at scale %g: sig differs by %.2e relative" % (scale, np.abs(res["sig"] * scale / plain["sig"] - 1.0).max()))
        assert np.allclose(res["sig"] * scale, plain["sig"], rtol=1e-12, atol=0)
        worst = np.abs(np.einsum("ni,ij->nj", plain["axis"], Q) * np.sign(np.einsum("ni,ij,nj->n", plain["axis"], Q, res["axis"]))[:, None] - res["axis"]).max()
        assert worst < 1e-9
    null = pr.point_precision(P, X, seen=seen, sigma_px=0.8, frame=None)
    ident = pr.point_precision(P, X, seen=seen, sigma_px=0.8, frame=np.eye(3, 4))
    for k in ("cov", "sig", "axis", "n_views", "info"):
        assert null[k].tobytes() == ident[k].tobytes(), k


def test_every_refused_rule():
    ident = np.eye(3, 4)
    assert pr.validate_common(1.0, None) is None and pr.validate_common(5e-324, ident) is None
    for s in (0.0, -1.0, NAN, INF, -INF):
        assert pr.validate_common(s, None)
    for i in range(12):
        for v in (NAN, INF, -INF):
            f = ident.copy().reshape(-1)
            f[i] = v
            assert pr.validate_common(1.0, f)
    assert pr.validate_vis(1, 1, 0.0, INF) is None and pr.validate_vis(640, 480, 0.5, 0.5000001) is None
    for w, h, near, far in ((0, 480, 0.0, 1.0), (640, 0, 0.0, 1.0), (640, 480, -1e-300, 1.0), (640, 480, NAN, 1.0), (640, 480, INF, INF),
                            (640, 480, 1.0, 1.0), (640, 480, 2.0, 1.0), (640, 480, 0.0, NAN)):
        assert pr.validate_vis(w, h, near, far), (w, h, near, far)
    assert pr.validate_points(1) is None and pr.validate_points(pr.MAX_POINTS) is None
    assert pr.validate_points(0) and pr.validate_points(-3) and pr.validate_points(pr.MAX_POINTS + 1)
    assert pr.validate_frames(0, 1) is None and pr.validate_frames(pr.MAX_POINTS // 16, 16) is None
    assert pr.validate_frames(-1, 4) and pr.validate_frames(4, 0) and pr.validate_frames(pr.MAX_POINTS // 16 + 1, 16)
    assert pr.validate_map(1, 1, 1, 0, INF) is None and pr.validate_map(1024, 1024, 128, 65, 0.0) is None
    for nx, ny, nz, mv, ms in ((0, 1, 1, 2, 1.0), (1, 0, 1, 2, 1.0), (1, 1, 0, 2, 1.0), (1025, 1, 1, 2, 1.0), (1, 1025, 1, 2, 1.0), (1, 1, 1025, 2, 1.0),
                               (1024, 1024, 129, 2, 1.0), (4, 4, 4, -1, 1.0), (4, 4, 4, 2, NAN)):
        assert pr.validate_map(nx, ny, nz, mv, ms), (nx, ny, nz, mv, ms)
    # the helpers' world transform: affine and invertible, or ValueError
    from mocap_core import helpers
    T = np.array([[0.0, 2.0, 0.0, 0.3], [0.0, 0.0, 2.0, -0.2], [2.0, 0.0, 0.0, 1.1], [0.0, 0.0, 0.0, 2.0]])
    assert np.allclose(helpers.precision_frame(T), pr.world_frame(T), rtol=1e-13, atol=1e-13)
    Xc = np.array([0.2, -0.4, 3.0])
    hom = T @ np.array([-Xc[0], -Xc[1], Xc[2], 1.0])
    xw = (hom[:3] / hom[3])[[0, 2, 1]]
    frame = helpers.precision_frame(T)
    assert np.allclose(frame[:, :3] @ xw + frame[:, 3], Xc, rtol=1e-13, atol=1e-13)
    assert helpers.precision_frame(None) is None or helpers._state["to_world"] is not None
    for bad in (np.diag([1.0, 1.0, 1.0, 0.0]), np.diag([1.0, 0.0, 1.0, 1.0]), np.eye(4) + np.eye(4)[[3, 0, 1, 2]] * 0.5, np.full((4, 4), NAN)):
        for fn in (helpers.precision_frame, pr.world_frame):
            with pytest.raises(ValueError):
                fn(bad)


def test_the_seven_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    n_args = {"mocap_point_precision": 15, "mocap_point_precision_dev": 15, "mocap_frame_precision": 14, "mocap_frame_precision_dev": 14,
              "mocap_coverage_map": 20, "mocap_coverage_map_dev": 20, "mocap_precision_limits": 3}
    for n, count in n_args.items():
        assert re.search(r"\b(int|void) %s\s*\(" % n, header), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) == count
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % n, header).group(1)
        assert decl.count(",") + 1 == count, n
        if n != "mocap_precision_limits":
            assert callable(getattr(capi.MocapCore, n[len("mocap_"):]))
    for name, value in (("MAX_POINTS", 1 << 24), ("MAX_VOXELS", 1 << 27), ("MAX_DIM", 1024), ("SUMMARY", 72), ("SWEEPS", 16)):
        assert "#define MOCAP_PM_%s %d" % (name, value) in header and getattr(capi, "PM_" + name) == value == getattr(pr, name)
    for name in ("OK", "BAD_POINT", "BAD_VIEW", "FEW_VIEWS", "DEGENERATE"):
        assert re.search(r"MOCAP_PM_%s = %d\b" % (name, getattr(capi, "PM_" + name)), header) and getattr(capi, "PM_" + name) == getattr(pr, name)
    assert capi.MocapCore.PRECISION_OUT == ("cov", "sig", "axis", "n_views", "info")
