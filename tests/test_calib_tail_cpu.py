"""No GPU: the calibration tail's ABI surface, its fixture (tests/golden/calib_tail_session.npz, written by
scripts/make_calib_tail_golden.py from the reference's own `determine-scale`, `acquire-floor` and `set-origin` handlers) and
the two host-only entry points, mocap_floor_from_factor and mocap_world_set_origin, called with a NULL context.

Gate of the floor matrix, 1e-9 absolute per entry: the reference solves the plane with scipy.linalg.lstsq (gelsd), this code
back-substitutes a QR factor; both are backward stable, so the fits differ by O(cond * eps) ~ 1e-13 at cond([x y 1]) <= 1.1e3,
and the rotation is a smooth function of the fit at a 12 degree tilt (a NumPy emulation of a 64-row-block TSQR tree measured
<= 2.4e-15 on these inputs, a normal-equations sum 5e-13)."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import linalg

from conftest import PKG, ROOT, load_golden

SYMBOLS = ("mocap_determine_scale", "mocap_determine_scale_dev", "mocap_floor_factor", "mocap_floor_factor_dev",
           "mocap_floor_from_factor", "mocap_world_set_origin")
RECORDS = (0, 1)


@pytest.fixture(scope="module")
def golden():
    return load_golden("calib_tail_session")


def points_of(g, rec):
    xyz, n = g["xyz"][rec], g["n_pts"][rec]
    return xyz[np.arange(xyz.shape[1])[None, :] < n[:, None]]


def factor_of(pts):
    """np.linalg.qr of [x y 1 | z], diagonal made non-negative, then the point count: mocap_floor_factor's output layout."""
    A = np.c_[pts[:, 0], pts[:, 1], np.ones(len(pts)), pts[:, 2]]
    R = np.linalg.qr(A, mode="r")
    if R.shape[0] < 4:
        R = np.vstack([R, np.zeros((4 - R.shape[0], 4))])
    sign = np.where(np.diag(R) < 0, -1.0, 1.0)
    return np.r_[(R * sign[:, None]).ravel(), float(len(pts))]


def test_header_declares_and_library_exports_the_calibration_tail():
    header = open(os.path.join(ROOT, "include", "mocap_core.h")).read()
    from mocap_core import capi
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(mocap_ctx\* ctx," % name, header), name
        assert name in capi.SIGNATURES, name
    assert "mocap_floor_from_factor(mocap_ctx* ctx, const double* factor, double* to_world, double* info)" in header
    lib = os.path.join(PKG, "lib", "libmocap_core.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name


def test_fixture_satisfies_the_generators_conditions(golden):
    g = golden
    assert g["xyz"].shape == (2, 300, 8, 3) and g["n_pts"].shape == (2, 300)
    assert g["n_pts"].min() == 0 and g["n_pts"].max() == 4
    for rec, (offset, cond_lo, cond_hi) in enumerate((((2.0, -1.5, 0.7), 5.0, 30.0), ((20.0, -15.0, 3.0), 1.0e3, 1.25e3))):
        n = g["n_pts"][rec]
        assert (n == 2).sum() >= 60
        valid = np.arange(8)[None, :] < n[:, None]
        assert np.isnan(g["xyz"][rec][~valid]).all() and np.isfinite(g["xyz"][rec][valid]).all()
        pts = points_of(g, rec)
        assert np.abs(pts.mean(axis=0) - offset).max() < 0.15
        pair = g["xyz"][rec][n == 2]
        d = np.sqrt(np.sum((pair[:, 0] - pair[:, 1]) ** 2, axis=1))
        assert np.abs(d - 0.4).max() < 0.02
        fit = np.asarray(linalg.lstsq(np.c_[pts[:, :2], np.ones(len(pts))], pts[:, 2])[0])
        tilt = np.degrees(np.arctan(np.hypot(fit[0], fit[1])))
        assert 2.0 <= tilt and abs(tilt - 12.0) < 0.5, tilt
        cond = np.linalg.cond(np.c_[pts[:, :2], np.ones(len(pts))])
        assert cond_lo < cond < cond_hi, cond                      # record 1: about 1.1e3
        assert (np.abs(g["pose_t"][rec]) > 0).all() and g["pose_t"][rec][1, 0] == 1.0
        assert not np.array_equal(g["floor_to_world"][rec], np.eye(4))
        # the emitted payloads are the handler's expressions on these inputs
        scale = 0.15 / np.mean(d)
        assert g["scaled_t"][rec][1, 0] == scale
        assert np.array_equal(g["scaled_t"][rec], g["pose_t"][rec] * scale)


@pytest.mark.parametrize("rec", RECORDS)
def test_floor_from_factor_reproduces_the_reference(golden, rec):
    from mocap_core import capi
    pts = points_of(golden, rec)
    W, info, rc = capi.floor_from_factor(factor_of(pts))
    assert rc == capi.MOCAP_OK
    err = np.abs(W - golden["floor_to_world"][rec]).max()
    A = np.c_[pts[:, :2], np.ones(len(pts))]
    fit, res = linalg.lstsq(A, pts[:, 2])[:2]
    got = np.array([info["a"], info["b"], info["c"]])
    rel = np.abs(got - fit) / np.abs(fit)
    rms = np.sqrt(np.sum((A @ fit - pts[:, 2]) ** 2) / len(pts))
    print(f"record {rec}: to_world {err:.3e} (gate 1e-9)  fit {rel.max():.3e} (gate 1e-10)  rms {info['rms_residual']:.6e} vs {rms:.6e}")
    assert err <= 1e-9
    assert (rel <= 1e-10).all()
    assert info["points"] == len(pts)
    assert abs(info["rms_residual"] - rms) <= 1e-9 * rms
    assert abs(info["tilt"] - np.arctan(np.hypot(fit[0], fit[1]))) <= 1e-10


@pytest.mark.parametrize("rec", RECORDS)
def test_world_set_origin_is_bit_exact(golden, rec):
    """T(-p) @ to_world: every product in an entry's sum is exact (a factor is 0 or 1, or the matrix's last row is (0, 0, 0, 1)),
    so neither the order of the sum nor a fused multiply-add in NumPy's matmul can change a bit."""
    from mocap_core import capi
    W = capi.world_set_origin(golden["floor_to_world"][rec], golden["origin_point"][rec])
    assert W.tobytes() == golden["origin_to_world"][rec].tobytes()
    p = golden["origin_point"][rec]
    assert np.array_equal(W[:3, 3], -p[[0, 2, 1]])            # y and z swapped (index.py:204)


def test_degenerate_inputs(golden):
    from mocap_core import capi
    pts = points_of(golden, 0)
    with pytest.raises(capi.MocapError) as e:                   # 2 points
        capi.floor_from_factor(factor_of(pts[:2]))
    assert e.value.code == capi.MOCAP_E_ARG
    t = np.arange(50.0)
    line = np.c_[0.25 * t + 2.0, 0.5 * t - 1.5, np.sin(t)]      # collinear in (x, y)
    with pytest.raises(capi.MocapError) as e:
        capi.floor_from_factor(factor_of(line))
    assert e.value.code == capi.MOCAP_E_ARG
    rng = np.random.default_rng(3)
    flat = np.c_[rng.integers(-8, 9, (40, 2)) / 4.0, np.full(40, 0.75)]   # exactly horizontal: z = 0.75
    W, info, rc = capi.floor_from_factor(factor_of(flat))
    assert rc == capi.MOCAP_E_NOCONV
    assert abs(info["a"]) < 1e-12 and abs(info["b"]) < 1e-12 and abs(info["c"] - 0.75) < 1e-12 and info["points"] == 40
    assert np.array_equal(W[3], [0, 0, 0, 1]) and np.array_equal(W[:3, 3], [0, 0, 0])   # the matrix was written
