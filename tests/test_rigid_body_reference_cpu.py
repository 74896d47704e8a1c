"""The rigid-body contract (include/mocap_core.h, "rigid bodies") as tests/rigid_body_reference.py states it, without a GPU:
the reference recovers planted assignments and poses, posability and the MOCAP_E_ARG rules behave as the header says, the
header's constants are the binding's, the library exports the new entry points, and the two routes to the pose agree."""
import os
import re

import numpy as np
import pytest

import rigid_body_reference as rb
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mocap_core.h")
NEW_SYMBOLS = ("mocap_set_rigid_bodies", "mocap_locate_rigid_bodies", "mocap_locate_rigid_bodies_dev", "mocap_track_frame_bodies",
               "mocap_track_frame_bodies_dev")
TOL, MAX_RMS = 0.01, 0.005


@pytest.fixture(scope="module")
def planted_runs():
    """Two bodies of 4 and 5 markers, 12 clutter points in a 2 m cube, 0.5 mm noise, one marker hidden in half the trials."""
    rng = np.random.default_rng(20)
    bodies = [rb.make_body(rng, 4), rb.make_body(rng, 5)]
    models = [rb.Model(b) for b in bodies]
    runs = []
    for trial in range(40):
        hide = [(int(rng.integers(0, 4)),), (int(rng.integers(0, 5)),)] if trial % 2 else []
        pts, n, planted = rb.make_scene(rng, bodies, 32, 12, hide=hide)
        runs.append((pts, n, planted, rb.locate(pts, n, models, TOL, MAX_RMS)))
    return models, runs


def test_reference_recovers_planted_assignments_and_poses(planted_runs):
    models, runs = planted_runs
    nodes = 0
    for pts, n, planted, res in runs:
        claimed = set()
        for b, model in enumerate(models):
            r, p = res[b], planted[b]
            assert r["found"] == 1 and r["status"] == 0
            assert r["assign"][:model.n] == p["assign"] and r["assign"][model.n:] == [-1] * (8 - model.n)
            assert r["n_used"] == sum(a >= 0 for a in p["assign"])
            used = [m for m in range(model.n) if p["assign"][m] >= 0]
            assert not claimed & {p["assign"][m] for m in used}
            claimed |= {p["assign"][m] for m in used}
            # the fitted pose reproduces the planted markers to the noise level; R is a proper rotation
            fit = (r["R"] @ model.q[used].T).T + r["t"]
            truth = (p["R"] @ model.q[used].T).T + p["t"]
            assert np.abs(fit - truth).max() < 0.003
            assert np.abs(r["R"].T @ r["R"] - np.eye(3)).max() < 1e-14 and np.linalg.det(r["R"]) > 0
            assert 0 < r["rms"] < 0.003 and r["score"] >= 0
            assert r["best"] < r["runner_up"] if r["runner_up"] is not None else True
            nodes = max(nodes, rb.search(pts[:n], model, TOL)["nodes"])
    assert nodes < 5000          # the exhaustive recursion is cheap at test sizes


def test_pruned_walk_finds_the_exhaustive_optimum_and_counts_its_extensions(planted_runs):
    models, runs = planted_runs
    for pts, n, planted, res in runs[:10]:
        for model in models:
            ext, best = rb.count_extensions(pts[:n], model, TOL)
            assert best == rb.search(pts[:n], model, TOL)["best"]
            assert ext >= 3                               # a found body took at least three extensions
            capped, _ = rb.count_extensions(pts[:n], model, TOL, cap=1)
            assert capped == 2                            # ... so a cap of one stops the walk at the second


def test_horn_and_kabsch_agree(planted_runs):
    models, runs = planted_runs
    worst = 0.0
    for pts, n, planted, res in runs:
        for b, model in enumerate(models):
            a = res[b]["assign"]
            used = [m for m in range(model.n) if a[m] >= 0]
            Q, P = model.q[used], pts[[a[m] for m in used]]
            Rk, tk, rk = rb.kabsch(Q, P)
            Rh, th, rh = rb.horn(Q, P)
            worst = max(worst, np.abs(Rk - Rh).max(), np.abs(tk - th).max(), abs(rk - rh))
    assert worst < 1e-12, worst


def test_fifty_digit_pose_agrees_with_float64():
    rng = np.random.default_rng(3)
    q = rb.make_body(rng, 6)
    R, t = rb.random_rotation(rng), np.array([0.4, -1.2, 0.8])
    P = (R @ q.T).T + t + rng.normal(0, 0.0005, (6, 3))
    ref = rb.pose_mp(q, P)
    for fn in (rb.kabsch, rb.horn):
        dR, dt, dr = rb.pose_errors(*fn(q, P), ref)
        assert dR < 1e-13 and dt < 1e-13 and dr < 1e-14, (fn.__name__, dR, dt, dr)
    # an exact copy: the 50-digit pose is the planted one and rms is zero to the inputs' rounding
    P0 = (R @ q.T).T + t
    R0, t0, r0 = rb.pose_mp(q, P0)
    assert max(abs(float(R0[i][j]) - R[i, j]) for i in range(3) for j in range(3)) < 1e-14 and float(r0) < 1e-15


def test_posability():
    line = [[0.1 * i, 0, 0] for i in range(4)]
    assert not any(rb.posable_table(line))
    tri = [[0, 0, 0], [0.2, 0, 0], [0, 0.1, 0]]
    tab = rb.posable_table(tri)
    assert tab == [False] * 7 + [True]
    # three collinear markers and one off the line: every subset with the off-line marker and two others is posable
    body = [[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0, 0.15, 0]]
    tab = rb.posable_table(body)
    for s in range(16):
        want = bin(s).count("1") >= 3 and bool(s & 8)
        assert tab[s] == want, s
    # the threshold: sin of the angle at marker i between the two edges, 0.1
    for ang, want in ((0.09, False), (0.11, True)):
        thin = [[0, 0, 0], [1, 0, 0], [np.cos(ang), np.sin(ang), 0]]
        # (the triple is tested at i = 0 only: the lowest marker of the triple is the apex)
        assert rb.triple_spans(*thin) == want
    assert rb.posable_table([[0, 0, 0], [1, 0, 0], [2, 0.05, 0]])[7] is False


def test_e_arg_rules():
    rng = np.random.default_rng(5)
    good = rb.make_body(rng, 4)
    assert rb.validate([good], TOL, MAX_RMS) is None
    assert rb.validate([], TOL, MAX_RMS) is None                       # B = 0 clears
    assert rb.validate([good] * 8, TOL, MAX_RMS) is None
    assert rb.validate([good] * 9, TOL, MAX_RMS) is not None           # B > 8
    assert rb.validate([good[:2]], TOL, MAX_RMS) is not None           # fewer than 3 markers
    assert rb.validate([rb.make_body(rng, 8)], TOL, MAX_RMS) is None
    assert rb.validate([np.vstack([rb.make_body(rng, 8), [[1, 1, 1]]])], TOL, MAX_RMS) is not None   # more than 8
    bad = good.copy()
    bad[1, 2] = np.inf
    assert rb.validate([bad], TOL, MAX_RMS) is not None                # non-finite coordinate
    close = good.copy()
    close[1] = close[0] + [0.019, 0, 0]
    assert rb.validate([close], TOL, MAX_RMS) is not None              # two markers less than 2 tol apart
    close[1] = close[0] + [0.021, 0, 0]
    assert rb.validate([close], TOL, MAX_RMS) is None
    assert rb.validate([[[0.1 * i, 0, 0] for i in range(4)]], TOL, MAX_RMS) is not None   # collinear: not posable
    for tol, rms in ((0.0, MAX_RMS), (-1.0, MAX_RMS), (TOL, 0.0), (float("nan"), MAX_RMS)):
        assert rb.validate([good], tol, rms) is not None
    assert rb.validate([good, bad], TOL, MAX_RMS) is not None          # one bad body refuses the whole registration


def test_header_constants_match_the_binding_and_the_reference():
    from mocap_core import capi
    text = open(HEADER).read()
    macro = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))   # noqa: E731
    enum = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))        # noqa: E731
    assert macro("MOCAP_RB_MAX_BODIES") == capi.RB_MAX_BODIES == rb.MAX_BODIES == 8
    assert macro("MOCAP_RB_MAX_MARKERS") == capi.RB_MAX_MARKERS == rb.MAX_MARKERS == 8
    assert macro("MOCAP_RB_MAX_POINTS") == capi.RB_MAX_POINTS == rb.MAX_POINTS == 64
    assert macro("MOCAP_RB_DEFAULT_WORK_CAP") == capi.RB_DEFAULT_WORK_CAP == rb.DEFAULT_WORK_CAP
    assert enum("MOCAP_RB_ST_RMS") == capi.RB_ST_RMS == rb.ST_RMS
    assert enum("MOCAP_RB_ST_WORK_CAP") == capi.RB_ST_WORK_CAP == rb.ST_WORK_CAP


def test_header_declares_and_library_exports_the_entry_points():
    from mocap_core import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(mocap_[a-z_0-9]+)\s*\(", text))
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name) is not None
        # the binding passes as many arguments as the header declares
        proto = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(capi.SIGNATURES[name][1]) == proto.count(",") + 1, name
    for method in ("set_rigid_bodies", "locate_rigid_bodies", "locate_rigid_bodies_dev", "track_frame_bodies", "track_frame_bodies_dev"):
        assert callable(getattr(capi.MocapCore, method))
    from mocap_core import helpers
    for fn in ("set_rigid_bodies", "locate_rigid_bodies", "track_frame_bodies"):
        assert callable(getattr(helpers, fn))


def test_payload_gains_a_bodies_list_only_when_asked():
    from mocap_core import helpers
    base = helpers.object_points_payload([1.0], [[0.0, 0.0, 0.0]], [])
    assert "bodies" not in base
    body = {"name": "wand", "R": np.eye(3), "t": np.zeros(3), "rms": 0.001, "markers": [0, 2, -1]}
    got = helpers.object_points_payload([1.0], [[0.0, 0.0, 0.0]], [], bodies=[body])
    assert {k: v for k, v in got.items() if k != "bodies"} == base
    assert got["bodies"] == [{"name": "wand", "R": np.eye(3).tolist(), "t": [0.0, 0.0, 0.0], "rms": 0.001, "markers": [0, 2, -1]}]
