"""The rigid-body stage on the GPU (csrc/rigid_body.hip, include/mocap_core.h "rigid bodies") against the plain statement of
its contract in tests/rigid_body_reference.py: assignments, claiming, occlusion, ties, the mirror and work-cap flags exactly;
scores to 1e-12; poses against a 50-digit evaluation on the GPU's own assignment; determinism; the live path."""
import numpy as np
import pytest

import rigid_body_reference as rb

pytestmark = pytest.mark.gpu

TOL, MAX_RMS = 0.01, 0.005
OUT_KEYS = ("found", "n_used", "assign", "R", "t", "rms", "score", "rb_status")


# ---------------------------------------------------------------- scenes (built without a GPU; the reference runs once per module)
def _frames(rng, bodies, K_max, n_frames, n_total=None, n_clutter=None, hide_every=2):
    """Planted frames: every body present; in every hide_every-th frame one marker of each body is hidden.  n_total fixes the
    number of points (clutter fills up), else n_clutter clutter points are added."""
    out = []
    for f in range(n_frames):
        hide = [(int(rng.integers(0, len(q))),) if len(q) > 3 else () for q in bodies] if (hide_every and f % hide_every == 1) else []
        visible = sum(len(q) for q in bodies) - sum(len(h) for h in hide)
        clutter = n_total - visible if n_total is not None else n_clutter
        pts, n, planted = rb.make_scene(rng, bodies, K_max, clutter, hide=hide)
        out.append((pts, n, planted))
    return out


def build_cases():
    """name -> (bodies, K_max, [(points [K_max][3], n, planted)]).  The shapes the contract's paths turn on: a wave with idle
    lanes (K_max = 32, about 20 points), every lane live (64 of 64), frames of 0 .. 3 points, one 3-marker body, 4 / 5 / 8
    markers, eight bodies."""
    cases = {}
    rng = np.random.default_rng(101)
    bodies = [rb.make_body(rng, 4), rb.make_body(rng, 5)]
    cases["k32_b2"] = (bodies, 32, _frames(rng, bodies, 32, 24, n_clutter=12))
    rng = np.random.default_rng(102)
    bodies = [rb.make_body(rng, 4), rb.make_body(rng, 5), rb.make_body(rng, 8)]
    cases["k64_full_b3"] = (bodies, 64, _frames(rng, bodies, 64, 8, n_total=64))
    rng = np.random.default_rng(103)
    bodies = [rb.make_body(rng, 3)]
    frames = []
    for n in (0, 1, 2):                                   # clutter only: the body is hidden altogether
        frames.append(rb.make_scene(rng, bodies, 8, n, hide=[(0, 1, 2)]))
    frames.append(rb.make_scene(rng, bodies, 8, 0))       # exactly the body's three markers
    frames.append(rb.make_scene(rng, bodies, 8, 5))       # a full frame of 8
    frames.append(rb.make_scene(rng, bodies, 8, 2, hide=[(1,)]))   # two of three markers: not found
    cases["k8_b1_n3"] = (bodies, 8, frames)
    rng = np.random.default_rng(104)
    bodies = [rb.make_body(rng, 3 + b % 3) for b in range(8)]
    cases["k64_b8"] = (bodies, 64, _frames(rng, bodies, 64, 4, n_clutter=10, hide_every=0))
    return cases


def reference_results(case, work_cap=rb.DEFAULT_WORK_CAP, with_runner_up=True):
    bodies, K_max, frames = case
    models = [rb.Model(q) for q in bodies]
    return [rb.locate(pts, n, models, TOL, MAX_RMS, work_cap=work_cap, with_runner_up=with_runner_up) for pts, n, _ in frames]


def batch(case):
    bodies, K_max, frames = case
    xyz = np.stack([pts for pts, _, _ in frames])
    n_pts = np.array([n for _, n, _ in frames], dtype=np.int32)
    return xyz, n_pts


@pytest.fixture(scope="module")
def cases():
    c = build_cases()
    return {name: (case, reference_results(case)) for name, case in c.items()}


@pytest.fixture()
def rcore(core):
    core.set_world_transform(None)
    yield core
    core.set_rigid_bodies([])


def check_against_reference(got, ref, default_cap=True):
    """found, n_used, assign and status exactly; score to 1e-12 relative; the entries of an unfound body zero."""
    F = len(ref)
    for f in range(F):
        for b, r in enumerate(ref[f]):
            where = (f, b)
            assert got["found"][f, b] == r["found"], where
            assert got["rb_status"][f, b] == r["status"], where
            assert got["n_used"][f, b] == r["n_used"], where
            assert got["assign"][f, b].tolist() == list(r["assign"]), where
            if default_cap:
                assert not got["rb_status"][f, b] & rb.ST_WORK_CAP, where
            if r["found"]:
                assert abs(got["score"][f, b] - r["score"]) <= 1e-12 * r["score"], (where, got["score"][f, b], r["score"])
            else:
                for k in ("R", "t", "rms", "score"):
                    assert not np.any(got[k][f, b]), (where, k)


# ---------------------------------------------------------------- 1. planted scenes
@pytest.mark.parametrize("name", ["k32_b2", "k64_full_b3", "k8_b1_n3", "k64_b8"])
def test_planted_scenes_equal_the_reference(rcore, cases, name):
    (bodies, K_max, frames), ref = cases[name]
    # precondition, asserted on the reference: no winner whose runner-up has the same count and a score within 1e-9 relative
    for f, per_body in enumerate(ref):
        for b, r in enumerate(per_body):
            if r["best"] is not None and r["runner_up"] is not None and r["best"][0] == r["runner_up"][0]:
                assert r["runner_up"][1] - r["best"][1] > 1e-9 * r["runner_up"][1], (name, f, b, r["best"], r["runner_up"])
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS)
    xyz, n_pts = batch(cases[name][0])
    got = rcore.locate_rigid_bodies(xyz, n_pts)
    check_against_reference(got, ref)
    # the planted bodies are what is found (the frame that shows two of three markers aside)
    n_found = int(got["found"].sum())
    n_planted = sum(sum(a >= 0 for a in p["assign"]) >= 3 for _, _, planted in frames for p in planted)
    assert n_found == n_planted, (n_found, n_planted)
    for f, (_, _, planted) in enumerate(frames):
        for b, p in enumerate(planted):
            if got["found"][f, b]:
                assert got["assign"][f, b, :len(p["assign"])].tolist() == p["assign"], (f, b)


# ---------------------------------------------------------------- 2. exact tie
@pytest.mark.parametrize("dup_first", [False, True])
def test_exact_duplicate_point_the_smaller_index_wins(rcore, dup_first):
    rng = np.random.default_rng(7)
    q = rb.make_body(rng, 4)
    pts, n, planted = rb.make_scene(rng, [q], 16, 5)
    src = planted[0]["assign"][2]
    if dup_first:   # the copy goes in front of everything: shift the frame up by one slot
        pts = np.vstack([pts[src:src + 1], pts[:15]])
        n += 1
        want = 0
    else:
        pts[n] = pts[src]
        n += 1
        want = src
    assert sum(pts[k].tobytes() == pts[want].tobytes() for k in range(n)) == 2
    model = rb.Model(q)
    ref = rb.locate(pts, n, [model], TOL, MAX_RMS)
    assert ref[0]["found"] and ref[0]["runner_up"][:2] == ref[0]["best"][:2]      # the tie is exact in the reference
    rcore.set_rigid_bodies([q], tol=TOL, max_rms=MAX_RMS)
    got = rcore.locate_rigid_bodies(pts[None], [n])
    check_against_reference(got, [ref])
    assert got["assign"][0, 0, 2] == want


# ---------------------------------------------------------------- 3. occlusion and claiming
def test_hidden_markers_collinear_rest_and_identical_bodies(rcore):
    rng = np.random.default_rng(11)
    q5 = rb.make_body(rng, 5)
    m5 = rb.Model(q5)
    frames = []
    for hide in ((3,), (0, 4), (1, 2)):
        sub = sum(1 << m for m in range(5) if m not in hide)
        assert m5.posable[sub]
        frames.append(rb.make_scene(rng, [q5], 32, 10, hide=[hide]))
    rcore.set_rigid_bodies([q5], tol=TOL, max_rms=MAX_RMS)
    xyz, n_pts = np.stack([p for p, _, _ in frames]), [n for _, n, _ in frames]
    got = rcore.locate_rigid_bodies(xyz, n_pts)
    ref = [rb.locate(p, n, [m5], TOL, MAX_RMS) for p, n, _ in frames]
    check_against_reference(got, ref)
    assert got["found"][:, 0].tolist() == [1, 1, 1] and got["n_used"][:, 0].tolist() == [4, 3, 3]
    for f, (_, _, planted) in enumerate(frames):
        assert got["assign"][f, 0, :5].tolist() == planted[0]["assign"]

    # hidden down to a collinear subset: not found, status 0
    line = np.array([[0.0, 0, 0], [0.08, 0, 0], [0.2, 0, 0], [0.05, 0.12, 0.0], [0.1, -0.03, 0.15]])
    ml = rb.Model(line)
    assert ml.posable[31] and not ml.posable[7]
    pts, n, planted = rb.make_scene(rng, [line], 32, 10, hide=[(3, 4)])
    rcore.set_rigid_bodies([line], tol=TOL, max_rms=MAX_RMS)
    got = rcore.locate_rigid_bodies(pts[None], [n])
    ref = rb.locate(pts, n, [ml], TOL, MAX_RMS)
    check_against_reference(got, [ref])
    assert got["found"][0, 0] == 0 and got["rb_status"][0, 0] == 0

    # two identical bodies, two copies in the frame: body 0 takes the lexicographically first, body 1 the other
    pts, n, planted = rb.make_scene(rng, [q5, q5], 32, 10)
    rcore.set_rigid_bodies([q5, q5], tol=TOL, max_rms=MAX_RMS)
    got = rcore.locate_rigid_bodies(pts[None], [n])
    ref = rb.locate(pts, n, [m5, m5], TOL, MAX_RMS)
    check_against_reference(got, [ref])
    a0, a1 = got["assign"][0, 0, :5].tolist(), got["assign"][0, 1, :5].tolist()
    assert got["found"][0].tolist() == [1, 1] and not set(a0) & set(a1)
    both = sorted([planted[0]["assign"], planted[1]["assign"]])
    assert [a0, a1] == both


# ---------------------------------------------------------------- 4. pose accuracy on the GPU's own assignment
def test_pose_against_fifty_digits(rcore, cases):
    worst = {"gpu": [0.0, 0.0, 0.0], "kabsch": [0.0, 0.0, 0.0], "ratio": 0.0, "orth": 0.0}
    n_cases = 0
    for name in ("k32_b2", "k64_full_b3"):
        (bodies, K_max, frames), ref = cases[name]
        rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS)
        xyz, n_pts = batch(cases[name][0])
        got = rcore.locate_rigid_bodies(xyz, n_pts)
        for f in range(len(frames)):
            for b, q in enumerate(bodies):
                if not got["found"][f, b]:
                    continue
                a = got["assign"][f, b]
                used = [m for m in range(len(q)) if a[m] >= 0]
                Q, P = np.asarray(q)[used], xyz[f][[a[m] for m in used]]
                exact = rb.pose_mp(Q, P)
                d_ref = rb.pose_errors(*rb.kabsch(Q, P), exact)       # float64 NumPy Kabsch against the 50-digit values
                d_gpu = rb.pose_errors(got["R"][f, b], got["t"][f, b], got["rms"][f, b], exact)
                floor = 64 * np.spacing(max(1.0, float(np.abs(got["t"][f, b]).max())))
                R = got["R"][f, b]
                orth = np.abs(R.T @ R - np.eye(3)).max()
                for k in range(3):
                    worst["gpu"][k] = max(worst["gpu"][k], d_gpu[k])
                    worst["kabsch"][k] = max(worst["kabsch"][k], d_ref[k])
                    worst["ratio"] = max(worst["ratio"], d_gpu[k] / max(16 * d_ref[k], floor))
                worst["orth"] = max(worst["orth"], orth)
                n_cases += 1
                print(f"pose {name} f={f} b={b} n={len(used)}: gpu dR={d_gpu[0]:.2e} dt={d_gpu[1]:.2e} drms={d_gpu[2]:.2e} | "
                      f"kabsch dR={d_ref[0]:.2e} dt={d_ref[1]:.2e} drms={d_ref[2]:.2e} | |RtR-I|={orth:.2e}")
                for k, what in enumerate(("R", "t", "rms")):
                    assert d_gpu[k] <= max(16 * d_ref[k], floor), (name, f, b, what, d_gpu[k], d_ref[k], floor)
                assert orth <= 1e-14 and np.linalg.det(R) > 0, (name, f, b, orth)
    print(f"pose summary over {n_cases} cases: worst gpu (dR, dt, drms) = {worst['gpu']}, worst kabsch = {worst['kabsch']}, "
          f"worst error / bound = {worst['ratio']:.3f}, worst |RtR - I| = {worst['orth']:.2e}")
    assert n_cases >= 60


# ---------------------------------------------------------------- 5. mirror
def test_mirrored_body_is_rejected_on_rms_and_claims_nothing(rcore):
    rng = np.random.default_rng(13)
    chiral = np.array([[0.0, 0, 0], [0.2, 0, 0], [0, 0.15, 0], [0, 0, 0.1]])
    tri = chiral[:3]
    pts, n, planted = rb.make_scene(rng, [chiral * np.array([-1.0, 1, 1])], 16, 5)
    models = [rb.Model(chiral), rb.Model(tri)]
    ref = rb.locate(pts, n, models, TOL, MAX_RMS)
    assert ref[0]["status"] == rb.ST_RMS and ref[0]["best"][0] == -4 and ref[1]["found"]
    rcore.set_rigid_bodies([chiral, tri], tol=TOL, max_rms=MAX_RMS)
    got = rcore.locate_rigid_bodies(pts[None], [n])
    check_against_reference(got, [ref])
    assert got["found"][0].tolist() == [0, 1] and got["rb_status"][0].tolist() == [rb.ST_RMS, 0]
    # nothing was claimed: the triangle takes three of the very points the mirrored match sat on
    assert got["assign"][0, 1, :3].tolist() == planted[0]["assign"][:3]
    assert not got["assign"][0, 0].any() and not got["R"][0, 0].any()


# ---------------------------------------------------------------- 6. work cap
def test_work_cap(rcore, cases):
    (bodies, K_max, frames), ref = cases["k32_b2"]
    xyz, n_pts = batch(cases["k32_b2"][0])
    models = [rb.Model(q) for q in bodies]
    # cap 1: whatever the reference finds -- here every body searched over ALL the frame's points, since nothing is claimed --
    # is flagged; later bodies still see the points
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS, work_cap=1)
    got = rcore.locate_rigid_bodies(xyz, n_pts)
    flagged = 0
    for f, (pts, n, _) in enumerate(frames):
        for b, model in enumerate(models):
            alone = rb.locate(pts, n, [model], TOL, MAX_RMS, with_runner_up=False)[0]
            if alone["found"]:
                assert got["rb_status"][f, b] == rb.ST_WORK_CAP and got["found"][f, b] == 0, (f, b)
                flagged += 1
            assert got["found"][f, b] == 0 and not got["assign"][f, b].any() and not got["R"][f, b].any()
    assert flagged == 2 * len(frames)
    check_against_reference(got, reference_results(cases["k32_b2"][0], work_cap=1, with_runner_up=False), default_cap=False)
    # a cap in the middle of the batch's own extension counts: flagged exactly where the documented walk needs more
    ext = sorted(r["extensions"] for per_body in ref for r in per_body)
    mid = ext[len(ext) // 2]
    assert ext[0] <= mid < ext[-1]
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS, work_cap=mid)
    got = rcore.locate_rigid_bodies(xyz, n_pts)
    ref_mid = reference_results(cases["k32_b2"][0], work_cap=mid, with_runner_up=False)
    check_against_reference(got, ref_mid, default_cap=False)
    st = np.array([[r["status"] for r in per_body] for per_body in ref_mid])
    assert (st == rb.ST_WORK_CAP).any() and (st == 0).any()
    # the default cap (work_cap = 0) flags nothing here
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS, work_cap=0)
    check_against_reference(rcore.locate_rigid_bodies(xyz, n_pts), ref)


# ---------------------------------------------------------------- 7. determinism
def _dev_outputs(torch, F, B):
    dev = torch.device("cuda", 0)
    z = lambda shape, dt: torch.full(shape, 77, dtype=dt, device=dev)   # noqa: E731  (every entry must be overwritten)
    return {"found": z((F, B), torch.int32), "n_used": z((F, B), torch.int32), "assign": z((F, B, 8), torch.int8),
            "R": z((F, B, 9), torch.float64), "t": z((F, B, 3), torch.float64), "rms": z((F, B), torch.float64),
            "score": z((F, B), torch.float64), "rb_status": z((F, B), torch.int32)}


def _locate_dev(core, torch, xyz, n_pts, B_max):
    dev = torch.device("cuda", 0)
    F, K_max, _ = xyz.shape
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev)
    d_n = torch.from_numpy(np.ascontiguousarray(n_pts, dtype=np.int32)).to(dev)
    o = _dev_outputs(torch, F, B_max)
    torch.cuda.synchronize()
    core.locate_rigid_bodies_dev(F, K_max, d_xyz.data_ptr(), d_n.data_ptr(), B_max, *[o[k].data_ptr() for k in OUT_KEYS])
    core.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_twenty_launches_are_byte_identical(rcore):
    import torch
    rng = np.random.default_rng(17)
    bodies = [rb.make_body(rng, 4), rb.make_body(rng, 5), rb.make_body(rng, 8)]
    frames = _frames(rng, bodies, 64, 64, n_total=64)
    xyz, n_pts = np.stack([p for p, _, _ in frames]), np.array([n for _, n, _ in frames], dtype=np.int32)
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS)
    first = _locate_dev(rcore, torch, xyz, n_pts, 3)
    assert first["found"].sum() >= 3 * 64 - 8 and not (first["found"] == 77).any()
    host = rcore.locate_rigid_bodies(xyz, n_pts)
    for k in OUT_KEYS:
        assert first[k].tobytes() == host[k].tobytes(), k      # the host form is the same kernel
    for _ in range(19):
        again = _locate_dev(rcore, torch, xyz, n_pts, 3)
        for k in OUT_KEYS:
            assert again[k].tobytes() == first[k].tobytes(), k


# ---------------------------------------------------------------- 8. live path
def test_track_frame_bodies_is_track_frame_plus_the_locator(rcore):
    import torch
    from mocap_core import synth
    rig = synth.ring_rig(4)
    rng = np.random.default_rng(19)
    q = rb.make_body(rng, 4)
    R, t = rb.random_rotation(rng), np.array([0.1, -0.2, 0.3])

    def plant(sampled):
        out = sampled.copy()
        out[:, :4] = (R @ q.T).T + t
        return out

    blobs, counts, _ = synth.make_blob_stream(rig, 2, 6, seed=23, noise_px=0.02, dropout=0.0, truncate=False, world=plant)
    rcore.set_cameras(rig["K"], rig["R"], rig["t"])
    rcore.set_rigid_bodies([q], tol=TOL, max_rms=MAX_RMS)
    plain = rcore.track_frame(blobs, counts, K_max=16, O_max=4)
    both = rcore.track_frame_bodies(blobs, counts, K_max=16, O_max=4)
    for k, v in plain.items():
        assert both[k].tobytes() == v.tobytes(), k
    assert both["n_pts"].tolist() == [6, 6] and both["found"][:, 0].tolist() == [1, 1] and both["n_used"][:, 0].tolist() == [4, 4]
    assert (both["rms"] < 0.002).all() and (both["rms"] > 0).all()
    # the body outputs are the batch locator's on the same points, bit for bit (slots beyond n_pts hold NaN in the host arrays)
    loc = _locate_dev(rcore, torch, np.nan_to_num(both["xyz"], nan=0.0), both["n_pts"], 1)
    for k in OUT_KEYS:
        assert both[k].tobytes() == loc[k].tobytes(), k
    # the fitted pose carries the model onto the triangulated points
    for f in range(2):
        a = both["assign"][f, 0, :4]
        fit = (both["R"][f, 0] @ q.T).T + both["t"][f, 0]
        assert np.abs(fit - both["xyz"][f][a]).max() < 0.005
    # no bodies registered: the same shared fields, zero-filled body outputs
    rcore.set_rigid_bodies([])
    none = rcore.track_frame_bodies(blobs, counts, K_max=16, O_max=4, B_max=2)
    for k, v in plain.items():
        assert none[k].tobytes() == v.tobytes(), k
    for k in OUT_KEYS:
        assert none[k].shape[:2] == (2, 2) and not none[k].any(), k


# ---------------------------------------------------------------- 9. refused registrations change nothing
def test_refused_registrations_leave_the_previous_one_in_force(rcore, cases):
    from mocap_core import capi
    (bodies, K_max, frames), ref = cases["k32_b2"]
    xyz, n_pts = batch(cases["k32_b2"][0])
    rcore.set_rigid_bodies(bodies, tol=TOL, max_rms=MAX_RMS)
    before = rcore.locate_rigid_bodies(xyz, n_pts)
    assert before["found"].all()
    good = np.asarray(bodies[0])
    nonfinite, close = good.copy(), good.copy()
    nonfinite[2, 1] = np.nan
    close[1] = close[0] + [0.019, 0, 0]
    line = [[0.1 * i, 0, 0] for i in range(4)]
    refused = [dict(markers=[good] * 9), dict(markers=[good[:2]]), dict(markers=[np.vstack([good] * 3)[:9]]),
               dict(markers=[nonfinite]), dict(markers=[good, close]), dict(markers=[line]), dict(markers=[good], tol=0.0),
               dict(markers=[good], max_rms=0.0), dict(markers=[good], tol=float("nan")), dict(markers=[good], work_cap=-1)]
    for kw in refused:
        args = dict(tol=TOL, max_rms=MAX_RMS)
        args.update(kw)
        assert rb.validate(args["markers"], args["tol"], args["max_rms"], args.get("work_cap", 0)) is not None, kw
        with pytest.raises(capi.MocapError) as e:
            rcore.set_rigid_bodies(**args)
        assert e.value.code == capi.MOCAP_E_ARG, kw
        assert rcore.rigid_bodies_n == 2
        after = rcore.locate_rigid_bodies(xyz, n_pts)
        for k in OUT_KEYS:
            assert after[k].tobytes() == before[k].tobytes(), (kw, k)
    # more than 64 point slots, fewer body slots than bodies: refused like the search kernel's M <= 64
    with pytest.raises(capi.MocapError) as e:
        rcore.locate_rigid_bodies(np.zeros((1, 65, 3)), [0])
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError) as e:
        rcore.locate_rigid_bodies(xyz, n_pts, B_max=1)
    assert e.value.code == capi.MOCAP_E_ARG
    # more body slots than bodies: the extra slots are zero
    wide = rcore.locate_rigid_bodies(xyz, n_pts, B_max=4)
    for k in OUT_KEYS:
        assert wide[k][:, :2].tobytes() == before[k].tobytes() and not wide[k][:, 2:].any(), k
