"""Rigid-body learning on the device (include/mocap_core.h, "rigid-body learning"; csrc/body_learn.hip) against the plain statement
of the contract (tests/body_learn_reference.py): discrete outputs exactly, continuous ones against the 50-digit evaluation, the
bits from call to call, the refusals, and a learned body through registration and the per-frame search."""
import math

import numpy as np
import pytest

import body_learn_reference as bl
import rigid_body_reference as rb

pytestmark = pytest.mark.gpu

INF = float("inf")
Q5 = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.15, 0.0], [0.05, 0.05, 0.18], [0.17, 0.16, 0.07]])
Q8 = np.array([[0.0, 0, 0], [0.12, 0, 0], [0, 0.1, 0], [0.05, 0.05, 0.2], [0.15, 0.1, 0.05], [-0.05, 0.1, 0.1], [0.1, -0.06, 0.12],
               [-0.04, -0.05, 0.06]])


def learn(core, cap, sel=None, status=None, **kw):
    return core.learn_rigid_body(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"] if sel is None else sel, status, **kw)


def reference(cap, sel=None, status=None, exact=False, **kw):
    fn = bl.learn_mp if exact else bl.learn
    return fn(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"] if sel is None else sel, status, **kw)


def raw_host(core, cap, sel=None, status=None, ref_frame=-1, iters=4, max_rms=INF, result=None):
    """The C entry point itself -> (return code, the 129 doubles)."""
    from mocap_core.capi import _p
    xyz = np.ascontiguousarray(cap["xyz"], dtype=np.float64)
    n_pts = np.ascontiguousarray(cap["n_pts"], dtype=np.int32)
    ids = np.ascontiguousarray(cap["id"], dtype=np.int32)
    sel = np.ascontiguousarray(cap["sel"] if sel is None else sel, dtype=np.int32)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    res = np.zeros(129) if result is None else result
    rc = core.lib.mocap_learn_rigid_body(core._h, xyz.shape[0], xyz.shape[1], _p(xyz), _p(n_pts), _p(ids), _p(status), sel.size,
                                         _p(sel), int(ref_frame), int(iters), float(max_rms), _p(res))
    return rc, res


def raw_dev(core, cap, status=None, ref_frame=-1, iters=4, max_rms=INF):
    import torch
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cap["xyz"], cap["n_pts"].astype(np.int32), cap["id"].astype(np.int32))]
    d_st = None if status is None else torch.from_numpy(np.ascontiguousarray(status, dtype=np.int32)).to(dev)
    d_res = torch.full((129,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    F, K_max = cap["xyz"].shape[:2]
    core.learn_rigid_body_dev(F, K_max, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0 if d_st is None else d_st.data_ptr(),
                              cap["sel"], ref_frame, iters, max_rms, d_res.data_ptr())
    core.synchronize()
    return d_res.cpu().numpy()


def check(got, ref, what, atol=1e-10):
    """Discrete outputs exactly; the continuous ones close to the float64 statement (the bound proper is test_accuracy's)."""
    assert not bl.same_discrete(got, ref), (what, bl.same_discrete(got, ref), {k: (got[k], ref[k]) for k in bl.same_discrete(got, ref)})
    for k in bl.FIELDS:
        d = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k], dtype=np.float64)).max()
        assert d <= atol, (what, k, d)


def prefix(cap, F):
    return {k: (v[:F] if isinstance(v, np.ndarray) else v) for k, v in cap.items()}


def to_end(cap, f, slot=0):
    """Frees `slot` of frame f: its point and id move behind the frame's last point."""
    n = int(cap["n_pts"][f])
    cap["xyz"][f, n], cap["id"][f, n] = cap["xyz"][f, slot], cap["id"][f, slot]
    cap["n_pts"][f] = n + 1


def decorate(cap, rng):
    """The gather's corner cases, wherever the frame has the room: a duplicated id behind the real point (frame 1) and in front of
    it (frame 3: the lowest slot wins), a non-finite point carrying a selected id in front of the real one (frame 2), and with 64
    slots a frame filled to the brim whose slot 63 holds a selected id (frame 4)."""
    F, K_max = cap["xyz"].shape[:2]
    sel = cap["sel"]
    room = lambda f, k=1: f < F and cap["n_pts"][f] + k <= K_max      # noqa: E731
    if room(1):
        n = cap["n_pts"][1]
        cap["xyz"][1, n], cap["id"][1, n] = rng.uniform(-1, 1, 3), sel[0]
        cap["n_pts"][1] = n + 1
    if room(2):
        to_end(cap, 2)
        cap["xyz"][2, 0], cap["id"][2, 0] = [0.1, np.inf, 0.2], sel[1]
    if room(3):
        to_end(cap, 3)
        cap["xyz"][3, 0], cap["id"][3, 0] = rng.uniform(-1, 1, 3), sel[2]
    if K_max == 64 and F > 4:
        n = int(cap["n_pts"][4])
        j = np.nonzero(cap["id"][4, :n] == sel[0])[0]
        keep = [k for k in range(n) if k not in j[:1]]
        pts, ids = cap["xyz"][4, keep].copy(), cap["id"][4, keep].copy()
        cap["xyz"][4, :63] = rng.uniform(-1, 1, (63, 3))
        cap["id"][4, :63] = 5000 + np.arange(63)
        cap["xyz"][4, :len(keep)], cap["id"][4, :len(keep)] = pts, ids
        cap["xyz"][4, 63], cap["id"][4, 63] = cap["R"][4] @ cap["template"][0] + cap["t"][4], sel[0]
        cap["n_pts"][4] = 64
    return cap


SHAPES = [(3, 3), (3, 8), (8, 8), (3, 64), (8, 64)]           # (N, K_max)
LARGE = [(3, 3), (8, 64)]                                     # ... of which these go up to 64 * 256 + 1 frames
FRAMES = [1, 63, 64, 65, 255, 256, 257]


@pytest.fixture(scope="module")
def captures():
    out = {}
    for N, K_max in SHAPES:
        rng = np.random.default_rng(100 * N + K_max)
        q = Q8[:N]
        F = 16385 if (N, K_max) in LARGE else 257
        cap = bl.make_capture(rng, q, F, K_max, noise=0.0005, dropout=0.0 if K_max == 3 else 0.15, n_clutter=min(3, K_max - N))
        cap["template"] = q
        out[(N, K_max)] = decorate(cap, rng)
    return out


# ---------------------------------------------------------------- 1. shapes at which the tree changes path; the gather's corners
@pytest.mark.parametrize("F,N,K_max", [(F, N, K) for F in FRAMES for (N, K) in SHAPES] + [(16385, N, K) for (N, K) in LARGE])
def test_shapes_where_the_tree_changes_path(core, captures, F, N, K_max):
    cap = prefix(captures[(N, K_max)], F)
    max_rms = INF
    assert math.isinf(max_rms) and bl.gate_margin({"frame_rms": []}, max_rms) > 1e-9          # no gate: no frame near it
    got = learn(core, cap, iters=2, max_rms=max_rms)
    ref = reference(cap, iters=2, max_rms=max_rms)
    check(got, ref, (F, N, K_max))
    assert got["status"] == 0 and got["ref_frame"] == 0 and got["frames_valid"] == F
    if K_max == 64 and F > 4:                                        # the corner cases are in the capture
        slots, _ = bl.gather(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"])
        assert slots[4, 0] == 63 and cap["n_pts"][4] == 64
        assert slots[3, 2] == 0 and slots[2, 1] != 0 and cap["id"][2, 0] == cap["sel"][1]   # the duplicate in front wins; the non-finite point does not


# ---------------------------------------------------------------- 2. the valid-slot rule
def test_valid_slot_rule(core):
    """Twelve frames of a 200-frame capture are empty valid frames in the base capture.  Filling them with garbage beyond n_pts,
    with complete marker sets under an n_pts outside 0 .. K_max or a non-zero status, or with clutter and 0 or 1 present markers
    changes nothing but frames_valid -- bit for bit.  A frame with 2 present markers is valid, poses nothing, and by the
    contract's pair statistics counts for that one pair: every other output keeps its bits."""
    rng = np.random.default_rng(41)
    full = bl.make_capture(rng, Q5, 200, 16, noise=0.0005, dropout=0.2, n_clutter=3)
    special = list(range(7, 200, 17))
    base = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in full.items()}
    base["n_pts"][special] = 0
    rc, r0 = raw_host(core, base, iters=3, max_rms=0.004)
    assert rc == 0 and r0[125] == 200 and r0[128] == 0 and r0[124] > 100
    ref = reference(base, iters=3, max_rms=0.004)
    assert bl.gate_margin(reference(base, iters=3, max_rms=0.004, exact=True), 0.004) > 1e-9
    check(core.learned_body(r0, 5), ref, "base")

    def variant(edit, status=None):
        cap = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        edit(cap)
        rc, r = raw_host(core, cap, status=status, iters=3, max_rms=0.004)
        assert rc == 0
        return r

    def same_but(r, valid, skip=()):
        keep = [i for i in range(129) if i != 125 and i not in skip]
        assert r[keep].tobytes() == r0[keep].tobytes() and r[125] == valid

    def garbage(cap):                                               # NaN and matching ids beyond n_pts, in every frame
        for f in range(200):
            n = int(cap["n_pts"][f])
            cap["xyz"][f, n:] = np.nan
            cap["xyz"][f, n:n + 2] = 0.25
            cap["id"][f, n:] = cap["sel"][f % 5]
    same_but(variant(garbage), 200)

    def bad_counts(cap):                                            # complete frames under an impossible count
        for i, f in enumerate(special):
            cap["n_pts"][f] = (-1, 17, 1 << 30, -(1 << 31))[i % 4]
            cap["xyz"][f], cap["id"][f] = full["xyz"][f], full["id"][f]
    same_but(variant(bad_counts), 200 - len(special))

    def restore(cap):                                               # complete frames, switched off by their status
        for f in special:
            cap["n_pts"][f], cap["xyz"][f], cap["id"][f] = full["n_pts"][f], full["xyz"][f], full["id"][f]
    status = np.zeros(200, dtype=np.int32)
    status[special] = [1, 2, 4, -1] * 3
    same_but(variant(restore, status), 200 - len(special))

    def few(k):
        def edit(cap):                                              # clutter and k of the body's markers
            for f in special:
                cap["n_pts"][f] = 6
                cap["xyz"][f, :6] = rng.uniform(-1, 1, (6, 3))
                cap["id"][f, :6] = 7000 + np.arange(6)
                cap["id"][f, 1:1 + k] = cap["sel"][3:3 + k]
        return edit
    same_but(variant(few(0)), 200)
    same_but(variant(few(1)), 200)
    p34 = rb_pair(3, 4)
    r2 = variant(few(2))
    same_but(r2, 200, skip=(40 + p34, 68 + p34, 96 + p34))
    assert r2[96 + p34] == r0[96 + p34] + len(special)


def rb_pair(i, j):
    return i * (2 * 8 - i - 1) // 2 + (j - i - 1)


# ---------------------------------------------------------------- 3. no reference frame
def test_no_reference_frame(core):
    rng = np.random.default_rng(42)
    cap = bl.make_capture(rng, Q5, 70, 12, noise=0.0005, n_clutter=2)
    for f in range(70):                                             # marker 4 never together with marker 0
        n = cap["n_pts"][f]
        cap["id"][f, np.nonzero(cap["id"][f, :n] == cap["sel"][4 if f % 2 else 0])[0]] = 3000
    want = np.zeros(129)
    want[126], want[128] = -1.0, 1.0
    rc, r = raw_host(core, cap, result=np.full(129, 5.0))
    assert rc == 0 and r.tobytes() == want.tobytes()                                          # no complete frame
    assert raw_dev(core, cap).tobytes() == want.tobytes()
    rc, r = raw_host(core, cap, ref_frame=3, result=np.full(129, 5.0))
    assert rc == 0 and r.tobytes() == want.tobytes()                                          # the given frame is incomplete
    check(core.learned_body(r, 5), reference(cap, ref_frame=3), "incomplete")
    whole = bl.make_capture(rng, Q5, 70, 12, noise=0.0005, n_clutter=2)
    status = np.zeros(70, dtype=np.int32)
    status[3] = 1
    rc, r = raw_host(core, whole, status=status, ref_frame=3, result=np.full(129, 5.0))
    assert rc == 0 and r.tobytes() == want.tobytes()                                          # the given frame is not valid
    whole["n_pts"][5] = 13
    rc, r = raw_host(core, whole, ref_frame=5, result=np.full(129, 5.0))
    assert rc == 0 and r.tobytes() == want.tobytes()
    rc, r = raw_host(core, whole, status=status, ref_frame=-1)                               # ... while the search skips both
    assert rc == 0 and r[126] == 0 and r[128] == 0 and r[125] == 68
    from mocap_core import capi, helpers
    helpers.set_core(core)
    with pytest.raises(capi.MocapError, match="ref_frame"):
        helpers.learn_rigid_body(cap, sel=cap["sel"])


# ---------------------------------------------------------------- 4. a marker without a used frame
def unseen_scene():
    """Eight markers.  0 .. 2 are in every frame; each later frame shows one of 4 .. 7; marker 3 is in the reference frame and in
    the frames whose marker 1 is 4 cm off (rejected in every round).  In the reference frame 4 .. 7 sit 1 cm further from the
    centroid than on the body: round 1 takes it (rms 0) and every plain frame (one marker off in four, rms below the gate), round 2
    poses it against a template whose markers 4 .. 7 have moved to the other frames' average -- four markers off in eight, above
    the gate -- so that marker 3 has no used frame left."""
    rng = np.random.default_rng(5)
    F = 161
    cap = bl.make_capture(rng, Q8, F, 12, noise=0.0001, n_clutter=2)
    c = Q8.mean(axis=0)
    for k in range(4, 8):
        u = (Q8[k] - c) / np.linalg.norm(Q8[k] - c)
        bl.displace(cap, [0], k, cap["R"][0] @ (0.01 * u))
    off = [f for f in range(1, F) if f % 10 == 5]
    for f in range(1, F):
        n = cap["n_pts"][f]
        for m in ([] if f in off else [3]) + [m for m in range(4, 8) if m != 4 + f % 4]:
            cap["id"][f, np.nonzero(cap["id"][f, :n] == cap["sel"][m])[0][0]] = 2000 + m
    bl.displace(cap, off, 1, np.array([0.03, 0.02, -0.03]))
    return cap, off


def test_marker_unseen_keeps_its_position(core):
    cap, off = unseen_scene()
    gate = 0.0045
    exact = reference(cap, iters=3, max_rms=gate, exact=True)
    assert bl.gate_margin(exact, gate) > 1e-9
    got, ref = learn(core, cap, iters=3, max_rms=gate), reference(cap, iters=3, max_rms=gate)
    assert not bl.same_discrete(got, exact) and not bl.same_discrete(ref, exact)
    check(got, ref, "unseen")
    assert got["status"] == bl.ST_MARKER_UNSEEN and got["marker_frames"][3] == 0 and got["marker_rms"][3] == 0.0
    assert got["marker_frames"][0] == got["frames_used"] > 100 and got["ref_frame"] == 0
    one = learn(core, cap, iters=1, max_rms=gate)                  # round 1 still had the reference frame
    assert one["status"] == 0 and one["marker_frames"][3] == 1
    # what the marker keeps is "Q of the round before": the float64 statement compared above does exactly that, round by round
    two = learn(core, cap, iters=2, max_rms=gate)
    assert two["status"] == bl.ST_MARKER_UNSEEN and two["marker_frames"][3] == 0
    check(two, reference(cap, iters=2, max_rms=gate), "unseen, two rounds")


# ---------------------------------------------------------------- 5. accuracy against fifty digits
def accuracy_scene(name):
    rng = np.random.default_rng(51)
    if name == "n5_gated":
        cap = bl.make_capture(rng, Q5, 100, 16, noise=0.0005, dropout=0.2, n_clutter=3)
        bl.displace(cap, range(4, 100, 9), 2, np.array([0.02, -0.01, 0.015]))
        return cap, 0.003
    if name == "n8_k64":
        return bl.make_capture(rng, Q8, 60, 64, noise=0.001, dropout=0.25, n_clutter=20), INF
    return bl.make_capture(rng, Q8[:3], 257, 8, noise=0.0002, n_clutter=1), INF


@pytest.mark.parametrize("name", ["n5_gated", "n8_k64", "n3_f257"])
def test_accuracy_against_fifty_digits(core, name):
    worst = {"device": 0.0, "numpy": 0.0, "ratio": 0.0}
    cap, gate = accuracy_scene(name)
    for iters in (1, 4):
        exact = reference(cap, iters=iters, max_rms=gate, exact=True)
        assert bl.gate_margin(exact, gate) > 1e-9
        got, ref = learn(core, cap, iters=iters, max_rms=gate), reference(cap, iters=iters, max_rms=gate)
        assert not bl.same_discrete(got, exact), (name, iters, bl.same_discrete(got, exact))
        assert not bl.same_discrete(ref, exact), (name, iters, bl.same_discrete(ref, exact))
        e_dev, e_ref = bl.field_errors(got, exact), bl.field_errors(ref, exact)
        for k in bl.FIELDS:
            floor = 64 * np.spacing(max(1.0, e_dev[k][1]))
            bound = max(16 * e_ref[k][0], floor)
            worst["device"], worst["numpy"] = max(worst["device"], e_dev[k][0]), max(worst["numpy"], e_ref[k][0])
            worst["ratio"] = max(worst["ratio"], e_dev[k][0] / bound)
            print(f"learn {name} iters={iters} {k}: device {e_dev[k][0]:.2e} numpy {e_ref[k][0]:.2e} bound {bound:.2e}")
            assert e_dev[k][0] <= bound, (name, iters, k, e_dev[k][0], e_ref[k][0], floor)
    print(f"learn accuracy summary {name}: worst device error {worst['device']:.3e}, worst numpy error {worst['numpy']:.3e}, "
          f"worst error / bound {worst['ratio']:.3f}")


# ---------------------------------------------------------------- 6. the bits do not depend on the call
def test_bits_do_not_depend_on_the_call(core):
    import torch
    rng = np.random.default_rng(61)
    cap = bl.make_capture(rng, Q5, 5000, 16, noise=0.0005, dropout=0.2, n_clutter=4)
    status = (rng.random(5000) < 0.05).astype(np.int32)
    status[0] = 0
    kw = dict(status=status, iters=4, max_rms=0.004)
    rc, host = raw_host(core, cap, **kw)
    assert rc == 0 and host[128] == 0 and 1000 < host[124] < host[125] == 5000 - status.astype(bool).sum()
    assert raw_host(core, cap, **kw)[1].tobytes() == host.tobytes()
    dev = raw_dev(core, cap, **kw)
    assert dev.tobytes() == host.tobytes()
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        other = raw_dev(core, cap, **kw)
    finally:
        core.set_stream(0)
    assert other.tobytes() == host.tobytes()


def test_chained_behind_track_frame_ids_dev(core):
    """Four frames of the 8 x 16 synthetic stream through mocap_track_frame_ids_dev; the points and ids go from its device buffers
    straight into mocap_learn_rigid_body_dev.  The result equals the host form's on the copied-back arrays, bit for bit."""
    import torch
    import marker_track_reference as mt
    from mocap_core import synth
    rig = synth.ring_rig(8)
    drift = lambda sampled: sampled[:1] + np.arange(4)[:, None, None] * np.array([0.005, 0.0, 0.0])   # noqa: E731
    blobs, counts, _ = synth.make_blob_stream(rig, 4, 16, seed=31, noise_px=0.02, dropout=0.0, min_sep=0.15, world=drift)
    t = 50.0 + np.arange(4) / 60.0
    core.set_world_transform(None)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_marker_tracker(**mt.DEFAULTS)
    try:
        dev = torch.device("cuda", 0)
        F, C, M, K, O = 4, 8, 16, 32, 4
        d_in = [torch.from_numpy(a).to(dev) for a in (blobs, counts, t)]
        shapes = {"xyz": ((F, K, 3), torch.float64), "err": ((F, K), torch.float64), "corr": ((F, K, C), torch.int16),
                  "n_pts": ((F,), torch.int32), "status": ((F,), torch.int32), "pos": ((F, O, 3), torch.float64),
                  "heading": ((F, O), torch.float64), "error": ((F, O), torch.float64), "droneIndex": ((F, O), torch.int32),
                  "n_obj": ((F,), torch.int32), "id": ((F, K), torch.int32), "hits": ((F, K), torch.int32),
                  "n_tracks": ((F,), torch.int32), "mk_status": ((F,), torch.int32)}
        d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        d_res = torch.zeros(129, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        core.track_frame_ids_dev(F, M, d_in[0].data_ptr(), d_in[1].data_ptr(), 5.0, K, 1 << 20,
                                 *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")], O,
                                 *[d[k].data_ptr() for k in ("pos", "heading", "error", "droneIndex", "n_obj")], d_in[2].data_ptr(),
                                 *[d[k].data_ptr() for k in ("id", "hits", "n_tracks", "mk_status")])
        core.synchronize()
        ids, hits, n3 = d["id"][3].cpu().numpy(), d["hits"][3].cpu().numpy(), int(d["n_pts"][3])
        sel = sorted(int(i) for i in ids[:n3][hits[:n3] == 4])[:5]      # five tracks that lasted the four frames
        assert len(sel) == 5
        core.learn_rigid_body_dev(F, K, d["xyz"].data_ptr(), d["n_pts"].data_ptr(), d["id"].data_ptr(), d["status"].data_ptr(),
                                  sel, -1, 2, INF, d_res.data_ptr())
        core.synchronize()
        chained = d_res.cpu().numpy()
        cap = {"xyz": d["xyz"].cpu().numpy(), "n_pts": d["n_pts"].cpu().numpy(), "id": d["id"].cpu().numpy(), "sel": sel}
        status = d["status"].cpu().numpy()
    finally:
        core.set_marker_tracker(T_max=0)
    assert not status.any() and cap["n_pts"].min() >= 12
    rc, host = raw_host(core, cap, status=status, iters=2)
    assert rc == 0 and chained.tobytes() == host.tobytes()
    got = core.learned_body(chained, 5)
    assert got["status"] == 0 and got["ref_frame"] == 0 and got["frames_used"] == 4 and got["marker_frames"].tolist() == [4] * 5
    check(got, reference(cap, status=status, iters=2), "chained")
    assert got["min_pair_distance"] >= 0.1 and got["pair_std"].max() < 0.005      # the stream's markers are 0.15 m apart and move as one


# ---------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_result_untouched(core):
    from mocap_core import capi
    rng = np.random.default_rng(71)
    cap = bl.make_capture(rng, Q5, 10, 8, noise=0.0005, n_clutter=2)
    sel = cap["sel"]
    wide = {"xyz": np.zeros((10, 65, 3)), "n_pts": np.zeros(10, dtype=np.int32), "id": np.zeros((10, 65), dtype=np.int32), "sel": sel}
    none = {"xyz": np.zeros((10, 0, 3)), "n_pts": np.zeros(10, dtype=np.int32), "id": np.zeros((10, 0), dtype=np.int32), "sel": sel}
    empty = prefix(cap, 0)
    cases = [("K_max 65", wide, {}), ("K_max 0", none, {}), ("n_frames 0", empty, {}),
             ("N 2", cap, {"sel": sel[:2]}), ("N 9", cap, {"sel": list(range(9))}),
             ("negative id", cap, {"sel": [sel[0], -1, sel[2]]}), ("repeated id", cap, {"sel": [sel[0], sel[1], sel[2], sel[1]]}),
             ("iters 0", cap, {"iters": 0}), ("iters 17", cap, {"iters": 17}), ("iters -1", cap, {"iters": -1}),
             ("max_rms 0", cap, {"max_rms": 0.0}), ("max_rms < 0", cap, {"max_rms": -1.0}), ("max_rms NaN", cap, {"max_rms": float("nan")}),
             ("max_rms -inf", cap, {"max_rms": -INF}), ("ref_frame -2", cap, {"ref_frame": -2}), ("ref_frame F", cap, {"ref_frame": 10})]
    for what, c, kw in cases:
        canary = np.full(129, 12345.678)
        rc, r = raw_host(core, c, result=canary, **kw)
        assert rc == capi.MOCAP_E_ARG, (what, rc)
        assert (r == 12345.678).all(), what
        assert b"mocap_learn_rigid_body" in core.lib.mocap_last_error(core._h), what
    # the device form refuses the same way, before anything is enqueued
    import torch
    d_res = torch.full((129,), 12345.678, dtype=torch.float64, device="cuda:0")
    with pytest.raises(capi.MocapError) as e:
        core.learn_rigid_body_dev(10, 8, d_res.data_ptr(), d_res.data_ptr(), d_res.data_ptr(), 0, sel, -1, 0, INF, d_res.data_ptr())
    assert e.value.code == capi.MOCAP_E_ARG
    with pytest.raises(capi.MocapError):
        core.learn_rigid_body_dev(10, 8, 0, d_res.data_ptr(), d_res.data_ptr(), 0, sel, -1, 4, INF, d_res.data_ptr())
    core.synchronize()
    assert (d_res.cpu().numpy() == 12345.678).all()
    rc, r = raw_host(core, cap, max_rms=INF, ref_frame=9, iters=16)             # the edges of what is accepted
    assert rc == 0 and r[126] == 9 and r[128] == 0


# ---------------------------------------------------------------- 8. learn -> register -> locate
def test_learned_body_registers_and_is_found(core):
    import torch
    from mocap_core import helpers
    assert all(rb.posable_table(Q5)[s] for s in range(32) if bin(s).count("1") >= 3)
    rng = np.random.default_rng(81)
    noise = 0.0005
    cap = bl.make_capture(rng, Q5, 300, 16, noise=noise, dropout=0.2, n_clutter=3)
    fresh = bl.make_capture(rng, Q5, 60, 16, noise=noise, dropout=0.3, n_clutter=3, complete_first=False)
    core.set_world_transform(None)
    helpers.set_core(core)
    try:
        learned = helpers.learn_rigid_body({"xyz": cap["xyz"], "n_out": cap["n_pts"], "id": cap["id"]}, name="wand")
        assert learned["sel"] == cap["sel"] and learned["name"] == "wand" and learned["status"] == 0 and learned["frames_used"] > 250
        assert abs(learned["min_pair_distance"] - min(rb.dist(Q5[i], Q5[j]) for i in range(5) for j in range(i))) < 1e-3
        # the same capture resident on the GPU: read in place, the same bits
        dev = torch.device("cuda", 0)
        resident = {"xyz": torch.from_numpy(cap["xyz"]).to(dev), "n_pts": torch.from_numpy(cap["n_pts"]).to(dev),
                    "id": torch.from_numpy(cap["id"]).to(dev)}
        again = helpers.learn_rigid_body(resident, name="wand")
        assert again["sel"] == learned["sel"] and all(np.asarray(again[k]).tobytes() == np.asarray(learned[k]).tobytes() for k in bl.FIELDS)
        with pytest.raises(ValueError, match="track ids"):
            helpers.learn_rigid_body({"xyz": cap["xyz"][:, :2], "n_pts": np.minimum(cap["n_pts"], 2), "id": cap["id"][:, :2]})
        tol, max_rms = 0.005, 0.005
        assert tol < learned["min_pair_distance"] / 2
        helpers.set_rigid_bodies([learned], tol=tol, max_rms=max_rms)
        got = core.locate_rigid_bodies(fresh["xyz"], fresh["n_pts"])
        helpers.set_rigid_bodies([{"name": "planted", "markers": Q5.tolist()}], tol=tol, max_rms=max_rms)
        plant = core.locate_rigid_bodies(fresh["xyz"], fresh["n_pts"])
    finally:
        helpers.set_rigid_bodies([])
    shows = fresh["shown"].sum(axis=1)
    assert (shows >= 3).sum() >= 50 and (shows == 3).sum() >= 5
    worst = 0.0
    for f in range(60):
        if shows[f] >= 3:
            assert got["found"][f, 0] == 1 and plant["found"][f, 0] == 1 and got["n_used"][f, 0] == shows[f], f
            assert got["assign"][f, 0].tolist() == plant["assign"][f, 0].tolist(), f
            worst = max(worst, got["rms"][f, 0] / plant["rms"][f, 0])
            assert got["rms"][f, 0] <= 1.5 * plant["rms"][f, 0], (f, got["rms"][f, 0], plant["rms"][f, 0])
    print(f"learned against planted template over {(shows >= 3).sum()} fresh frames: worst rms ratio {worst:.3f}")
