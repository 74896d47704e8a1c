"""CPU: the "body trajectories" contract (include/mocap_core.h) as tests/body_session_reference.py states it -- the six symbols, the
lanes form against the scalar one bit for bit, the statement against planted truth (poses of noise-free motions, rigidly filled
markers, the angular velocity of a constant-rate rotation) and against a 50-digit evaluation of the same fit, the sign rule as a
walk against its prefix-parity form, and the flags of the two smoothers.

Every bound below is four times the largest deviation of the STATEMENT, measured here on the CPU over this file's seeds (the
conditioning varies with the seed); `measure()` prints them (python tests/test_body_session_reference_cpu.py) and DESIGN.md 3.7q
records both numbers.  None is taken from the device: the device is compared with the statement bit for bit."""
import os
import re

import numpy as np

import body_session_reference as bs
import rigid_body_reference as rbr
import track_smooth_reference as ts
from conftest import ROOT

INF = float("inf")
SEEDS = (1, 2, 3, 4, 5, 6)
PAR = dict(degree=2, W=8, span=INF, n_min=5, max_gap=4)

# measured (largest over SEEDS) -> bound = 4 x measured
MEASURED = {
    "pose_R": 1.47e-14, "pose_t": 8.88e-16, "pose_rms": 1.04e-15,          # noise-free motions: |R - R_true|, |t - c_true|, rms (metres)
    "fill": 2.91e-15,                                              # noise-free: |SRC_RIGID sample - the hidden marker's true position| (metres)
    "omega": 3.54e-3,                                             # constant-rate rotation: |omega - rate * axis| / rate
    "mp_pose_R": 3.15e-15, "mp_pose_t": 1.93e-16,                       # noisy frames: the float64 pose against the 50-digit one
    "mp_quat_s": 9.99e-16, "mp_omega": 1.27e-14,                        # noisy windows: quat_s, and omega relative to 1 / h, against the 50-digit fit
}


def bound(k):
    return 4.0 * MEASURED[k]


# ---------------------------------------------------------------- the symbols
def test_the_six_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    header = open(os.path.join(ROOT, "include", "mocap_core.h")).read()
    lib = capi.load_library()
    for name, n_args in (("mocap_pose_rows", 16), ("mocap_pose_rows_dev", 16), ("mocap_smooth_rotations", 15),
                         ("mocap_smooth_rotations_dev", 15), ("mocap_fill_rows", 16), ("mocap_fill_rows_dev", 16)):
        proto = re.search(r"\bint %s\((.*?)\);" % name, header, flags=re.S)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == n_args and getattr(lib, name) is not None
    for k, v in (("POSED", bs.POSED), ("FEW", bs.FEW), ("DEGENERATE", bs.DEGENERATE), ("RMS", bs.RMS), ("SRC_NONE", bs.SRC_NONE),
                 ("SRC_MEASURED", bs.SRC_MEASURED), ("SRC_RIGID", bs.SRC_RIGID), ("SRC_RIGID_FILLED", bs.SRC_RIGID_FILLED),
                 ("MAX_BODIES", bs.MAX_BODIES)):
        assert getattr(capi, "BP_" + k) == v and re.search(r"MOCAP_BP_%s\b[ =]+%d\b" % (k, v), header), k


def test_validate_names_every_refusal():
    _, traj, bodies, _ = bs.make_session(1, 20, (3, 4))
    R, F, _ = traj.shape
    assert bs.validate(bodies, R, F) is None
    line = np.array([[0.0, 0, 0], [0.1, 0, 0], [0.3, 0, 0]])
    bad = [[], bodies * 33, [([0, 1], bodies[0][1][:2])], [([0, 1, R], bodies[0][1])], [([0, 1, 1], bodies[0][1])],
           [bodies[0], ([0, 3, 4, 5], bodies[1][1])], [([0, 1, 2], np.where(np.eye(3) > 0, np.nan, bodies[0][1]))], [([0, 1, 2], line)]]
    for bb in bad:
        assert bs.validate(bb, R, F) is not None
    assert bs.validate(bodies, 0, F) and bs.validate(bodies, 1025, F) and bs.validate(bodies, R, 0) and bs.validate(bodies, R, 2 ** 31 // R + 1)


# ---------------------------------------------------------------- the two forms of the statement
def test_the_lanes_form_is_the_scalar_form_bit_for_bit():
    for seed in SEEDS[:3]:
        _, traj, bodies, _ = bs.make_session(seed, 120, (3, 5, 8))
        o = bs.pose_rows(traj, bodies, INF, raw=True)
        n = 0
        for b, (rows, Q) in enumerate(bodies):
            for f in np.flatnonzero(o["flag"][b] == bs.POSED):
                pm = [m for m in range(len(rows)) if o["present"][b, f] >> m & 1]
                q, R, t, rms = bs.pose_sample([traj[rows[m], f] for m in pm], [Q[m] for m in pm])
                assert bs.same_bits(q, o["quat_raw"][b, f]) and bs.same_bits(np.reshape(R, (3, 3)), o["R"][b, f])
                assert bs.same_bits(t, o["t_pose"][b, f]) and rms == o["rms"][b, f]
                n += 1
        assert n > 200


def test_the_sign_walk_is_the_prefix_parity_on_random_sequences_with_exact_zeros():
    rng = np.random.default_rng(0)
    basis = np.vstack([np.eye(4), -np.eye(4)])
    hit = {"zero": 0, "flip": 0, "zero at s = 1": 0, "w = 0 first": 0}
    for trial in range(300):
        F = int(rng.integers(1, 40))
        quat = rng.standard_normal((F, 4))
        quat /= np.linalg.norm(quat, axis=1, keepdims=True)
        axis = rng.uniform(size=F) < 0.5                             # half of them unit vectors: dots of exactly 0, w of exactly 0
        quat[axis] = basis[rng.integers(0, 8, int(axis.sum()))]
        posed = rng.uniform(size=F) < 0.7
        quat[~posed] = np.nan
        walk, parity = bs.sign_walk(quat, posed), bs.sign_parity(quat, posed)
        assert np.array_equal(walk, parity), trial
        p = np.flatnonzero(posed)
        d = (quat[p[1:]] * quat[p[:-1]]).sum(axis=1) if p.size > 1 else np.zeros(0)
        hit["zero"] += int((d == 0).sum())
        hit["flip"] += int((d < 0).sum())
        hit["zero at s = 1"] += int(((d == 0) & (walk[p[:-1]] == 1)).sum())
        hit["w = 0 first"] += int(p.size > 0 and quat[p[0], 0] == 0)
        out = np.where(walk[:, None] == 1, -quat, quat)
        if p.size > 1:                                               # the output never turns against its predecessor
            assert ((out[p[1:]] * out[p[:-1]]).sum(axis=1) >= 0).all()
    assert min(hit.values()) >= 20, hit


# ---------------------------------------------------------------- against truth
def _noise_free(seed):
    t, traj, bodies, truth = bs.make_session(seed, 300, (3, 4, 8), n_loose=1, sigma=0.0, dropout=0.10)
    return t, traj, bodies, truth, bs.pose_rows(traj, bodies, INF)


def measure_poses():
    dR = dt = dr = 0.0
    for seed in SEEDS:
        _, _, _, truth, o = _noise_free(seed)
        m = o["flag"] == bs.POSED
        assert m.mean() > 0.7
        dR = max(dR, np.abs(o["R"][m] - truth["R"][m]).max())
        dt = max(dt, np.abs(o["t_pose"][m] - truth["c"][m]).max())
        dr = max(dr, o["rms"][m].max())
        q = o["quat"][m]
        assert np.abs((q * q).sum(axis=1) - 1.0).max() < 1e-15
    return {"pose_R": dR, "pose_t": dt, "pose_rms": dr}


def test_noise_free_motions_are_reproduced():
    got = measure_poses()
    for k, v in got.items():
        assert v <= bound(k), (k, v, bound(k))


def measure_fill():
    worst, n = 0.0, 0
    for seed in SEEDS:
        t, traj, bodies, truth, o = _noise_free(seed)
        rot = bs.smooth_rotations(t, o["quat"], **PAR)
        tr = ts.smooth(t, o["t_pose"], **PAR)
        fill = bs.fill_rows(traj, bodies, o["flag"], o["R"], o["t_pose"], rot["flag"], rot["quat_s"], tr["pos"])
        m = fill["src"] == bs.SRC_RIGID
        n += int(m.sum())
        worst = max(worst, np.abs(fill["filled"][m] - truth["rows"][m]).max())
        assert bs.same_bits(fill["filled"][fill["src"] == bs.SRC_MEASURED], traj[fill["src"] == bs.SRC_MEASURED])
        assert np.isnan(fill["filled"][fill["src"] == bs.SRC_NONE]).all() and (fill["src"][-1] <= bs.SRC_MEASURED).all()
    assert n > 1000
    return {"fill": worst}


def test_rigidly_filled_markers_are_where_the_markers_were():
    got = measure_fill()
    assert got["fill"] <= bound("fill"), got


def _spinning(seed, F=200, rate_hz=120.0):
    """A body turning at a constant rate about a fixed axis, noise-free, regular stamps -> t, traj, bodies, rate * axis."""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    rate = float(rng.uniform(1.0, 6.0))                                  # rad / s
    t = 1.0 + np.arange(F) / rate_hz
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    ang = rate * (t - t[0])
    Rm = np.eye(3)[None] + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
    q = bs.template(rng, 4)
    traj = np.einsum("fij,nj->nfi", Rm @ rbr.random_rotation(rng), q) + rng.uniform(-1, 1, 3)
    return t, traj, [([0, 1, 2, 3], q)], rate * axis, rate


def measure_omega():
    worst = 0.0
    for seed in SEEDS:
        t, traj, bodies, want, rate = _spinning(seed)
        o = bs.pose_rows(traj, bodies, INF)
        rot = bs.smooth_rotations(t, o["quat"], **PAR)
        m = rot["flag"][0] == ts.SMOOTHED
        assert m.sum() >= 190
        worst = max(worst, np.abs(rot["omega"][0, m] - want).max() / rate)
    return {"omega": worst}


def test_angular_velocity_of_a_constant_rate_rotation_is_rate_times_axis():
    """The component-wise quadratic is not the rotation: over a window of +-8 frames at 120 Hz and up to 6 rad/s the half angle
    moves by up to 0.2 rad, and the fit's truncation shows in the fourth digit.  The bound is the measured one times four."""
    got = measure_omega()
    assert got["omega"] <= bound("omega"), got


# ---------------------------------------------------------------- against 50 digits
def measure_mp():
    dR = dt = dq = dw = 0.0
    for seed in SEEDS[:3]:
        t, traj, bodies, _ = bs.make_session(seed, 80, (3, 5), sigma=0.0005, dropout=0.10)
        o = bs.pose_rows(traj, bodies, INF)
        for b, (rows, Q) in enumerate(bodies):
            for f in np.flatnonzero(o["flag"][b] == bs.POSED)[::9]:
                pm = [m for m in range(len(rows)) if o["present"][b, f] >> m & 1]
                ref = rbr.pose_mp([Q[m] for m in pm], [traj[rows[m], f] for m in pm])
                eR, et, _ = rbr.pose_errors(o["R"][b, f], o["t_pose"][b, f], o["rms"][b, f], ref)
                dR, dt = max(dR, eR), max(dt, et)
        rot = bs.smooth_rotations(t, o["quat"], **PAR)
        where = np.zeros(rot["flag"].shape, dtype=bool)
        where[:, ::7] = True
        mp = bs.smooth_rotations_mp(t, o["quat"], ref=rot, where=where, **PAR)
        m = np.isfinite(mp["quat_s"][:, :, 0])
        assert m.sum() >= 15 and {ts.SMOOTHED, ts.FILLED} <= set(np.unique(rot["flag"][m]))
        h = 8.0 / 120.0
        dq = max(dq, np.abs(rot["quat_s"][m] - mp["quat_s"][m]).max())
        dw = max(dw, np.abs(rot["omega"][m] - mp["omega"][m]).max() * h)
    return {"mp_pose_R": dR, "mp_pose_t": dt, "mp_quat_s": dq, "mp_omega": dw}


def test_the_float64_statement_against_its_50_digit_evaluation():
    got = measure_mp()
    for k, v in got.items():
        assert v <= bound(k), (k, v, bound(k))


# ---------------------------------------------------------------- the two smoothers
def test_translation_and_rotation_smoothers_give_the_same_flags():
    for seed in SEEDS[:3]:
        t, traj, bodies, _ = bs.make_session(seed, 300, (3, 4, 8), dropout=0.12)
        t[50], t[51] = np.nan, t[49]
        o = bs.pose_rows(traj, bodies, 0.002)
        for par in (PAR, dict(degree=1, W=1, span=INF, n_min=2, max_gap=1), dict(degree=3, W=32, span=0.1, n_min=5, max_gap=10)):
            rot = bs.smooth_rotations(t, o["quat"], **par)
            tr = ts.smooth(t, o["t_pose"], **par)
            assert np.array_equal(rot["flag"], tr["flag"]) and np.array_equal(rot["n_used"], tr["n_used"])
            assert {ts.SMOOTHED, ts.FILLED, ts.BAD_TIME} <= set(np.unique(rot["flag"]))
            fit = (rot["flag"] == ts.SMOOTHED) | (rot["flag"] == ts.FILLED)
            assert np.isfinite(rot["quat_s"][fit]).all() and np.isnan(rot["quat_s"][~fit]).all() and np.isnan(rot["omega"][~fit]).all()
            assert np.abs(np.linalg.norm(rot["quat_s"][fit], axis=1) - 1.0).max() < 1e-15


def measure():
    out = {}
    for fn in (measure_poses, measure_fill, measure_omega, measure_mp):
        out.update(fn())
    return out


if __name__ == "__main__":
    for k, v in measure().items():
        print(f'    "{k}": {v:.3g},')
