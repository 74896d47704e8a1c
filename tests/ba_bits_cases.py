"""The joint bundle adjustment and the lens calibration on a fixed list of seeded inputs, every output reduced to a SHA-256 of its
bytes: what tests/test_gpu_ba_bits.py holds the library to, bit for bit, across commits (the record: tests/golden/ba_schur_bits.json,
written by scripts/record_ba_bits.py from the library of the commit before the two solvers were given one Schur loop).  The inputs are
the smallest at which the kernels take every path: no intrinsic column and NP = 16, a partial wave with unseen views, two workgroups
(a slab fold over P = 2) with a NaN point, a point behind a camera, every state of the intrinsic column rule, and loops that reject
trials.  Nothing is stored but the digests and the counters."""
import hashlib

import numpy as np

import ba_joint_reference as bj
import ba_lens_reference as bl
from test_gpu_ba_joint import COMBOS, SHAPES as JOINT_SHAPES, _lin_input as joint_lin_input
from test_gpu_ba_lens import CASES as LENS_CASES, _lin_input as lens_lin_input

CLEAR = ("cost0", "cost", "passes", "accepted", "linearisations", "participating", "excluded", "down_weighted", "status")
TIMES = ("elapsed_ms", "device_ms")
LOOP = dict(ftol=0.0, max_iter=12)
HUBERS = (0.0, 2.0)
# (C, N, calibrated rig, focal scales as unknowns)
JOINT_LOOPS = {"2x67": (2, 67, False, False), "3x67": (3, 67, True, True), "4x257": (4, 257, False, False)}
# (C, N, flags)
LENS_LOOPS = {"3x67-all": (3, 67, bl.ALL), "4x257-fcr": (4, 257, bl.FOCAL | bl.CENTRE | bl.RADIAL), "3x67-none": (3, 67, 0)}
PROGRESS_CASE = "joint-loop/3x67/huber=2.0"     # runs with a progress callback registered


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _entry(arrays, info, digest):
    """One case's record: a digest per output array (info without its two time slots among them), the counters in the clear."""
    arrays = dict(arrays, info=np.array([float(v) for k, v in info.items() if k not in TIMES]))
    out = {"digest": {k: digest(v) for k, v in arrays.items()}}
    out.update({k: float(info[k]) for k in CLEAR})
    return out


def _loop_obs(obs):
    """The capture of a loop case; at 257 points, point 100 keeps one view only: it is excluded, its row of X_out is NaN."""
    obs = obs.copy()
    if len(obs) == 257:
        obs[100, 1:] = np.nan
    return obs


def run_cases(core, digest=sha256):
    """Every case through `core` (a MocapCore of its own: its cameras are set here) -> {case id: record}."""
    out = {}
    for name in JOINT_SHAPES:
        if name == "16x1031":
            continue
        rig, obs, start, X, fs, focal = joint_lin_input(name)
        core.set_cameras(rig["K"], start["R"], start["t"])
        for lam, hub in COMBOS:
            got = core.ba_joint_normal_eq(obs, start["R"], start["t"], X, fscale=fs, refine_focal=focal, huber_px=hub, lam=lam)
            info = dict(got["info"], cost=got["cost"])
            out[f"joint-lin/{name}/lam={lam}/huber={hub}"] = _entry({"S": got["S"], "rhs": got["rhs"], "cost": got["cost"]}, info, digest)
    for name, flags in LENS_CASES:
        if name == "16x1031":
            continue
        obs, R, t, K, dist, X = lens_lin_input(name)
        for lam, hub in COMBOS:
            got = core.ba_lens_normal_eq(obs, R, t, K, dist, X, refine=flags, huber_px=hub, lam=lam)
            info = dict(got["info"], cost=got["cost"])
            out[f"lens-lin/{name}/flags={flags}/lam={lam}/huber={hub}"] = _entry({"S": got["S"], "rhs": got["rhs"], "cost": got["cost"]}, info, digest)
    for name, (C, N, calibrated, focal) in JOINT_LOOPS.items():
        rig, obs, _, start = bj.planted_case(C, N, noise_px=0.3, calibrated=calibrated)
        obs = _loop_obs(obs)
        core.set_cameras(rig["K"], start["R"], start["t"])
        for hub in HUBERS:
            key = f"joint-loop/{name}/huber={hub}"
            seen = []
            if key == PROGRESS_CASE:
                core.set_ba_progress(lambda p: seen.append(p.copy()))
            try:
                R, t, s, X, info = core.ba_joint_solve(obs, start["R"], start["t"], refine_focal=focal, huber_px=hub, **LOOP)
            finally:
                core.set_ba_progress(None)
            arrays = {"R": R, "t": t, "fscale": s if focal else np.zeros(0), "X": X}
            if key == PROGRESS_CASE:
                arrays["progress"] = np.concatenate(seen) if seen else np.zeros(0)
            out[key] = _entry(arrays, info, digest)
    for name, (C, N, flags) in LENS_LOOPS.items():
        rig, obs, _, start = bl.planted_case(C, N, noise_px=0.3)
        obs = _loop_obs(obs)
        for hub in HUBERS:
            R, t, K, dist, X, info = core.ba_lens_solve(obs, start["R"], start["t"], start["K"], start["dist"], refine=flags, huber_px=hub, **LOOP)
            out[f"lens-loop/{name}/huber={hub}"] = _entry({"R": R, "t": t, "K": K, "dist": dist, "X": X}, info, digest)
    return out


def check_not_vacuous(rec):
    """What the record must show for the comparison to mean something (asserted on the fixture and on the library under test)."""
    for key, r in rec.items():
        if key.endswith("huber=2.0") and "-lin/" in key:
            assert r["down_weighted"] > 0, key
        if key.endswith("huber=2.0") and "-loop/" in key:
            # `down_weighted` is the count at the last accepted step: at 0.3 px of noise a converged rig has next to no view beyond
            # 2 px (the parent's library: 0 in five of the six cases, 1 in the sixth).  That the threshold acted is on record in
            # the start: a down-weighted view's share 2 h s - h^2 is below its s^2, so the first cost is below the one without Huber.
            assert r["cost0"] < rec[key.replace("huber=2.0", "huber=0.0")]["cost0"], key
        if "4x257" in key:
            assert r["excluded"] >= 1, key
        if key.startswith("lens-lin/4x257"):
            assert int(r["status"]) & bl.ST_BAD_DEPTH, key
        if "-loop/" in key:
            assert int(r["status"]) & bl.ST_MAX_ITER and r["passes"] == LOOP["max_iter"], key
    for solver in ("joint", "lens"):      # the re-linearisation after a rejected trial is on record
        assert any(r["passes"] > r["accepted"] for key, r in rec.items() if key.startswith(solver + "-loop/")), solver
