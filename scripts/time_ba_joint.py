"""Timing probe (GPU box): what a pass of the joint bundle adjustment costs.

   python scripts/time_ba_joint.py [--reps N] [--points 1000,100000] [--passes P]

An 8-camera ring rig, 0.3 px noise, poses from synth.perturb_rig; `--passes` passes per solve (default 10, ftol 0 so that none stops
early), 2 warm-up solves, then `reps` solves (default 10).  Per solve the library reports the milliseconds between the device events
around its passes (info[10]: linearisation, Gram, camera blocks, fold, back-substitution and the waits for the host's share) and the
host clock around the whole call; both are divided by the passes made.  Printed: the median and the spread over the solves.
Next to it mocap_ba_solve (the reference's algorithm, resident; its code is the parent commit's, this change does not touch it) on the
same 8 x 1 000 input: elapsed milliseconds per iteration.
A pass is 6 launches (linearise, Gram, Gram reduce, camera blocks, fold, back-substitution) and one host round trip.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", default="1000,100000")
    ap.add_argument("--passes", type=int, default=10)
    a = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime PyTorch ships is loaded first, as in the tests)
    from scipy.spatial.transform import Rotation
    from mocap_core import capi, synth
    C = 8
    rig = synth.ring_rig(C)
    start = synth.perturb_rig(rig, np.random.default_rng(1))
    core = capi.MocapCore(0)
    core.set_cameras(rig["K"], start["R"], start["t"])

    def spread(v):
        return f"median {np.median(v):.4f} (min {min(v):.4f} .. max {max(v):.4f}; {len(v)} solves)"

    for N in [int(x) for x in a.points.split(",")]:
        obs, _ = synth.make_ba_observations(rig, N, seed=6, noise_px=0.3)
        dev, wall, info = [], [], None
        for i in range(2 + a.reps):
            info = core.ba_joint_solve(obs, start["R"], start["t"], ftol=0.0, max_iter=a.passes)[4]
            if i >= 2:
                dev.append(info["device_ms"] / info["passes"])
                wall.append(info["elapsed_ms"] / info["passes"])
        print(f"joint BA, {C} x {N}: {info['passes']:.0f} passes, {info['accepted']:.0f} accepted, {info['linearisations']:.0f} linearisations, "
              f"cost {info['cost0']:.1f} -> {info['cost']:.1f}")
        print(f"  ms per pass between device events: {spread(dev)}")
        print(f"  ms per pass, host clock over the whole call (set-up, upload and download included): {spread(wall)}")
    obs, _ = synth.make_ba_observations(rig, 1000, seed=6, noise_px=0.3)
    x0 = [rig["K"][0][0, 0]]
    for c in range(1, C):
        x0 += [rig["K"][c][0, 0]] + Rotation.from_matrix(start["R"][c]).as_rotvec().tolist() + start["t"][c].tolist()
    per = []
    for i in range(2 + a.reps):
        _, info = core.ba_solve(np.array(x0), obs, ftol=1e-2, f32_residuals=True, use_cauchy=True)
        if i >= 2:
            per.append(info["elapsed_ms"] / max(info["iterations"], 1))
    print(f"mocap_ba_solve (resident), {C} x 1000: {info['iterations']:.0f} iterations, {info['nfev']:.0f} evaluations")
    print(f"  ms per iteration, host clock over the whole call: {spread(per)}")
    core.close()


if __name__ == "__main__":
    main()
