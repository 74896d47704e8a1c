"""Timing probe (GPU box): what a pass of the joint bundle adjustment costs.

   python scripts/time_ba_joint.py [--reps N] [--points 1000,100000] [--passes P] [--parent-lib PATH]

An 8-camera ring rig, 0.3 px noise, poses from synth.perturb_rig; `--passes` passes per solve (default 10, ftol 0 so that none stops
early), 2 warm-up solves, then `reps` solves (default 10).  Per solve the library reports the milliseconds between the device events
around its passes (info[10]: linearisation, Gram, camera blocks, fold, back-substitution and the waits for the host's share) and the
host clock around the whole call; both are divided by the passes made.  Printed: the median and the spread over the solves.
With --parent-lib (a build of the parent commit's library) the solves run on both libraries, taking turns solve by solve, so that a
drift of the machine shows in both: the parent's figures of the same call are the yardstick, never the branch alone.
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
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime PyTorch ships is loaded first, as in the tests)
    from scipy.spatial.transform import Rotation
    from mocap_core import capi, synth
    from time_ba_lens import parent_core
    C = 8
    rig = synth.ring_rig(C)
    start = synth.perturb_rig(rig, np.random.default_rng(1))
    core = capi.MocapCore(0)
    par = parent_core(capi, a.parent_lib) if a.parent_lib else None
    cores = [("branch", core)] + ([("parent", par)] if par else [])
    for _, c in cores:
        c.set_cameras(rig["K"], start["R"], start["t"])

    def spread(v):
        return f"median {np.median(v):.4f} (min {min(v):.4f} .. max {max(v):.4f}; {len(v)} solves)"

    for N in [int(x) for x in a.points.split(",")]:
        obs, _ = synth.make_ba_observations(rig, N, seed=6, noise_px=0.3)
        times, info = {name: ([], []) for name, _ in cores}, None
        for i in range(2 + a.reps):
            for name, c in cores:          # taking turns
                info = c.ba_joint_solve(obs, start["R"], start["t"], ftol=0.0, max_iter=a.passes)[4]
                if i >= 2:
                    times[name][0].append(info["device_ms"] / info["passes"])
                    times[name][1].append(info["elapsed_ms"] / info["passes"])
        print(f"joint BA, {C} x {N}: {info['passes']:.0f} passes, {info['accepted']:.0f} accepted, {info['linearisations']:.0f} linearisations, "
              f"cost {info['cost0']:.1f} -> {info['cost']:.1f}")
        for name, _ in cores:
            print(f"  {name}'s library, ms per pass between device events: {spread(times[name][0])}")
            print(f"  {name}'s library, ms per pass, host clock over the whole call (set-up, upload and download included): {spread(times[name][1])}")
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
    if par:
        par.close()
    core.close()


if __name__ == "__main__":
    main()
