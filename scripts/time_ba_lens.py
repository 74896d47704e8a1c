"""Timing probe (GPU box): what a pass of the lens calibration costs, beside the joint bundle adjustment.

   python scripts/time_ba_lens.py [--reps N] [--points 1000,65536] [--passes P] [--parent-lib PATH]

An 8-camera ring rig with planted lenses (tests/ba_lens_reference.planted_case: a raw capture that fills the images, 0.3 px noise,
start = perturbed poses, nominal K, zero coefficients), all four flags: `--passes` passes per solve (default 10, ftol 0 so that none
stops early), 2 warm-up solves, then `reps` solves (default 10).  Per solve the library reports the milliseconds between the device
events around its passes (info[10]: linearisation, Gram, camera blocks, fold, back-substitution and the waits for the host's share)
and the host clock around the whole call; both are divided by the passes made.  Printed: the median and the spread over the solves.
Next to it, in the same session, mocap_ba_joint_solve on mocap_undistort_points of the same capture under the planted lenses (the
comparison: poses and points only, a camera block of 7 and NP <= 64 against 14 and NP = 112).  With --parent-lib (a build of the
parent commit's library) both solvers run on both libraries, taking turns solve by solve, so that a drift of the machine shows in
both: the parent's figures of the same call are the yardstick, never the branch alone.
A pass is 6 launches (linearise, Gram, Gram reduce, camera blocks over 4 row bands, fold, back-substitution) and one host round trip.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def parent_core(capi, path, device_id=0):
    """A context of another build of the library: only the symbols the comparison calls are bound."""
    lib = ctypes.CDLL(path)
    for name in ("mocap_create", "mocap_destroy", "mocap_last_error", "mocap_set_cameras", "mocap_ba_joint_solve", "mocap_ba_lens_solve",
                 "mocap_undistort_points"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi.SIGNATURES[name]
    core = object.__new__(capi.MocapCore)
    h = ctypes.c_void_p()
    if lib.mocap_create(device_id, ctypes.byref(h)) != capi.MOCAP_OK:
        raise RuntimeError("mocap_create failed on the parent's library")
    core.lib, core._h, core.device_id, core.C = lib, h, device_id, 0
    return core


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", default="1000,65536")
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (the HIP runtime PyTorch ships is loaded first, as in the tests)
    import ba_lens_reference as bl
    from mocap_core import capi
    C = 8
    core = capi.MocapCore(0)
    par = parent_core(capi, a.parent_lib) if a.parent_lib else None

    def spread(v):
        return f"median {np.median(v):.4f} (min {min(v):.4f} .. max {max(v):.4f}; {len(v)} solves)"

    cores = [("branch", core)] + ([("parent", par)] if par else [])

    def turns(solve):
        """2 warm-up rounds, then `reps`: the libraries take turns solve by solve -> {library: (device ms, host ms) per pass}, last info"""
        times, info = {name: ([], []) for name, _ in cores}, None
        for i in range(2 + a.reps):
            for name, c in cores:
                info = solve(c)
                if i >= 2:
                    times[name][0].append(info["device_ms"] / info["passes"])
                    times[name][1].append(info["elapsed_ms"] / info["passes"])
        return times, info

    for N in [int(x) for x in a.points.split(",")]:
        rig, obs, _, start = bl.planted_case(C, N, noise_px=0.3)
        times, info = turns(lambda c: c.ba_lens_solve(obs, start["R"], start["t"], start["K"], start["dist"], refine=bl.ALL, ftol=0.0,
                                                      max_iter=a.passes)[5])
        print(f"lens calibration, {C} x {N}, all flags (n_c = {bl.n_cam_params(C, bl.ALL)}): {info['passes']:.0f} passes, {info['accepted']:.0f} "
              f"accepted, {info['linearisations']:.0f} linearisations, cost {info['cost0']:.1f} -> {info['cost']:.1f}")
        for name, _ in cores:
            print(f"  {name}'s library, ms per pass between device events: {spread(times[name][0])}")
            print(f"  {name}'s library, ms per pass, host clock over the whole call (set-up, upload and download included): {spread(times[name][1])}")
        ideal = core.undistort_points(obs, rig["K"], rig["dist"])
        for _, c in cores:
            c.set_cameras(rig["K"], start["R"], start["t"])
        times, info = turns(lambda c: c.ba_joint_solve(ideal, start["R"], start["t"], ftol=0.0, max_iter=a.passes)[4])
        print(f"joint BA on the undistorted capture, {C} x {N}: {info['passes']:.0f} passes, {info['accepted']:.0f} accepted")
        for name, _ in cores:
            print(f"  {name}'s library, ms per pass between device events: {spread(times[name][0])}")
            print(f"  {name}'s library, ms per pass, host clock over the whole call: {spread(times[name][1])}")
    if par:
        par.close()
    core.close()


if __name__ == "__main__":
    main()
