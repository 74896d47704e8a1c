"""Timing probe (GPU box): what one camera resection costs.

   python scripts/time_resection.py [--reps N] [--shapes 1031x257,100000x4096]

One camera with a planted pose (tests/resection_reference.planted_case: 20 % of the views moved by 20 .. 50 px, 0.3 px noise), X and
obs already on the device, the context on a stream of PyTorch's so that device events can be recorded around one
mocap_resect_camera_dev call: 2 warm-up calls, then `reps` calls (default 10).  Printed per shape (rows x hypotheses): the median and
the spread of the milliseconds between the events for
  full       the whole call (search, two rounds of refinement with their host round trips, finish)
  search     max_iter = 0: compaction, hypotheses, scoring, winner, finish -- no refinement
  evaluate   n_hyp = 0, max_iter = 0 with the planted pose as the prior: compaction, one candidate, finish
and the scoring kernel's share of the full call ESTIMATED as (search - evaluate) / full: what the hypotheses and their scoring add to
a call that does neither.  It is a difference of event times, not a profiler's per-kernel figure, and it contains the three-point
solver's launch.  The call waits for the device several times (once per linearisation), so the event times contain the host's share.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="1031x257,100000x4096")
    a = ap.parse_args()
    import torch
    from mocap_core import capi
    import resection_reference as rr
    core = capi.MocapCore(0)
    stream = torch.cuda.Stream()
    core.set_stream(stream.cuda_stream)

    def spread(v):
        return f"median {np.median(v):.4f} ms (min {min(v):.4f} .. max {max(v):.4f}; {len(v)} calls)"

    for shape in a.shapes.split(","):
        N, H = (int(x) for x in shape.split("x"))
        c = rr.planted_case(N, outliers=0.2, noise=0.3, seed=3)
        d_X = torch.from_numpy(np.ascontiguousarray(c["X"])).cuda()
        d_obs = torch.from_numpy(np.ascontiguousarray(c["obs"])).cuda()
        torch.cuda.synchronize()
        modes = {"full": dict(n_hyp=H, max_iter=20), "search": dict(n_hyp=H, max_iter=0),
                 "evaluate": dict(n_hyp=0, max_iter=0, prior=(c["R"], c["t"]))}
        med, info = {}, None
        for mode, kw in modes.items():
            ms = []
            for i in range(2 + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                out = core.resect_camera_dev(N, d_X.data_ptr(), d_obs.data_ptr(), c["K"], threshold_px=2.0, seed=7, min_inliers=8, **kw)
                e1.record(stream)
                e1.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
                if mode == "full":
                    info = out[3]
            med[mode] = float(np.median(ms))
            print(f"resection {N} rows x {H} hypotheses, {mode:8s}: {spread(ms)}")
        print(f"  full: {info['inliers']} inliers of {info['valid']} rows, {info['accepted']} steps, {info['linearisations']} linearisations, "
              f"rms {info['rms_winner']:.3f} -> {info['rms_final']:.3f} px; hypotheses + scoring (search - evaluate) = "
              f"{med['search'] - med['evaluate']:.4f} ms = {100.0 * (med['search'] - med['evaluate']) / med['full']:.1f} % of the full call")
    core.close()


if __name__ == "__main__":
    main()
