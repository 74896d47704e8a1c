"""Timing probe (GPU box): what the point refinement costs.

   python scripts/time_point_refine.py [--frames F] [--reps N] [--iters I] [--parent-lib PATH]

F resident frames (default 100 000) of the 8 x 16 bench stream, K_max 64, everything between two device events on the context's
stream, `reps` passes (default 10) after 2 warm-up passes:
(a) mocap_track_frame_dev with the mode off on this library, and -- with --parent-lib, a build of the parent commit's tree -- on
    the parent's: the two take turns, pass by pass; they should differ by noise only, since no launch is added.
(b) the same call with the mode on (`iters`, default 4): the added time, next to the staged mocap_refine_points_dev alone.
(c) the same on a calibrated rig (one K per camera), mode off and on.
The refine kernel's registers and occupancy come from the compiler (hipcc -Rpass-analysis=kernel-resource-usage).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    import time_rigid_bodies as trb
    from mocap_core import capi, synth
    dev = torch.device("cuda:0")
    C, M, K, F = 8, 16, 64, a.frames
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def report(name, v):
        print(f"{name:44s} {np.median(v):8.3f} ms per {F} frames (min {min(v):.3f} .. max {max(v):.3f}; {len(v)} passes, device events) = "
              f"{np.median(v) / F * 1e3:.4f} us per frame")
        return float(np.median(v))

    for label, rig in (("8 x 16 bench stream, one K", synth.ring_rig(C)), ("8 x 16 stream, calibrated rig (one K per camera)",
                                                                          synth.calibrated_ring_rig(C, seed=0))):
        blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
        d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
        d_xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev)
        d_err = torch.empty((F, K), dtype=torch.float64, device=dev)
        d_corr = torch.empty((F, K, C), dtype=torch.int16, device=dev)
        d_n, d_s = (torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(2))
        d_info = torch.zeros((F, K), dtype=torch.int32, device=dev)
        cores = {"this build": capi.MocapCore(0)}
        if a.parent_lib and rig["K"].std(axis=0).max() == 0:
            cores["parent build"] = trb.parent_core(a.parent_lib, capi)
        for c in cores.values():
            c.set_cameras(rig["K"], rig["R"], rig["t"])
            c.set_stream(stream)

        def live(c):
            return lambda: c.track_frame_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 22, d_xyz.data_ptr(), d_err.data_ptr(),
                                             d_corr.data_ptr(), d_n.data_ptr(), d_s.data_ptr())

        print(f"---- {label}")
        ms = {f"track_frame_dev, mode off, {k}": [] for k in cores}
        for i in range(2 + a.reps):
            for k, c in cores.items():
                t = timed(live(c))
                if i >= 2:
                    ms[f"track_frame_dev, mode off, {k}"].append(t)
        med = {k: report(k, v) for k, v in ms.items()}
        core = cores["this build"]
        off = med["track_frame_dev, mode off, this build"]
        if "parent build" in cores:
            print(f"the default against the parent: {off - med['track_frame_dev, mode off, parent build']:+.3f} ms (median - median)")
        print(f"points per frame {d_n.float().mean().item():.2f}, frames flagged {int((d_s != 0).sum().item())}, kernel {core.last_frame_kernel()}")
        # the staged call alone, on the mode-off outputs (xyz and err are overwritten with the same values every pass)
        v = []
        for i in range(2 + a.reps):
            t = timed(lambda: core.refine_points_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), K, a.iters, d_xyz.data_ptr(), d_err.data_ptr(),
                                                     d_corr.data_ptr(), d_n.data_ptr(), d_s.data_ptr(), d_info.data_ptr()))
            if i >= 2:
                v.append(t)
        report(f"refine_points_dev alone, iters {a.iters}", v)
        info = d_info.cpu().numpy()
        refined = (info & capi.RF_REFINED) != 0
        print(f"points refined {int(refined.sum())}, left alone {int(((info != 0) & ~refined).sum())}, accepted steps per refined point "
              f"{(info[refined] >> capi.RF_STEPS_SHIFT).mean():.2f}")
        core.set_point_refinement(a.iters)
        v = []
        for i in range(2 + a.reps):
            t = timed(live(core))
            if i >= 2:
                v.append(t)
        on = report(f"track_frame_dev, mode on, iters {a.iters}", v)
        print(f"added by the refinement: {on - off:+.3f} ms per {F} frames = {(on - off) / F * 1e3:+.4f} us per frame ({(on / off - 1) * 100:+.1f} %)")
        for c in cores.values():
            c.set_stream(None)
            c.close()


if __name__ == "__main__":
    main()
