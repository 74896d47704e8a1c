"""Timing probe (GPU box): what the point consolidation costs, and what it does to the rigid bodies.

   python scripts/time_point_consolidate.py [--frames F] [--reps N] [--calls N] [--parent-lib PATH]

(a) Batch: F resident frames (default 100 000) of the 8 x 16 bench stream, K_max 128: mocap_consolidate_points_dev between two
    device events, `reps` passes (default 10) after 2 warm-up passes, the input restored from a device copy outside the timed
    region before every pass; next to it the frame kernel (mocap_match_triangulate_dev) on the same frames.  Printed: median,
    min .. max, microseconds per frame, the bytes the stage has to move and the time they take at 4 TB/s.
(b) Live call: mocap_track_frame, ONE frame per call, host wall clock, `calls` (default 1 000) after 50 warm-up calls each, taking
    turns in one process: the mode off against the parent commit's library (--parent-lib: a build of the parent's tree), then the
    mode on against the mode off on this library.
(c) Rigid bodies: the two-planted-bodies stream of scripts/time_rigid_bodies.py (its registration: tol 0.025, max_rms 0.010),
    found rates and rms rejections with the mode off and on.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    import time_rigid_bodies as trb
    from mocap_core import capi, synth
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    C, M, K = 8, 16, 128
    rig = synth.ring_rig(C)
    F = a.frames
    core.set_cameras(rig["K"], rig["R"], rig["t"])

    # ---- (a) batch on resident frames
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    d_xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev)
    d_err = torch.empty((F, K), dtype=torch.float64, device=dev)
    d_corr = torch.empty((F, K, C), dtype=torch.int16, device=dev)
    d_n, d_s, d_g, d_nin = (torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(4))
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def frame_pass():
        core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 22, d_xyz.data_ptr(), d_err.data_ptr(),
                                   d_corr.data_ptr(), d_n.data_ptr(), d_s.data_ptr(), d_g.data_ptr())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {"frame kernel": [], "consolidation": []}
    for i in range(2 + a.reps):
        t = timed(frame_pass)
        if i >= 2:
            ms["frame kernel"].append(t)
    keep = [x.clone() for x in (d_xyz, d_err, d_corr, d_n)]
    for i in range(2 + a.reps):
        for dst, src in zip((d_xyz, d_err, d_corr, d_n), keep):      # restore: outside the timed region
            dst.copy_(src)
        torch.cuda.synchronize()
        t = timed(lambda: core.consolidate_points_dev(F, K, d_xyz.data_ptr(), d_err.data_ptr(), d_corr.data_ptr(), d_n.data_ptr(),
                                                      d_s.data_ptr(), 0, d_nin.data_ptr()))
        if i >= 2:
            ms["consolidation"].append(t)
    core.set_stream(None)
    n_in, n_out = keep[3].cpu().numpy(), d_n.cpu().numpy()
    print(f"stream: {F} frames of 8 x 16, K_max {K}; points per frame {n_in.mean():.2f} -> {n_out.mean():.2f}, frames flagged "
          f"{int((d_s != 0).sum().item())}, frames not processed {int((d_nin < 0).sum().item())}, kernel {core.last_frame_kernel()}")
    for name, v in ms.items():
        print(f"{name:14s} {np.median(v):.3f} ms per {F} frames (min {min(v):.3f} .. max {max(v):.3f}; {len(v)} passes, device events) = "
              f"{np.median(v) / F * 1e3:.4f} us per frame")
    # what the stage has to touch: the rows it reads (corr, err, xyz of n_in points, two words per frame) and those it writes
    moved = float((n_in * (2 * C + 32) + n_out * (2 * C + 32)).sum() + 12 * F)
    print(f"bytes read and written {moved / 1e6:.1f} MB = {moved / F:.0f} per frame: {moved / 4e12 * 1e3:.4f} ms at 4 TB/s; the stage takes "
          f"{np.median(ms['consolidation']) / (moved / 4e12 * 1e3):.1f} x that")

    # ---- (b) live call, one frame per call
    Kl = 48
    N = 50 + a.calls

    def live(pairs):
        ts = {name: [] for name, _ in pairs}
        for f in range(N):
            for name, fn in pairs:
                t0 = time.perf_counter()
                fn(f % min(F, 1024))
                if f >= 50:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        for k, v in ts.items():
            print(f"{k:34s} p50 {np.median(v):.4f} ms per call (5th .. 95th percentile {np.percentile(v, 5):.4f} .. "
                  f"{np.percentile(v, 95):.4f}; {len(v)} calls, host wall clock, Python binding included)")
        return {k: float(np.median(v)) for k, v in ts.items()}

    call = lambda c: (lambda f: c.track_frame(blobs[f:f + 1], counts[f:f + 1], K_max=Kl, O_max=8))   # noqa: E731
    if a.parent_lib:
        old = trb.parent_core(a.parent_lib, capi)
        old.set_cameras(rig["K"], rig["R"], rig["t"])
        med = live([("track_frame, mode off", call(core)), ("track_frame, parent build", call(old))])
        print(f"the default against the parent: {med['track_frame, mode off'] - med['track_frame, parent build']:+.4f} ms per call (p50 - p50)")
    on = capi.MocapCore(0)
    on.set_cameras(rig["K"], rig["R"], rig["t"])
    on.set_point_consolidation(capi.CONSOLIDATE_BLOBS)
    med = live([("track_frame, mode off", call(core)), ("track_frame, mode on", call(on))])
    print(f"added by the consolidation {med['track_frame, mode on'] - med['track_frame, mode off']:+.4f} ms per call (p50 - p50)")
    on.close()

    # ---- (c) rigid bodies on the two-planted-bodies stream, off and on
    Fb, Kb, B = min(F, 20_000), 48, len(trb.BODIES)
    blobs, counts, _ = trb.planted_stream(synth, rig, Fb)
    core.set_rigid_bodies(trb.BODIES, tol=0.025, max_rms=0.010)
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    shapes = {"xyz": ((Fb, Kb, 3), torch.float64), "err": ((Fb, Kb), torch.float64), "corr": ((Fb, Kb, C), torch.int16),
              "n_pts": ((Fb,), torch.int32), "status": ((Fb,), torch.int32), "found": ((Fb, B), torch.int32),
              "n_used": ((Fb, B), torch.int32), "assign": ((Fb, B, 8), torch.int8), "R": ((Fb, B, 9), torch.float64),
              "t": ((Fb, B, 3), torch.float64), "rms": ((Fb, B), torch.float64), "score": ((Fb, B), torch.float64),
              "rb_status": ((Fb, B), torch.int32)}
    for mode in (capi.CONSOLIDATE_OFF, capi.CONSOLIDATE_BLOBS):
        core.set_point_consolidation(mode)
        d = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        torch.cuda.synchronize()
        core.track_frame_bodies_dev(Fb, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, Kb, 1 << 22,
                                    *[d[k].data_ptr() for k in ("xyz", "err", "corr", "n_pts", "status")], 0, 0, 0, 0, 0, 0, B,
                                    *[d[k].data_ptr() for k in ("found", "n_used", "assign", "R", "t", "rms", "score", "rb_status")])
        core.synchronize()
        found, st = d["found"].cpu().numpy(), d["rb_status"].cpu().numpy()
        rms = d["rms"][d["found"] == 1]
        print(f"rigid bodies, mode {'on ' if mode else 'off'}: {Fb} frames, points per frame {d['n_pts'].float().mean().item():.2f}, bodies found "
              f"{found.mean(axis=0).round(4).tolist()} of the frames, rms-rejected {int((st == capi.RB_ST_RMS).sum())}, work-capped "
              f"{int((st == capi.RB_ST_WORK_CAP).sum())}, mean rms of the found {float(rms.mean().item()) * 1e3 if rms.numel() else float('nan'):.3f} mm")
    core.close()


if __name__ == "__main__":
    main()
