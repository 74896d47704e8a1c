"""Timing probe (GPU box): what the marker tracker costs.

   python scripts/time_marker_track.py [--frames F] [--reps N] [--calls N] [--round-frames R]

(1) Batch: mocap_track_markers_dev over F frames (default 10 000) of the planted scenes of tests/marker_track_reference.py,
    (markers, K_max, clutter) = (20, 32, 3) and (40, 64, 3), generated at that length (60 Hz, the same paths, noise, occlusions
    and clutter as the tests' 96 frames), resident on the device; gate 0.05, max_missed 5, vel_alpha 0.5, T_max 64.  2 warm-up
    passes, then `reps` passes (default 7), each from a reset state and between two device events; printed: median,
    min .. max, microseconds per frame.  The association rounds per frame are counted by the reference's statement of the rounds
    (the kernel keeps no counter) over the first R frames (default: all), whose ids the device must reproduce.
(2) Live call: mocap_track_frame_ids next to mocap_track_frame, ONE frame of the 8 x 16 synthetic stream per call (its sixteen
    markers drifting slowly; sub-pixel blobs, so that the tracker matches them), host wall clock per call, `calls` (default
    1 000) each after 50 warm-up calls each, taking turns in one process; printed: p50 and the 5th .. 95th percentile.
(3) How many of those markers keep their id over 300 frames: on that stream, and on the stream as bench.py makes it (integer
    pixels, 0.3 px noise, 5 % dropout), where the frame path returns some markers twice and some points centimetres off.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--round-frames", type=int, default=10_000)
    a = ap.parse_args()
    import torch
    import marker_track_reference as mt
    from mocap_core import capi, synth
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    F = a.frames

    # ---- (1) batch on resident frames
    for markers, K_max, clutter, seed in ((20, 32, 3, 1), (40, 64, 3, 11)):
        t, xyz, n_pts, truth = mt.planted_scene(markers, K_max, clutter, seed, n_frames=F)
        d_t, d_xyz, d_n = (torch.from_numpy(x).to(dev) for x in (t, xyz, n_pts))
        o = [torch.zeros(s, dtype=torch.int32, device=dev) for s in ((F, K_max), (F, K_max), (F,), (F,))]
        core.set_marker_tracker(**mt.DEFAULTS)
        core.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ms = []
        for i in range(2 + a.reps):
            core.reset_marker_tracker()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            core.track_markers_dev(F, d_t.data_ptr(), K_max, d_xyz.data_ptr(), d_n.data_ptr(), *[x.data_ptr() for x in o])
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        core.set_stream(None)
        ids, n_tracks, status = o[0].cpu().numpy(), o[2].cpu().numpy(), o[3].cpu().numpy()
        R = min(a.round_frames, F)
        ref = mt.Tracker(associate=mt.associate_rounds, **mt.DEFAULTS)
        want = ref.run(t[:R], xyz[:R], n_pts[:R])
        assert np.array_equal(want["id"], ids[:R]) and np.array_equal(want["n_tracks"], n_tracks[:R]), "device and reference disagree"
        rounds = np.array(ref.rounds)
        print(f"scene ({markers}, {K_max}, {clutter}): {F} frames, points per frame mean {n_pts.mean():.1f}, live tracks mean {n_tracks.mean():.1f} "
              f"(max {n_tracks.max()}), frames FULL {int((status & capi.MT_ST_FULL).sum())}, markers that changed id "
              f"{mt.id_switches(ids, truth)}")
        print(f"  mocap_track_markers_dev {np.median(ms):.3f} ms per {F} frames (min {min(ms):.3f} .. max {max(ms):.3f}; {len(ms)} passes, "
              f"device events) = {np.median(ms) / F * 1e3:.3f} us per frame")
        print(f"  association rounds per frame over the first {R} frames: mean {rounds.mean():.3f}, max {rounds.max()}, "
              f"frames with more than one {int((rounds > 1).sum())}")

    # ---- (2) live call, one frame per call
    C, M, K = 8, 16, 48
    rig = synth.ring_rig(C)
    N = 50 + a.calls
    drift = lambda s: s[:1] + 0.05 * np.sin(np.arange(len(s))[:, None, None] / 60.0 * np.array([2.0, 3.0, 4.0]))   # noqa: E731
    clean = dict(noise_px=0.02, dropout=0.0, truncate=False)
    blobs, counts, _ = synth.make_blob_stream(rig, N, 16, seed=1, min_sep=0.15, world=drift, **clean)
    stamps = 50.0 + np.arange(N) / 60.0
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_marker_tracker(**mt.DEFAULTS)
    fns = [("track_frame", lambda f: core.track_frame(blobs[f:f + 1], counts[f:f + 1], K_max=K, O_max=8)),
           ("track_frame_ids", lambda f: core.track_frame_ids(blobs[f:f + 1], counts[f:f + 1], stamps[f:f + 1], K_max=K, O_max=8))]
    ts = {name: [] for name, _ in fns}
    for f in range(N):
        for name, fn in fns:
            t0 = time.perf_counter()
            res = fn(f)
            if f >= 50:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    for k, v in ts.items():
        print(f"{k:16s} p50 {np.median(v):.4f} ms per call (5th .. 95th percentile {np.percentile(v, 5):.4f} .. {np.percentile(v, 95):.4f}; "
              f"{len(v)} calls, host wall clock, Python binding included)")
    print(f"added by the marker tracker {np.median(ts['track_frame_ids']) - np.median(ts['track_frame']):.4f} ms per call (p50 - p50); "
          f"last frame: {int(res['n_pts'][0])} points, {int(res['n_tracks'][0])} live tracks")

    # ---- (3) what the frame path's own points do to the identities: 300 frames of that stream, clean and as bench.py makes it
    for name, kw in (("sub-pixel blobs, 0.02 px noise, no dropout", clean), ("bench.py's blobs: integer pixels, 0.3 px noise, 5 % dropout", {})):
        blobs, counts, _ = synth.make_blob_stream(rig, 300, 16, seed=1, min_sep=0.15, world=drift, **kw)
        core.set_marker_tracker(**mt.DEFAULTS)
        res = core.track_frame_ids(blobs, counts, stamps[:300], K_max=K, O_max=0)
        last = res["hits"][-1][:res["n_pts"][-1]]
        print(f"{name}: points per frame mean {res['n_pts'].mean():.2f} for 16 markers, ids handed out {int(res['id'].max()) + 1}, tracks of the last "
              f"frame seen in >= 290 of the 300 frames: {int((last >= 290).sum())}, in > 150: {int((last > 150).sum())}")
    core.close()


if __name__ == "__main__":
    main()
