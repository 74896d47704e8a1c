"""Timing probe (GPU box): what the object filter costs.

   python scripts/time_object_filter.py [--calls N] [--frames F] [--reps N]

(1) Live call: mocap_track_frame_filtered next to mocap_track_frame for ONE frame (the frame with the most objects of
    tests/golden/track_apptsx_chain.npz, the reference UI's rig), host wall clock per call.  The two take turns, `calls` each
    after 50 warm-up calls each; printed: the medians, their difference (the filter's two kernels behind the export) and the
    spread of each (5th .. 95th percentile).
(2) Recorded session: mocap_filter_objects_dev over `frames` frames (default 100 000) with 2 drones, each present with a decoy
    0.3 m away, inputs resident on the device, between two device events: 2 warm-up passes, then `reps` passes; printed: median,
    min .. max.  One pass is a `frames`-step dependent chain in one wave per drone plus frames x 2 x 4 independent dot products.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))


def session(F, seed=1):
    rng = np.random.default_rng(seed)
    t = 1.7e9 + np.cumsum(rng.uniform(0.012, 0.022, F))
    s = t - t[0]
    pos = np.zeros((F, 4, 3))
    pos[:, 0] = np.stack([np.cos(0.8 * s), np.sin(0.8 * s), 1.0 + 0.2 * np.sin(0.5 * s)], axis=1)
    pos[:, 1] = np.stack([-0.5 + 0.6 * np.sin(0.6 * s), 0.3 + 0.4 * np.sin(0.9 * s), 0.8 + 0.1 * np.cos(0.7 * s)], axis=1)
    pos[:, 2] = pos[:, 0] + [0.0, 0.3, 0.0]
    pos[:, 3] = pos[:, 1] + [0.3, 0.0, 0.0]
    pos += rng.normal(0.0, 1e-3, pos.shape)
    heading = np.stack([0.9 * np.sin(0.4 * s), 0.7 * np.cos(0.3 * s), 0.2 + 0 * s, 0.1 + 0 * s], axis=1)
    drone = np.tile(np.array([0, 1, 0, 1], dtype=np.int32), (F, 1))
    return t, pos, heading, drone, np.full(F, 4, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    from mocap_core import capi
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)

    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "track_apptsx_chain.npz")))
    core.set_cameras(g["K"], g["R"], g["t"])
    core.set_world_transform(g["to_world"])
    core.set_object_filter(2)
    f = int(np.argmax(g["ref_nobj"]))
    blobs, counts = g["blobs"][f:f + 1], g["counts"][f:f + 1]
    now = [1.7e9]

    def plain():
        core.track_frame(blobs, counts, K_max=48, O_max=8)

    def filtered():
        now[0] += 1 / 60.0
        core.track_frame_filtered(blobs, counts, now, K_max=48, O_max=8)
    for _ in range(50):
        plain()
        filtered()
    ts = {"track_frame": [], "track_frame_filtered": []}
    for _ in range(a.calls):
        for name, fn in (("track_frame", plain), ("track_frame_filtered", filtered)):
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    for k, v in ts.items():
        print(f"{k:22s} {med[k]:.4f} ms per call (5th .. 95th percentile {np.percentile(v, 5):.4f} .. {np.percentile(v, 95):.4f}; {len(v)} calls, "
              "host wall clock, Python binding included)")
    print(f"added by the filter     {med['track_frame_filtered'] - med['track_frame']:.4f} ms per call")

    F = a.frames
    t, pos, heading, drone, n_obj = (torch.from_numpy(x).to(dev) for x in session(F))
    fpos, fvel = (torch.empty((F, 2, 3), dtype=torch.float32, device=dev) for _ in range(2))
    fhead = torch.empty((F, 2), dtype=torch.float64, device=dev)
    chosen = torch.empty((F, 2), dtype=torch.int32, device=dev)
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def run():
        core.filter_objects_dev(F, t.data_ptr(), 4, pos.data_ptr(), heading.data_ptr(), drone.data_ptr(), n_obj.data_ptr(),
                                fpos.data_ptr(), fvel.data_ptr(), fhead.data_ptr(), chosen.data_ptr())
    ms = []
    for i in range(2 + a.reps):
        core.set_object_filter(2)      # every pass is the same session from a fresh state
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    assert int((chosen >= 0).sum().item()) == 2 * F
    print(f"mocap_filter_objects_dev {np.median(ms):.2f} ms per {F} frames x 2 drones (min {min(ms):.2f} .. max {max(ms):.2f}; {len(ms)} passes, "
          f"device events) = {np.median(ms) / F * 1e3:.3f} us per frame")
    core.close()


if __name__ == "__main__":
    main()
