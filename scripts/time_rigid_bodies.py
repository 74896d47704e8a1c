"""Timing probe (GPU box): what the rigid-body stage costs.

   python scripts/time_rigid_bodies.py [--frames F] [--reps N] [--calls N] [--parent-lib PATH]

(1) Batch: the 8 x 16 bench stream (bench.py's cameras, markers, noise and dropout) with two 4-marker bodies planted in every
    frame in place of eight of its sixteen markers, F frames (default 100 000) resident on the device.  The frame kernel
    (mocap_match_triangulate_dev, K_max = 48) and mocap_locate_rigid_bodies_dev on its outputs, each between two device
    events: 2 warm-up passes, then `reps` passes, the two taking turns; printed: median, min .. max, bodies found.
    tol = 25 mm (the reference's locate_objects gate; the stream's centroids are truncated to integer pixels), max_rms = 10 mm.
(2) Live call: mocap_track_frame_bodies next to mocap_track_frame for ONE frame of that stream, host wall clock per call,
    `calls` each after 50 warm-up calls each, taking turns; with --parent-lib also mocap_track_frame of that build of the library
    (the commit before this stage) in the same process and the same rotation: the unchanged call against itself.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))

BODIES = [np.array([[0.0, 0.0, 0.0], [0.16, 0.0, 0.0], [0.0, 0.11, 0.0], [0.05, 0.04, 0.09]]),
          np.array([[0.0, 0.0, 0.0], [0.13, 0.0, 0.02], [0.02, 0.19, 0.0], [0.07, 0.06, -0.08]])]


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def planted_stream(synth, rig, F, seed=1):
    rng = np.random.default_rng(seed + 1000)

    def plant(sampled):
        out = sampled.copy()
        for b, q in enumerate(BODIES):
            R = random_rotations(rng, F)
            t = rng.uniform(-0.5, 0.5, (F, 1, 3)) + (0.6 if b else -0.6) * np.array([1.0, 0, 0])
            out[:, 4 * b:4 * b + 4] = np.einsum("fij,mj->fmi", R, q) + t
        return out
    return synth.make_blob_stream(rig, F, 16, seed=seed, world=plant)


def parent_core(path, capi):
    """A MocapCore on another build of the library that may lack the newer entry points."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in capi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    core = capi.MocapCore.__new__(capi.MocapCore)
    core.lib = lib
    h = ctypes.c_void_p()
    assert lib.mocap_create(0, ctypes.byref(h)) == 0
    core._h, core.device_id, core.C = h, 0, 0
    core._hit_cap, core._force_wide = 32, False
    return core


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    import torch
    from mocap_core import capi, synth
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    C, M, K = 8, 16, 48
    rig = synth.ring_rig(C)
    F = a.frames
    blobs, counts, _ = planted_stream(synth, rig, F)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_rigid_bodies(BODIES, tol=0.025, max_rms=0.010)

    # ---- (2) live call, one frame
    b1, c1 = blobs[:1], counts[:1]
    fns = [("track_frame", lambda: core.track_frame(b1, c1, K_max=K, O_max=8)),
           ("track_frame_bodies", lambda: core.track_frame_bodies(b1, c1, K_max=K, O_max=8))]
    if a.parent_lib:
        old = parent_core(a.parent_lib, capi)
        old.set_cameras(rig["K"], rig["R"], rig["t"])
        fns.append(("track_frame (parent build)", lambda: old.track_frame(b1, c1, K_max=K, O_max=8)))
    for _ in range(50):
        for _, fn in fns:
            fn()
    ts = {name: [] for name, _ in fns}
    for _ in range(a.calls):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    for k, v in ts.items():
        print(f"{k:28s} {med[k]:.4f} ms per call (5th .. 95th percentile {np.percentile(v, 5):.4f} .. {np.percentile(v, 95):.4f}; "
              f"{len(v)} calls, host wall clock, Python binding included)")
    print(f"added by the rigid-body stage {med['track_frame_bodies'] - med['track_frame']:.4f} ms per call")
    one = core.track_frame_bodies(b1, c1, K_max=K, O_max=8)
    print("the frame:", int(one["n_pts"][0]), "points, bodies found", one["found"][0].tolist(), "rms", one["rms"][0].tolist())

    # ---- (1) batch on resident frames
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    d_xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev)
    d_err = torch.empty((F, K), dtype=torch.float64, device=dev)
    d_corr = torch.empty((F, K, C), dtype=torch.int16, device=dev)
    d_n, d_s, d_g = (torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(3))
    B = len(BODIES)
    o = {"found": torch.zeros((F, B), dtype=torch.int32, device=dev), "n_used": torch.zeros((F, B), dtype=torch.int32, device=dev),
         "assign": torch.zeros((F, B, 8), dtype=torch.int8, device=dev), "R": torch.zeros((F, B, 9), dtype=torch.float64, device=dev),
         "t": torch.zeros((F, B, 3), dtype=torch.float64, device=dev), "rms": torch.zeros((F, B), dtype=torch.float64, device=dev),
         "score": torch.zeros((F, B), dtype=torch.float64, device=dev), "status": torch.zeros((F, B), dtype=torch.int32, device=dev)}
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def frame_pass():
        core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 22, d_xyz.data_ptr(), d_err.data_ptr(),
                                   d_corr.data_ptr(), d_n.data_ptr(), d_s.data_ptr(), d_g.data_ptr())

    def body_pass():
        core.locate_rigid_bodies_dev(F, K, d_xyz.data_ptr(), d_n.data_ptr(), B, *[o[k].data_ptr() for k in
                                                                                   ("found", "n_used", "assign", "R", "t", "rms", "score", "status")])
    ms = {"frame kernel": [], "rigid bodies": []}
    for i in range(2 + a.reps):
        for name, fn in (("frame kernel", frame_pass), ("rigid bodies", body_pass)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms[name].append(e0.elapsed_time(e1))
    n = d_n.cpu().numpy()
    print(f"stream: {F} frames, points per frame mean {n.mean():.2f} (min {n.min()}, max {n.max()}), frames flagged {int((d_s != 0).sum().item())}, "
          f"kernel {core.last_frame_kernel()}")
    for name, v in ms.items():
        print(f"{name:14s} {np.median(v):.3f} ms per {F} frames (min {min(v):.3f} .. max {max(v):.3f}; {len(v)} passes, device events) = "
              f"{np.median(v) / F * 1e3:.4f} us per frame")
    found = o["found"].cpu().numpy()
    st = o["status"].cpu().numpy()
    print(f"bodies found {found.mean(axis=0).round(4).tolist()} of the frames, rms-rejected {int((st == capi.RB_ST_RMS).sum())}, "
          f"work-capped {int((st == capi.RB_ST_WORK_CAP).sum())}, mean rms of the found {float(o['rms'][o['found'] == 1].mean().item()) * 1e3:.3f} mm")
    core.close()


if __name__ == "__main__":
    main()
