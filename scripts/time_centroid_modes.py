#!/usr/bin/env python3
"""What the sub-pixel centroid mode costs: mocap_find_blobs_dev over 8 192 images resident in HBM
(1 024 frame sets of 8 synthetic PS3-Eye cameras), reference mode and weighted mode alternating on one binary, HIP-event
timing, warmed up in both modes first.  One JSON line: every run, the median and the spread (max - min) per mode.
    python scripts/time_centroid_modes.py [--frames 1024] [--steps 10]
MOCAP_CORE_LIB=<another build> times that build; one from before the mode existed is timed in reference mode alone, which
gives the figure the default mode has to stay inside -- repeat the command to get that build's own run-to-run spread."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
import torch  # noqa: E402
from mocap_core import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--markers", type=int, default=16)
    args = ap.parse_args()
    has_mode = hasattr(ctypes.CDLL(capi.LIB_PATH), "mocap_set_centroid_mode")
    if not has_mode:
        capi.SIGNATURES.pop("mocap_set_centroid_mode")
    C, M_max, F = args.cams, 32, args.frames
    rig = synth.ring_rig(C)
    images, _ = synth.render_camera_frames(rig, args.distinct, args.markers, seed=1)
    dev = torch.device("cuda", 0)
    core = capi.MocapCore(0)
    core.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * C)
    stream = torch.cuda.current_stream(dev)
    core.set_stream(stream.cuda_stream)
    d_img = torch.from_numpy(images).to(dev).repeat((F + args.distinct - 1) // args.distinct, 1, 1, 1, 1)[:F].contiguous()
    d_blobs = torch.zeros((F, C, M_max, 2), dtype=torch.float32, device=dev)
    d_counts = torch.zeros((F, C), dtype=torch.int32, device=dev)
    d_st = torch.zeros((F, C), dtype=torch.int32, device=dev)
    modes = (capi.CENTROID_REFERENCE, capi.CENTROID_WEIGHTED) if has_mode else (capi.CENTROID_REFERENCE,)

    def run(mode):
        if has_mode:
            core.set_centroid_mode(mode)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        core.find_blobs_dev(F, d_img.data_ptr(), M_max, d_blobs.data_ptr(), d_counts.data_ptr(), d_st.data_ptr())
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    checks = {}
    for mode in modes:                 # warm-up: code objects, workspaces
        run(mode)
        run(mode)
        checks[mode] = float(d_blobs.double().sum().item())
    ts = {mode: [] for mode in modes}
    for _ in range(args.steps):
        for mode in modes:
            ts[mode].append(run(mode))
    out = {"library": capi.LIB_PATH, "images": F * C, "points": int(d_counts.sum().item()), "status_nonzero": int((d_st != 0).sum().item())}
    for mode in modes:
        name = "weighted" if mode else "reference"
        out[name] = {"median_ms": float(np.median(ts[mode])), "spread_ms": float(max(ts[mode]) - min(ts[mode])),
                     "runs_ms": [round(t, 4) for t in ts[mode]], "coordinate_sum": checks[mode]}
    if has_mode:
        out["weighted_over_reference"] = out["weighted"]["median_ms"] / out["reference"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
