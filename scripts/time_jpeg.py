"""Timing probe (GPU box): what the preview stream costs the one-call live loop.

   python scripts/time_jpeg.py [--calls N] [--cameras C] [--frame-sets 1,64]

For 8 cameras x 320 x 320 (raw 240 x 320 frames of the synthetic ring rig, dots on black) and every batch size asked for,
four routes take turns, `calls` each after 10 warm-up calls each, host wall clock per call (Python binding included):
  track_frame_images        the chained call without the stream
  track_frame_images_jpeg   the same with the JPEG of the processed frames in its payload (quality 95)
  ... with overlays         the same call with mocap_set_preview_overlay(7): contours, centre marks and epipolar lines painted
                            into the frames before the encoder (the option is set outside the timed window)
  today's route             track_frame_images, then find_blobs(want_processed=True) to bring `processed` to the host
                            (a second blob pass: the chained call has no `processed` output), then PIL's encoder on one core
                            as the stand-in for cv.imencode -- reported split into download and encode
Printed: the median of each, 5th .. 95th percentile, what the JPEG adds to the chained call, what the download alone costs, and
the bytes that cross PCIe either way, under the hash of the library sources the figures belong to.  PIL missing: the encode column is skipped and says so.
"""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--frame-sets", default="1,64")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as everywhere)
    from mocap_core import capi, synth
    try:
        from PIL import Image
    except ImportError:
        Image = None
    import bench
    core = capi.MocapCore(0)
    C = a.cameras
    print(f"library sources {bench.kernel_source_hash()} (bench.kernel_source_hash)")
    rig = synth.ring_rig(C)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * C)
    for F in (int(x) for x in a.frame_sets.split(",")):
        images, _ = synth.render_camera_frames(rig, F, 6, seed=9)
        kw = dict(M_max=16, O_max=4)
        sizes = {}

        def plain():
            core.track_frame_images(images, **kw)

        def with_jpeg():
            sizes["jpeg"] = core.track_frame_images_jpeg(images, quality=95, **kw)["jpeg_size"]

        def with_overlays():
            sizes["overlay"] = core.track_frame_images_jpeg(images, quality=95, **kw)["jpeg_size"]

        def download():
            return core.find_blobs(images, M_max=16, want_processed=True)["processed"]

        def pil_encode(proc):
            for f in range(F):
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(np.hstack(list(proc[f]))[..., ::-1])).save(buf, "JPEG", quality=95, subsampling=2,
                                                                                              optimize=False)
                sizes["pil"] = len(buf.getvalue())
        for _ in range(10):
            plain()
            with_jpeg()
            core.set_preview_overlay(7)
            with_overlays()
            core.set_preview_overlay(0)
            proc = download()
        ts = {"track_frame_images": [], "track_frame_images_jpeg": [], "... with overlays (7)": [], "processed to the host": [],
              "PIL encode, one core": []}
        for _ in range(a.calls):
            for name, fn, flags in (("track_frame_images", plain, 0), ("track_frame_images_jpeg", with_jpeg, 0),
                                    ("... with overlays (7)", with_overlays, 7), ("processed to the host", download, 0)):
                core.set_preview_overlay(flags)
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
            core.set_preview_overlay(0)
            if Image is not None:
                t0 = time.perf_counter()
                pil_encode(proc)
                ts["PIL encode, one core"].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in ts.items() if v}
        print(f"--- {C} cameras x 320 x 320, {F} frame set(s) per call, {a.calls} calls each, host wall clock")
        for k, v in ts.items():
            if v:
                print(f"{k:26s} {med[k]:9.3f} ms per call (5th .. 95th percentile {np.percentile(v, 5):.3f} .. {np.percentile(v, 95):.3f})")
            else:
                print(f"{k:26s} skipped (PIL is not installed)")
        print(f"added by the JPEG          {med['track_frame_images_jpeg'] - med['track_frame_images']:9.3f} ms per call")
        print(f"added by the overlays      {med['... with overlays (7)'] - med['track_frame_images_jpeg']:9.3f} ms per call "
              f"(JPEG {int(np.mean(sizes['overlay']))} bytes per frame set with them)")
        print(f"today's route adds         {med['processed to the host'] + med.get('PIL encode, one core', 0.0):9.3f} ms per call "
              "(second blob pass + download" + (" + PIL)" if Image is not None else "; encode not measured)"))
        print(f"bytes over PCIe per frame set: JPEG {int(np.mean(sizes['jpeg']))}, processed {C * 320 * 320 * 3}")
    core.close()


if __name__ == "__main__":
    main()
