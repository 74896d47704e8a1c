"""Timing probe (GPU box): predicted precision -- the capture-volume map and the point form.

   python scripts/time_precision.py [--reps N] [--grid 256 256 128] [--cameras 8 64] [--points 1048576]

Per camera count C (default 8 and 64; the project's calibrated synthetic rigs) between two device events on the context's stream,
3 warm-up passes and then `reps` (default 20):
    mocap_coverage_map_dev     the grid (default 256 x 256 x 128) over a 6 x 6 x 3 m box around the rig's centre, by visibility, with
                               and without the `seen` output
    mocap_point_precision_dev  `points` points (default 2^20) in the named form, every camera named
printed as median, min .. max, voxels or points per second, the bytes the call must move once (map: 5 B per voxel out, 13 B with
`seen`; points: 24 B xyz + 8 B seen in, 104 B out) with the time those bytes take at 8.0 TB/s (the data sheet) and at 6.3 TB/s (the
copy rate DESIGN.md 3.7q reports), and the FP64 share of the vector peak bench.py --full divides by (78.6 TFLOP/s).  The FP64 work
is COUNTED FROM THE CONTRACT'S TEXT, one flop per operation it writes, a division and a square root as one each (the hardware
expands them): per camera tested 20 (a, b, w, pu, pv), per view 42 more (Ju, Jv, H), per decomposed point 3 rotations of 47 per
sweep at the statement's mean sweep count of the same inputs, plus 75 for sig, axis and cov.  No counter pass stands behind it.
Nothing is asserted."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VALU_PEAK_TF = 78.6      # bench.py's figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grid", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--cameras", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--points", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    import precision_reference as pr
    from mocap_core import capi, synth
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def timed(call):
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms)

    def line(name, r, n, unit, moved, flop):
        print(f"{name:34s} {r[0]:9.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, device events); {n / r[0] / 1e6:.2f} G{unit}/s; "
              f"must move {moved / 1e6:.0f} MB: {moved / 8.0e9:.3f} ms at 8.0 TB/s, {moved / 6.3e9:.3f} ms at 6.3 TB/s; "
              f"counted FP64 {flop / 1e9:.2f} Gflop = {100 * flop / (r[0] * 1e-3) / 1e12 / FP64_VALU_PEAK_TF:.1f} % of {FP64_VALU_PEAK_TF} TFLOP/s",
              flush=True)

    nx, ny, nz = a.grid
    V = nx * ny * nz
    for C in a.cameras:
        rig = synth.calibrated_ring_rig(C, seed=3)
        core.set_cameras(rig["K"], rig["R"], rig["t"])
        P = pr.camera_table(rig["K"], rig["R"], rig["t"])
        size = rig["image_size"]
        step = np.array([6.0, 6.0, 3.0]) / np.maximum(np.array(a.grid) - 1, 1)
        R0 = rig["R0"]
        e = [R0[:, d] * step[d] for d in range(3)]
        origin = rig["centre"] - sum(e[d] * (a.grid[d] - 1) / 2.0 for d in range(3))
        n_views = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
        sig_max = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
        seen = torch.empty((nz, ny, nx), dtype=torch.int64, device=dev)
        summary = torch.empty(capi.PM_SUMMARY, dtype=torch.int64, device=dev)
        print(f"--- {C} cameras, picture {size[0]} x {size[1]}, map {nx} x {ny} x {nz} = {V} voxels", flush=True)

        def run_map(with_seen):
            core.coverage_map_dev(a.grid, origin, e[0], e[1], e[2], size, 0.1, 20.0, 0.5, None, 3, 0.005, n_views.data_ptr(),
                                  sig_max.data_ptr(), seen.data_ptr() if with_seen else 0, summary.data_ptr())
        # the statement's sweep count on a coarse sample of the same grid (the map's own outputs give the views)
        sample = pr.coverage_map(P, (16, 16, 8), origin, e[0] * (nx - 1) / 15.0, e[1] * (ny - 1) / 15.0, e[2] * (nz - 1) / 7.0, size, 0.1, 20.0, 0.5)
        xs = pr.grid_points((16, 16, 8), origin, e[0] * (nx - 1) / 15.0, e[1] * (ny - 1) / 15.0, e[2] * (nz - 1) / 7.0)
        sweeps = pr.evaluate(P, xs, 0.5, vis=(size[0], size[1], 0.1, 20.0))["sweeps"]
        mean_sweeps = float(sweeps[sample["info"].reshape(-1) == pr.OK].mean()) if (sample["info"] == pr.OK).any() else 0.0
        for with_seen in (False, True):
            r = timed(lambda: run_map(with_seen))
            s = summary.cpu().numpy()
            views = float((np.arange(65) * s[:65]).sum())
            decomposed = float(s[2:65].sum())
            flop = V * C * 20.0 + views * 42.0 + decomposed * (3 * 47 * mean_sweeps + 75)
            line("mocap_coverage_map_dev" + (" +seen" if with_seen else ""), r, V, "voxel", V * (13 if with_seen else 5), flop)
        print(f"  views per voxel {views / V:.2f}; voxels with a covariance {100 * decomposed / V:.1f} %; GOOD {100 * s[65] / V:.1f} %; "
              f"mean sweeps (statement, 2048-voxel sample) {mean_sweeps:.2f}", flush=True)

        N = a.points
        rng = np.random.default_rng(C)
        x = rig["centre"][None] + rng.uniform(-1.0, 1.0, (N, 3))
        d_x = torch.from_numpy(x).to(dev)
        d_seen = torch.full((N,), -1 if C == 64 else (1 << C) - 1, dtype=torch.int64, device=dev)
        out = {"cov": torch.empty((N, 6), dtype=torch.float64, device=dev), "sig": torch.empty((N, 3), dtype=torch.float64, device=dev),
               "axis": torch.empty((N, 3), dtype=torch.float64, device=dev), "n_views": torch.empty(N, dtype=torch.int32, device=dev),
               "info": torch.empty(N, dtype=torch.int32, device=dev)}
        r = timed(lambda: core.point_precision_dev(N, d_x.data_ptr(), d_seen.data_ptr(), None, 0.0, float("inf"), 0.5, None,
                                                   *[out[k].data_ptr() for k in core.PRECISION_OUT]))
        ok = int((out["info"] == capi.PM_OK).sum())
        sw = pr.evaluate(P, x[:2048], 0.5, named=np.ones((2048, C), dtype=bool))
        mean_sweeps = float(sw["sweeps"][sw["info"] == pr.OK].mean())
        flop = N * C * 62.0 + ok * (3 * 47 * mean_sweeps + 75)
        line("mocap_point_precision_dev named", r, N, "point", N * (24 + 8 + 104), flop)
        print(f"  points with a covariance {100 * ok / N:.1f} %; mean sweeps (statement, 2048 points) {mean_sweeps:.2f}", flush=True)
    core.close()


if __name__ == "__main__":
    main()
