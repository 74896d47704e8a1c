"""Timing probe (GPU box): the calibration tail over a resident capture against what a caller had to do before it existed.

   python scripts/time_calib_tail.py [--frames F] [--k-max K] [--reps N]

Capture: `frames` frames (default 100 000) x K_max 48 slots (the 8 x 16 workload's outputs), 0-4 valid points per frame on a
tilted plane, resident on the device as the frame path leaves it.
(1) mocap_determine_scale_dev and mocap_floor_factor_dev, each between two device events on the context's stream: 3 warm-up
    passes, then `reps`; printed: median, min .. max, and the achieved GB/s over the bytes the kernels have to read (24 B per
    valid point + n_pts + status) next to the 8 TB/s of HBM.
(2) What a caller does today: copy xyz / n_out / status to the host, then the reference's arithmetic in NumPy (the pair loop of
    index.py:297-305 vectorised, scipy.linalg.lstsq over every point): host wall clock of the copy and of each piece.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--k-max", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from scipy import linalg
    from mocap_core import capi
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    F, K = a.frames, a.k_max
    rng = np.random.default_rng(1)
    n_pts = rng.integers(0, 5, F).astype(np.int32)
    uv = rng.uniform(-1, 1, (F, K, 2))
    xyz = np.concatenate([uv, (0.17 * uv[..., 0] - 0.1277 * uv[..., 1])[..., None]], axis=-1) + (2.0, -1.5, 0.7) + rng.normal(0, 0.002, (F, K, 3))
    xyz[np.arange(K)[None, :] >= n_pts[:, None]] = np.nan
    d_xyz, d_n = torch.from_numpy(xyz).to(dev), torch.from_numpy(n_pts).to(dev)
    d_st = torch.zeros(F, dtype=torch.int32, device=dev)
    d_res = torch.zeros(4, dtype=torch.float64, device=dev)
    d_fac = torch.zeros(17, dtype=torch.float64, device=dev)
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    calls = {
        "mocap_determine_scale_dev": (lambda: core.determine_scale_dev(F, K, d_xyz.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), 0.15, 0,
                                                                       d_res.data_ptr()),
                                      int((n_pts == 2).sum()) * 48 + 8 * F),
        "mocap_floor_factor_dev": (lambda: core.floor_factor_dev(F, K, d_xyz.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), d_fac.data_ptr()),
                                   int(n_pts.sum()) * 24 + 8 * F),
    }
    for name, (fn, nbytes) in calls.items():
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        print(f"{name:28s} {med * 1e3:.1f} us per {F} frames x K_max {K} (min {min(ms) * 1e3:.1f} .. max {max(ms) * 1e3:.1f}; {len(ms)} passes, "
              f"device events); {nbytes / 1e6:.2f} MB to read = {nbytes / med / 1e6:.1f} GB/s of 8000")
    print("result", d_res.cpu().numpy().tolist(), " points", float(d_fac[16].item()))

    # what a caller does today
    t0 = time.perf_counter()
    h_xyz, h_n, h_st = d_xyz.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    ok = (h_st == 0) & (h_n >= 0) & (h_n <= K)
    pair = ok & (h_n == 2)
    scale = 0.15 / np.mean(np.sqrt(np.sum((h_xyz[pair, 0] - h_xyz[pair, 1]) ** 2, axis=1)))
    t_scale = time.perf_counter() - t0
    t0 = time.perf_counter()
    pts = h_xyz[np.arange(K)[None, :] < np.where(ok, h_n, 0)[:, None]]
    fit = linalg.lstsq(np.c_[pts[:, :2], np.ones(len(pts))], pts[:, 2])[0]
    t_floor = time.perf_counter() - t0
    print(f"today: D2H of xyz / n_out / status ({(h_xyz.nbytes + h_n.nbytes + h_st.nbytes) / 1e6:.1f} MB, pageable) {t_copy * 1e3:.2f} ms, "
          f"NumPy pair scale {t_scale * 1e3:.2f} ms, gather + scipy lstsq {t_floor * 1e3:.2f} ms (host wall clock, one pass); "
          f"scale {scale!r}, fit {fit.tolist()}")
    core.close()


if __name__ == "__main__":
    main()
