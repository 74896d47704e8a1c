"""Timing probe (GPU box): rigid-body learning over a resident capture against what a caller has to do without it.

   python scripts/time_body_learn.py [--frames F] [--k-max K] [--iters I] [--reps N]

Capture: `frames` frames (default 100 000) x K_max 48 slots, a planted 5-marker body under a random rigid motion per frame
(0.5 mm noise, 10 % dropout per marker) plus 8 clutter points with other ids, slots shuffled, resident on the device as the frame
path and the marker tracker leave it.
(1) mocap_learn_rigid_body_dev between two device events on the context's stream: 3 warm-up passes, then `reps`; printed:
    median, min .. max.  The call is a chain of 4 + 2 iters launches; the same call with iters = 1 and 16 gives the cost of one
    round (two launches) and of the fixed part (gather, pair statistics: four launches), and a 256-frame capture the floor the
    launches alone set.
(2) What a caller does today: copy xyz / n_pts / id to the host, then the contract in NumPy (tests/body_learn_reference.py):
    host wall clock of the copy and of the statement, one pass.
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

Q5 = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.15, 0.0], [0.05, 0.05, 0.18], [0.17, 0.16, 0.07]])


def make_capture(F, K, n_clutter=8, noise=0.0005, dropout=0.1, seed=1):
    """Vectorised: -> xyz [F][K][3] (NaN beyond n_pts), n_pts [F], id [F][K] (markers 10 .. 14, clutter 1000 + slot, -1 beyond)."""
    rng = np.random.default_rng(seed)
    N = Q5.shape[0]
    Rm, up = np.linalg.qr(rng.standard_normal((F, 3, 3)))
    Rm = Rm * np.sign(np.einsum("fii->fi", up))[:, None, :]
    Rm[:, :, 0] *= np.sign(np.linalg.det(Rm))[:, None]
    t = rng.uniform(-1, 1, (F, 3))
    pts = np.concatenate([np.einsum("fij,mj->fmi", Rm, Q5) + t[:, None, :] + rng.normal(0, noise, (F, N, 3)),
                          rng.uniform(-1, 1, (F, n_clutter, 3))], axis=1)
    ids = np.concatenate([np.broadcast_to(10 + np.arange(N), (F, N)), np.broadcast_to(1000 + np.arange(n_clutter), (F, n_clutter))], axis=1)
    shown = np.concatenate([rng.random((F, N)) >= dropout, np.ones((F, n_clutter), dtype=bool)], axis=1)
    shown[0] = True
    order = np.argsort(np.where(shown, rng.random(shown.shape), 2.0), axis=1)      # shown points first, in random order
    n_pts = shown.sum(axis=1).astype(np.int32)
    xyz = np.full((F, K, 3), np.nan)
    idk = np.full((F, K), -1, dtype=np.int32)
    M = N + n_clutter
    xyz[:, :M] = np.take_along_axis(pts, order[:, :, None], axis=1)
    idk[:, :M] = np.take_along_axis(ids, order, axis=1)
    beyond = np.arange(K)[None, :] >= n_pts[:, None]
    xyz[beyond], idk[beyond] = np.nan, -1
    return xyz, n_pts, idk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--k-max", type=int, default=48)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import body_learn_reference as bl
    from mocap_core import capi
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    F, K = a.frames, a.k_max
    sel = [10, 11, 12, 13, 14]
    xyz, n_pts, ids = make_capture(F, K)
    d_xyz, d_n, d_id = (torch.from_numpy(x).to(dev) for x in (xyz, n_pts, ids))
    d_res = torch.zeros(capi.LB_RESULT, dtype=torch.float64, device=dev)
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)

    def timed(frames, iters):
        ms = []
        for i in range(3 + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            core.learn_rigid_body_dev(frames, K, d_xyz.data_ptr(), d_n.data_ptr(), d_id.data_ptr(), 0, sel, -1, iters, float("inf"),
                                      d_res.data_ptr())
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms)

    med, lo, hi = timed(F, a.iters)
    print(f"mocap_learn_rigid_body_dev   {med * 1e3:.1f} us per {F} frames x K_max {K}, iters {a.iters}, {4 + 2 * a.iters} launches "
          f"(min {lo * 1e3:.1f} .. max {hi * 1e3:.1f}; {a.reps} passes, device events)")
    got = core.learned_body(d_res.cpu().numpy(), 5)
    one, many = timed(F, 1)[0], timed(F, 16)[0]
    per_round = (many - one) / 15
    print(f"  per launch pair: one round (pose kernel + final) {per_round * 1e3:.1f} us; gather + pair statistics (four launches) "
          f"{(one - per_round) * 1e3:.1f} us")
    f_med = timed(256, a.iters)[0]
    print(f"  the same call over 256 frames (one workgroup per launch: the launches alone) {f_med * 1e3:.1f} us")
    print(f"  result: frames used {got['frames_used']} of {got['frames_valid']}, rms {got['rms']:.3e}, status {got['status']}, "
          f"template error {np.linalg.norm(bl.align(got['markers'], Q5) - Q5, axis=1).max():.2e} m")

    # what a caller does today
    t0 = time.perf_counter()
    h_xyz, h_n, h_id = d_xyz.cpu().numpy(), d_n.cpu().numpy(), d_id.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = bl.learn(h_xyz, h_n, h_id, sel, iters=a.iters)
    t_np = time.perf_counter() - t0
    print(f"today: D2H of xyz / n_pts / id ({(h_xyz.nbytes + h_n.nbytes + h_id.nbytes) / 1e6:.1f} MB, pageable) {t_copy * 1e3:.2f} ms, "
          f"the NumPy statement {t_np * 1e3:.1f} ms (host wall clock, one pass); frames used {ref['frames_used']}, "
          f"largest marker difference to the device {np.abs(ref['markers'] - got['markers']).max():.2e}")
    core.close()


if __name__ == "__main__":
    main()
