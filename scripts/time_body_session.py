"""Timing probe (GPU box): a session's bodies as 6-DoF series on the device ("body trajectories", include/mocap_core.h).

   python scripts/time_body_session.py [--frames F] [--reps N] [--check K]

For each of two shapes -- 8 bodies of 4 markers and 64 bodies of 8 markers, `frames` frames (default 100 000) at 120 Hz, 0.5 mm of
noise, 5 % dropout, the rows resident on the device as mocap_gather_tracks_dev leaves them -- each stage between two device events
on the context's stream, 3 warm-up passes, then `reps`; printed: median, min .. max.
  poses      mocap_pose_rows_dev (table + pose kernel + the four launches of the sign rule); also ns per (body, frame)
  origin     mocap_smooth_tracks_dev over t_pose (the existing kernel, for comparison)
  rotation   mocap_smooth_rotations_dev; bytes moved = what the stage must read and write once (t, quat in; quat_s, omega, res,
             n_used, flag out), against 8.0 TB/s (the HBM peak) and 6.3 TB/s (what a copy achieves)
  fill       mocap_fill_rows_dev with the smoothers' arrays; bytes likewise (traj in, filled and src out, and for the samples that
             are missing the pose of their body)
These are call times over what the algorithm must move, not kernel times: the share of the bound they print is an end-to-end
figure.  The first `check` frames of every output are compared with the NumPy statement (tests/body_session_reference.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK, COPY = 8.0e12, 6.3e12   # bytes / s: HBM3E as specified, and what a float4 copy achieves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check", type=int, default=2000)
    a = ap.parse_args()
    import torch
    import body_session_reference as bs
    import track_smooth_reference as ts
    from mocap_core import capi
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

    def show(name, r, extra=""):
        print(f"  {name:9s} {r[0]:9.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, device events){extra}")

    def roof(r, nbytes):
        return (f"; {nbytes / 1e6:.0f} MB to move: {nbytes / (r[0] * 1e-3) / 1e12:.2f} TB/s, {nbytes / PEAK / (r[0] * 1e-3):.0%} of the "
                f"8.0 TB/s bound, {nbytes / COPY / (r[0] * 1e-3):.0%} of a copy's 6.3 TB/s")

    par = (2, 8, float("inf"), 5, 4)
    for B, N in ((8, 4), (64, 8)):
        F = a.frames
        t, traj, bodies, _ = bs.make_session(B, F, (N,) * B, n_loose=0, dropout=0.05)
        R = traj.shape[0]
        print(f"{B} bodies x {N} markers, {F} frames, {R} rows ({traj.nbytes / 1e6:.0f} MB)")
        d_t, d_traj = torch.from_numpy(t).to(dev), torch.from_numpy(traj).to(dev)

        def f64(*s):
            return torch.zeros(s, dtype=torch.float64, device=dev)

        def i32(*s):
            return torch.zeros(s, dtype=torch.int32, device=dev)

        p = {"n_used": i32(B, F), "present": i32(B, F), "quat": f64(B, F, 4), "R": f64(B, F, 3, 3), "t_pose": f64(B, F, 3),
             "rms": f64(B, F), "flag": i32(B, F)}
        s = {"pos": f64(B, F, 3), "vel": f64(B, F, 3), "acc": f64(B, F, 3), "res": f64(B, F), "n_used": i32(B, F), "flag": i32(B, F)}
        r = {"quat_s": f64(B, F, 4), "omega": f64(B, F, 3), "res": f64(B, F), "n_used": i32(B, F), "flag": i32(B, F)}
        o = {"filled": f64(R, F, 3), "src": i32(R, F)}
        x = timed(lambda: core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, 0.005, *[p[k].data_ptr() for k in core.POSE_OUT]))
        show("poses", x, f"; {x[0] * 1e6 / (B * F):.2f} ns per (body, frame)")
        x = timed(lambda: core.smooth_tracks_dev(F, B, d_t.data_ptr(), p["t_pose"].data_ptr(), *par,
                                                 *[s[k].data_ptr() for k in ("pos", "vel", "acc", "res", "n_used", "flag")]))
        show("origin", x, roof(x, 8 * F + B * F * (24 + 72 + 8 + 8)))
        x = timed(lambda: core.smooth_rotations_dev(F, B, d_t.data_ptr(), p["quat"].data_ptr(), *par, *[r[k].data_ptr() for k in core.ROT_OUT]))
        show("rotation", x, roof(x, 8 * F + B * F * (32 + 32 + 24 + 8 + 8)))
        x = timed(lambda: core.fill_rows_dev(F, R, d_traj.data_ptr(), bodies, p["flag"].data_ptr(), p["R"].data_ptr(), p["t_pose"].data_ptr(),
                                             r["flag"].data_ptr(), r["quat_s"].data_ptr(), s["pos"].data_ptr(), o["filled"].data_ptr(),
                                             o["src"].data_ptr()))
        missing = int(np.isnan(traj[:, :, 0]).sum())
        show("fill", x, roof(x, R * F * (24 + 24 + 4) + missing * (4 + 72 + 24)))
        # the first frames against the statement (the sign rule is a prefix: a cut at the front changes nothing before it)
        K = min(a.check, F)
        got = {k: v[:, :K].cpu().numpy() for k, v in p.items()}
        ref = bs.pose_rows(traj[:, :K], bodies, 0.005)
        same = all(np.array_equal(got[k], ref[k]) if ref[k].dtype == np.int32 else bs.same_bits(got[k], ref[k]) for k in core.POSE_OUT)
        fill = {k: v[:, :K].cpu().numpy() for k, v in o.items()}
        print(f"  the first {K} frames of the poses equal the NumPy statement, integers exactly and doubles bit for bit: {same}; "
              f"POSED {np.mean(got['flag'] == bs.POSED):.1%}, filled rigidly {np.mean(fill['src'] == bs.SRC_RIGID):.1%} of the samples, "
              f"from the smoothed pose {np.mean(fill['src'] == bs.SRC_RIGID_FILLED):.2%}, left empty {np.mean(fill['src'] == bs.SRC_NONE):.2%}")
        del d_traj, p, s, r, o
        torch.cuda.empty_cache()
    core.close()
    assert ts.SMOOTHED == capi.TS_SMOOTHED


if __name__ == "__main__":
    main()
