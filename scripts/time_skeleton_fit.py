"""Timing probe (GPU box): all joints of a frame closed at once on the device, beside mocap_pose_joints and mocap_pose_rows.

   python scripts/time_skeleton_fit.py [--frames F] [--reps N] [--bodies 8 64] [--hidden 0.08 0.30] [--iters 8] [--sigma 0.0005]

The sessions are scripts/time_joint_poses.py's: per body count B (default 8 and 64) and per share of hidden (body, frame)s (default
8 % and 30 %) `frames` frames (default 100 000) of chained bodies with four markers each (tests/joint_pose_reference.py,
tree_session: ball joints and hinges alternate, every fourth body flies free); a hidden body shows 0, 1 or 2 of its markers; here
with `sigma` metres of marker noise, so that a fit has something to close.  The session is resident on the device; the flags and
poses are mocap_pose_rows_dev's and mocap_pose_joints_dev's own.  Between two device events on the context's stream, 3 warm-up passes
and then `reps` (default 20):
    mocap_pose_rows_dev        the yardstick: every (body, frame) fitted or flagged
    mocap_pose_joints_dev      max_rounds 4, max_rms inf, axis_len 0.1 with the planted joints
    mocap_fit_skeleton_dev     w_joint 1, `iters` passes (default 8) over the jointed poses
printed as median, min .. max, with the bytes each call must move at least once and the time those bytes take at 8.0 TB/s (the data
sheet) and at 6.3 TB/s (the copy rate DESIGN.md 3.7q reports).  For mocap_fit_skeleton that is, per (body, frame): flag, quat and
t_pose in (60 B), the markers in (96 B), quat_s, Rm_s, t_s and rms_s out (136 B), 46 B for the sign walk; per frame 24 B out.  The
workspace traffic of the passes is not in that figure: it is what the call moves on top.  Nothing is asserted."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bodies", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--hidden", type=float, nargs="+", default=[0.08, 0.30])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.0005)
    a = ap.parse_args()
    import torch
    import joint_pose_reference as jp
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

    def line(name, r, moved, what):
        print(f"{name:28s} {r[0]:9.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, device events); must move {moved / 1e6:.0f} MB "
              f"({what}): {moved / 8.0e9:.3f} ms at 8.0 TB/s, {moved / 6.3e9:.3f} ms at 6.3 TB/s", flush=True)

    def f64(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    def i32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)

    for B in a.bodies:
        F, N = a.frames, 4
        clean, bodies, joints, _ = jp.tree_session(B, F, [-1 if b % 4 == 0 else b - 1 for b in range(B)], n_markers=[N] * B, shares={})
        R = clean.shape[0]
        for share in a.hidden:
            rng = np.random.default_rng(B)
            traj = clean + a.sigma * rng.standard_normal(clean.shape)
            seen = np.where(rng.uniform(size=(B, F)) < share, rng.choice(3, size=(B, F), p=[0.25, 0.25, 0.5]), N)   # markers shown
            rank = np.argsort(np.argsort(rng.uniform(size=(B, N, F)), axis=1), axis=1)
            traj[:B * N][(rank >= seen[:, None, :]).reshape(B * N, F)] = np.nan
            d_traj = torch.from_numpy(traj).to(dev)
            p = {"quat": f64(B, F, 4), "R": f64(B, F, 9), "t_pose": f64(B, F, 3), "rms": f64(B, F)}
            p.update({k: i32(B, F) for k in ("n_used", "present", "flag")})
            o = {k: i32(B, F) for k in ("flag", "hops", "via")}
            o.update(quat=f64(B, F, 4), R=f64(B, F, 9), t_pose=f64(B, F, 3), rms_j=f64(B, F))
            s = dict(quat=f64(B, F, 4), R=f64(B, F, 9), t_pose=f64(B, F, 3), rms_s=f64(B, F), cost0=f64(F), cost=f64(F), steps=i32(F), n_act=i32(F))
            print(f"--- {B} bodies x {F} frames, {100 * share:.0f} % of the (body, frame)s hidden, {len(joints)} joints, "
                  f"{1e3 * a.sigma:g} mm of noise", flush=True)
            r = timed(lambda: core.pose_rows_dev(F, R, d_traj.data_ptr(), bodies, float("inf"), *[p[k].data_ptr() for k in core.POSE_OUT]))
            line("mocap_pose_rows_dev", r, B * F * (N * 24 + 148), "the markers in, 148 B out per (body, frame)")
            r = timed(lambda: core.pose_joints_dev(F, R, d_traj.data_ptr(), bodies, p["flag"].data_ptr(), p["quat"].data_ptr(), p["R"].data_ptr(),
                                                   p["t_pose"].data_ptr(), joints, 0.1, float("inf"), a.rounds,
                                                   *[o[k].data_ptr() for k in core.JOINT_POSE_OUT]))
            hidden = int((p["flag"] != capi.BP_POSED).sum())
            line(f"mocap_pose_joints_dev r={a.rounds}", r, B * F * (132 + 148 + 8 * a.rounds + 46) + hidden * (N * 24 + 96 + 148),
                 "see scripts/time_joint_poses.py")
            r = timed(lambda: core.fit_skeleton_dev(F, R, d_traj.data_ptr(), bodies, o["flag"].data_ptr(), o["quat"].data_ptr(),
                                                    o["t_pose"].data_ptr(), joints, 0.1, 1.0, a.iters,
                                                    *[s[k].data_ptr() for k in core.SKELETON_FIT_OUT]))
            line(f"mocap_fit_skeleton_dev i={a.iters}", r, B * F * (60 + N * 24 + 136 + 46) + F * 24, "see the head of this file")
            steps, cost0, cost = s["steps"].cpu().numpy(), s["cost0"].cpu().numpy(), s["cost"].cpu().numpy()
            print(f"  frames with steps > 0: {100 * (steps > 0).mean():.1f} %, mean steps {steps.mean():.2f}; cost {cost0.sum():.4g} -> {cost.sum():.4g} m^2; "
                  f"active joints per frame {s['n_act'].double().mean().item():.2f}", flush=True)
    core.close()


if __name__ == "__main__":
    main()
