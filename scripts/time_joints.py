"""Timing probe (GPU box): the joints of a recorded session found on the device, and the series of its joints, beside two yardsticks.

   python scripts/time_joints.py [--frames F] [--reps N] [--bodies 8 64]

Per body count B (default 8 and 64) a session of `frames` frames (default 100 000) of chained bodies (tests/joints_reference.py,
session: ball joints and hinges alternate, every fourth body flies free, 8 % of the flags not POSED), resident on the device as
mocap_pose_rows_dev leaves it.  Between two device events on the context's stream, 3 warm-up passes and then `reps` (default 20):
    mocap_find_joints_dev      min_common 30, tol_rank 1e-4, max_sep 1 cm
    mocap_joint_series_dev     over the tree edges found
    mocap_rigid_groups_dev     at R = B rows over the same F (the bodies' origins as rows): the pair pass this one was modelled on
printed as median, min .. max, with the bytes each pass must move at least once -- the pose tables, 100 B per (body, frame), once per
pair pass; the series' inputs and outputs once -- and the time those bytes take at 8.0 TB/s (the data sheet) and at 6.3 TB/s (the copy
rate DESIGN.md 3.7q reports).  Nothing is asserted."""
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
    a = ap.parse_args()
    import torch
    import joints_reference as jr
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
        print(f"{name:26s} {r[0]:9.3f} ms (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, device events); must move {moved / 1e6:.0f} MB "
              f"({what}): {moved / 8.0e9:.3f} ms at 8.0 TB/s, {moved / 6.3e9:.3f} ms at 6.3 TB/s")

    for B in a.bodies:
        F = a.frames
        flag, Rm, t = jr.session(B, F, B)
        quat = np.zeros((B, F, 4))
        quat[..., 0] = 1.0                                        # (the series' arithmetic does not depend on the values)
        d = {"flag": torch.from_numpy(flag).to(dev), "R": torch.from_numpy(Rm).to(dev), "t": torch.from_numpy(t).to(dev),
             "quat": torch.from_numpy(quat).to(dev)}
        o = {k: torch.zeros((B, B), dtype=torch.int32, device=dev) for k in ("cnt", "kind", "accepted")}
        o.update({k: torch.zeros((B, B, 3), dtype=torch.float64, device=dev) for k in ("lam", "centre", "axis")})
        o.update(sep=torch.zeros((B, B), dtype=torch.float64, device=dev), parent=torch.zeros(B, dtype=torch.int32, device=dev),
                 n_joints=torch.zeros(1, dtype=torch.int32, device=dev))
        print(f"--- {B} bodies x {F} frames")
        r = timed(lambda: core.find_joints_dev(F, B, d["flag"].data_ptr(), d["R"].data_ptr(), d["t"].data_ptr(), 30, 1e-4, 0.01,
                                               *[o[k].data_ptr() for k in core.JOINTS_OUT]))
        line("mocap_find_joints_dev", r, 2 * B * F * 100, "the pose tables once per pair pass, two passes")
        got = {k: v.cpu().numpy() for k, v in o.items()}
        kinds = {name: int((got["kind"][np.triu_indices(B, 1)] == v).sum()) for name, v in
                 (("UNSEEN", jr.UNSEEN), ("SINGULAR", jr.SINGULAR), ("FIXED", jr.FIXED), ("HINGE", jr.HINGE), ("BALL", jr.BALL))}
        print(f"  pairs {B * (B - 1) // 2}: {kinds}; accepted {int(got['accepted'].sum()) // 2}, tree edges {int(got['n_joints'][0])}")
        joints = [{"a": min(c, int(p)), "b": max(c, int(p)), "kind": int(got["kind"][c, p]), "c_a": got["centre"][min(c, p), max(c, p)],
                   "c_b": got["centre"][max(c, p), min(c, p)], "axis_b": got["axis"][max(c, p), min(c, p)]}
                  for c, p in enumerate(got["parent"]) if p >= 0]
        if joints:
            J = len(joints)
            s = {"present": torch.zeros((J, F), dtype=torch.int32, device=dev), "centre": torch.zeros((J, F, 3), dtype=torch.float64, device=dev),
                 "gap": torch.zeros((J, F), dtype=torch.float64, device=dev), "quat_rel": torch.zeros((J, F, 4), dtype=torch.float64, device=dev),
                 "twist": torch.zeros((J, F, 2), dtype=torch.float64, device=dev)}
            r = timed(lambda: core.joint_series_dev(F, B, d["flag"].data_ptr(), d["quat"].data_ptr(), d["R"].data_ptr(), d["t"].data_ptr(),
                                                    joints, *[s[k].data_ptr() for k in core.SERIES_OUT]))
            line(f"mocap_joint_series_dev J={J}", r, J * F * (2 * 132 + 84), "two bodies' 132 B in and 84 B out per (joint, frame)")
        rows = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
        g = {"cnt": torch.zeros((B, B), dtype=torch.int32, device=dev), "n_groups": torch.zeros(1, dtype=torch.int32, device=dev)}
        g.update({k: torch.zeros((B, B), dtype=torch.float64, device=dev) for k in ("dist", "spread")})
        g.update({k: torch.zeros(B, dtype=torch.float64, device=dev) for k in ("travel", "gspread")})
        g.update({k: torch.zeros(B, dtype=torch.int32, device=dev) for k in ("group_of", "gsize", "ghead", "gconf")})
        r = timed(lambda: core.rigid_groups_dev(F, B, rows.data_ptr(), 30, 0.003, float("inf"), 0.0, *[g[k].data_ptr() for k in core.RIGID_OUT]))
        line(f"mocap_rigid_groups_dev R={B}", r, 3 * B * F * 24, "the rows once per pass: bounds and two pair passes")
    core.close()


if __name__ == "__main__":
    main()
