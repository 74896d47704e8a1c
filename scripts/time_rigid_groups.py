"""Timing probe (GPU box): the rigid groups of a recorded session found on the device, beside the host route it replaces -- the
rows copied to the host and the NumPy statement of the contract run on them.

   python scripts/time_rigid_groups.py [--frames F] [--reps N]

(1) Session: `frames` frames (default 100 000), 16 rows: two bodies of five markers under rigid motions of their own, five loose
    markers, one static, 0.5 mm noise, 5 % dropout; resident on the device as mocap_gather_tracks_dev leaves it.
    mocap_rigid_groups_dev (tol 3 mm, min_common 50) between two device events on the context's stream: 3 warm-up passes, then `reps`;
    printed: median, min .. max, and whether the groups are the planted bodies.
(2) The same at R = 128: 24 bodies of four markers and 32 loose ones.
(3) The propagation's worst case: the chain of tests/rigid_groups_reference.py at R = 256 (three rounds of launches, 255 edges in a line).
(4) The host route: the D2H copy of the rows (wall clock) and the NumPy statement (tests/rigid_groups_reference.py, vectorised), one
    pass, results compared bit for bit.  At R = 128 the statement runs on the first 1/25 of the frames only (on all of them it needs
    gigabytes and minutes); its time scaled by 25 is printed as an estimate and named as one.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import rigid_groups_reference as rg
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

    def run(name, traj, kw, statement=True):
        R, F, _ = traj.shape
        d_traj = torch.from_numpy(traj).to(dev)
        o = {"cnt": torch.zeros((R, R), dtype=torch.int32, device=dev), "n_groups": torch.zeros(1, dtype=torch.int32, device=dev)}
        o.update({k: torch.zeros((R, R), dtype=torch.float64, device=dev) for k in ("dist", "spread")})
        o.update({k: torch.zeros(R, dtype=torch.float64, device=dev) for k in ("travel", "gspread")})
        o.update({k: torch.zeros(R, dtype=torch.int32, device=dev) for k in ("group_of", "gsize", "ghead", "gconf")})
        r = timed(lambda: core.rigid_groups_dev(F, R, d_traj.data_ptr(), kw["min_common"], kw["tol"], kw["max_dist"], kw["min_travel"],
                                                *[o[k].data_ptr() for k in core.RIGID_OUT]))
        print(f"mocap_rigid_groups_dev {name:8s} {r[0]:9.3f} ms per {F} frames x {R} rows (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, "
              f"device events)")
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["n_groups"] = int(got["n_groups"][0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        back = d_traj.cpu()
        copy = time.perf_counter() - t0
        assert back.shape == d_traj.shape
        print(f"  the rows to the host (D2H of {traj.nbytes / 1e6:.0f} MB, pageable): {copy * 1e3:.1f} ms (host wall clock, one pass)")
        wall = None
        if statement:
            t0 = time.perf_counter()
            ref = rg.rigid_groups(traj, **kw)
            wall = time.perf_counter() - t0
            print(f"  the NumPy statement on the same data: {wall * 1e3:.1f} ms (host wall clock, one pass); equal to the device's, integers "
                  f"exactly and dist, spread, travel, gspread bit for bit: {rg.same(got, ref)}")
        return got, wall

    kw = dict(min_common=50, tol=0.003, max_dist=float("inf"), min_travel=0.0)
    traj, owner = rg.make_scene(1, a.frames, bodies=(5, 5), n_loose=5, n_static=1, dropout=0.05)
    got, _ = run("session", traj, kw)
    print(f"  the groups are the two planted bodies: "
          f"{sorted(rg.rows_of_groups(got)) == sorted(np.flatnonzero(owner == b).tolist() for b in (0, 1))}, "
          f"conflicts {got['gconf'][:got['n_groups']].tolist()}")
    traj, owner = rg.make_scene(2, a.frames, bodies=(4,) * 24, n_loose=32, n_static=0, dropout=0.05)
    got, _ = run("R = 128", traj, kw, statement=False)
    print(f"  groups {got['n_groups']}, of which planted bodies: "
          f"{sum(1 for g in rg.rows_of_groups(got) if len(set(owner[g])) == 1 and owner[g[0]] >= 0 and len(g) == 4)} of 24")
    part = np.ascontiguousarray(traj[:, :max(a.frames // 25, 1)])
    _, wall = run("R = 128 / 25", part, kw)
    print(f"  (scaled by 25 to all {a.frames} frames the NumPy statement at R = 128 is an ESTIMATE of {wall * 25:.1f} s, not a measurement)")
    run("chain", rg.chain(256), rg.CHAIN)
    core.close()


if __name__ == "__main__":
    main()
