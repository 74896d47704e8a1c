"""Timing probe (GPU box): the fragments of a recorded session's markers stitched into chains on the device, beside the NumPy
statement of the contract on the same data.

   python scripts/time_track_stitch.py [--frames F] [--markers M] [--cuts C] [--reps N]

(1) Session: `frames` frames (default 100 000) at 120 Hz with 20 % jitter, `markers` (16) markers on slow sinusoids 0.5 m apart,
    0.5 mm noise, dropouts of 1 .. 4 frames, each marker hidden `cuts` (4) times for 10 .. 40 frames so that it is markers x (cuts + 1)
    rows, shuffled; resident on the device as mocap_gather_tracks_dev leaves it.  mocap_stitch_tracks_dev (fit_frames 8, max_dt
    0.5 s, gate 3 cm + 0.3 m/s) between two device events on the context's stream: 3 warm-up passes, then `reps`; printed: median,
    min .. max, and whether every chain is one marker's fragments.
(2) The association's worst case: the ladder of tests/track_stitch_reference.py at R = 1024, one commit per round, 1 023 rounds.
(3) The NumPy statement (tests/track_stitch_reference.py, vectorised) on both, host wall clock, one pass; results compared.
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


def make_rows(F, M, cuts, noise=0.0005, seed=1):
    """-> t [F], rows [M * (cuts + 1)][F][3], owner [rows]"""
    rng = np.random.default_rng(seed)
    t = np.cumsum((1.0 + 0.2 * rng.uniform(-1.0, 1.0, F)) / 120.0)
    side = int(np.ceil(np.sqrt(M)))
    home = np.array([[0.5 * (m % side), 0.5 * (m // side), 1.0] for m in range(M)])
    w, ph = rng.uniform(0.3, 2.0, (M, 3)), rng.uniform(0.0, 2.0 * np.pi, (M, 3))
    pts = home[:, None] + 0.1 * np.sin(w[:, None] * t[None, :, None] + ph[:, None]) + rng.normal(0.0, noise, (M, F, 3))
    starts = (rng.random((M, F)) < 0.02)
    starts[:, :20] = False
    for k in range(4):                                   # dropouts of 1 .. 4 frames
        gone = starts & (rng.integers(1, 5, (M, F)) > k)
        pts[:, k:][gone[:, :F - k]] = np.nan
    rows, owner = [], []
    for m in range(M):
        edges = np.sort(rng.choice(np.arange(F // 20, F - F // 20, max(F // (4 * cuts + 4), 50)), cuts, replace=False))
        lo = 0
        for e in list(edges) + [F]:
            row = np.full((F, 3), np.nan)
            row[lo:e] = pts[m, lo:e]
            rows.append(row)
            owner.append(m)
            lo = e + int(rng.integers(10, 41))
    order = rng.permutation(len(rows))
    return t, np.stack(rows)[order], np.array(owner)[order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--markers", type=int, default=16)
    ap.add_argument("--cuts", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import track_stitch_reference as st
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

    def run(name, t, traj, kw):
        R, F, _ = traj.shape
        d_t, d_traj = torch.from_numpy(t).to(dev), torch.from_numpy(traj).to(dev)
        o = {k: torch.zeros(R, dtype=torch.int32, device=dev) for k in ("next", "prev", "chain", "row_of")}
        o.update(ext=torch.zeros((R, 3), dtype=torch.int32, device=dev), cost=torch.zeros(R, dtype=torch.float64, device=dev),
                 n_chains=torch.zeros(1, dtype=torch.int32, device=dev))
        r = timed(lambda: core.stitch_tracks_dev(F, R, d_t.data_ptr(), d_traj.data_ptr(), kw["fit_frames"], kw["max_dt"], kw["gate"],
                                                 kw["gate_rate"], *[o[k].data_ptr() for k in core.STITCH_OUT]))
        print(f"mocap_stitch_tracks_dev {name:10s} {r[0]:9.3f} ms per {F} frames x {R} rows (min {r[1]:.3f} .. max {r[2]:.3f}; {a.reps} passes, "
              f"device events)")
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["n_chains"] = int(got["n_chains"][0])
        t0 = time.perf_counter()
        ref = st.stitch(t, traj, kw["fit_frames"], kw["max_dt"], kw["gate"], kw["gate_rate"])
        wall = time.perf_counter() - t0
        print(f"  the NumPy statement on the same data: {wall * 1e3:.1f} ms (host wall clock, one pass); equal to the device's, integers "
              f"exactly and cost bit for bit: {st.same(got, ref)}; links {int((ref['next'] >= 0).sum())}, chains {ref['n_chains']}, "
              f"admissible pairs {int(np.isfinite(ref['table']).sum())}, rounds that commit {st.associate_rounds(ref['table'])[3]}")
        return ref

    t, rows, owner = make_rows(a.frames, a.markers, a.cuts)
    ref = run("session", t, rows, dict(fit_frames=8, max_dt=0.5, gate=0.03, gate_rate=0.3))
    chains = st.chains_of(ref)
    print(f"  every chain one marker's fragments, every marker one chain: "
          f"{len(chains) == a.markers and all(len(set(owner[c])) == 1 and len(c) == a.cuts + 1 for c in chains)}")
    t, traj = st.ladder(1024)
    run("ladder", t, traj, st.LADDER)
    core.close()


if __name__ == "__main__":
    main()
