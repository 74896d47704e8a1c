"""The accuracy table of DESIGN 3.7r (CPU, no GPU needed): what a capture must look like for a lens calibration to be worth anything.

   python scripts/lens_accuracy_table.py [--seeds 3] [--cameras 4]

The plain-double statement of the contract (tests/ba_lens_reference.solve, all eight intrinsics of every camera as unknowns) on planted
rigs with planted lenses: half_extent 0.7 (the default of synth.make_ba_observations: markers in the middle of the pictures) and 1.3
(markers out to the corners), noise 0.3 px (integer centroids) and 0.05 px (the sub-pixel centroid mode), 300 and 3 000 points; per
cell the median over the seeds (capture seeds 6, 7, ...) of the largest rotation error, relative focal error, principal-point error and
k1 error over the cameras.  The start is perturb_rig's poses (20 mrad, 5 cm), the nominal K and zero coefficients."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--cameras", type=int, default=4)
    a = ap.parse_args()
    import ba_lens_reference as bl
    np.seterr(all="ignore")
    print("| half_extent | noise px | N | views | rotation mrad | focal % | centre px | k1 | passes |")
    print("|---|---|---|---|---|---|---|---|---|")
    for he in (0.7, 1.3):
        for noise in (0.3, 0.05):
            for N in (300, 3000):
                rows = []
                for s in range(a.seeds):
                    rig, obs, _, start = bl.planted_case(a.cameras, N, noise_px=noise, seed=6 + s, half_extent=he)
                    R, t, K, d, _, info = bl.solve(obs, start["R"], start["t"], start["K"], start["dist"], flags=bl.ALL)
                    f, c, k1 = bl.lens_errors(K, d, rig)
                    rows.append((int((~np.isnan(obs[..., 0])).sum()), bl.pose_errors(R, t, rig)[0] * 1e3, f * 100, c, k1, info["passes"]))
                m = np.median(np.array(rows), axis=0)
                print(f"| {he} | {noise} | {N} | {m[0]:.0f} | {m[1]:.2f} | {m[2]:.2f} | {m[3]:.2f} | {m[4]:.4f} | {m[5]:.0f} |", flush=True)


if __name__ == "__main__":
    main()
