"""Where a frame's time goes in the search kernel (GPU box): the shares of its phases, from the measuring build.

   make -C low-cost-mocap_amd lib/libmocap_core_phaseclocks.so
   python scripts/time_frame_phases.py [--lib PATH] [--frames F] [--calibrated]

bench.py's 8 x 16 workload (100 000 frames, K_max = 48, stream seed 1) once through lib/libmocap_core_phaseclocks.so
(csrc/frame_bb.hip with -DMOCAP_BB_PHASE_CLOCKS): wave 0 of every workgroup reads the cycle counter behind the barriers
that separate the phases and the workgroups add their sums, in units of 256 cycles, to eleven counters behind the status
array.  The clocks cost registers (the measuring build of the headline kernel spills where the product does not) and wave 0's
issue slots, so the figures are SHARES of a workgroup's time in the frame loop, not times: use them to rank the phases, and
time the product library with scripts/time_calibrated_rig.py.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
PHASES = ("other: buffer swap, status stores, the loop", "B0: camera-0 pairs", "B0: provisional pairs", "B1 and the per-blob table",
          "the row copy", "phase C and its scans", "D: the seed pass", "D: the seed push", "D: evaluation rounds", "D: test rounds",
          "phase E (with the search's last wait)")
C, M, K_MAX, GATE, G_CAP = 8, 16, 48, 5.0, 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "low-cost-mocap_amd", "lib", "libmocap_core_phaseclocks.so"))
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--calibrated", action="store_true", help="the rig with one intrinsic matrix per camera")
    a = ap.parse_args()
    os.environ["MOCAP_CORE_LIB"] = os.path.abspath(a.lib)   # (read when mocap_core.capi is imported)
    import torch
    from mocap_core import capi, synth
    rig = synth.calibrated_ring_rig(C, seed=1) if a.calibrated else synth.ring_rig(C)
    F = a.frames
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    dev = torch.device("cuda:0")
    core = capi.MocapCore(0)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    xyz = torch.empty((F, K_MAX, 3), dtype=torch.float64, device=dev)
    err = torch.empty((F, K_MAX), dtype=torch.float64, device=dev)
    corr = torch.empty((F, K_MAX, C), dtype=torch.int16, device=dev)
    n_out = torch.zeros(F, dtype=torch.int32, device=dev)
    status = torch.zeros(F + len(PHASES), dtype=torch.int32, device=dev)   # + the measuring build's counters
    core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), GATE, K_MAX, G_CAP, xyz.data_ptr(), err.data_ptr(),
                               corr.data_ptr(), n_out.data_ptr(), status.data_ptr())
    core.synchronize()
    kernel = core.last_frame_kernel()
    s = status.cpu().numpy()
    core.close()
    units = s[F:].astype("int64")
    assert units.sum() > 0, "no counts: is %s the measuring build?" % a.lib
    print("%s, %d frames of %d x %d, %d points, %d frames flagged" % (kernel, F, C, M, int(n_out.sum().item()), int((s[:F] != 0).sum())))
    print("shares of a workgroup's cycles in the frame loop (measuring build: not times)")
    for name, u in zip(PHASES, units):
        print("  %-46s %5.1f %%" % (name, 100.0 * u / units.sum()))


if __name__ == "__main__":
    main()
