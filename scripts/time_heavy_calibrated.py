"""Timing probe (GPU box): ms per whole hot-path call (mocap_match_triangulate_dev_auto: first pass + device-side re-submit, the
call bench.py times) over F resident 64 x 256 stress frames, on the CALIBRATED stress rig (one plain K per camera:
synth.calibrated_stress_rig) and, as control in the same run, on the identical-K stress rig.  HIP events, `reps` runs each, every
run printed; the frames left flagged after the call are counted.  A/B of two library builds: MOCAP_CORE_LIB=<path> picks the
library (the streams are cached in the temporary directory between runs).
    python scripts/time_heavy_calibrated.py [frames=12500] [reps=5]"""
import os, sys, tempfile, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
from mocap_core import capi, devcheck, synth
F = int(sys.argv[1]) if len(sys.argv) > 1 else 12500
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
C, M, K = 64, 256, 384
SEED = int(os.environ.get("TW_SEED", "1"))
dev = torch.device("cuda:0")
print("library", capi.LIB_PATH, flush=True)
for name, rig in (("calibrated", synth.calibrated_stress_rig(C)), ("identical-K", synth.stress_rig(C))):
    cache = os.path.join(tempfile.gettempdir(), f"stress_{name}_{F}_{SEED}.npz")
    if os.path.exists(cache):
        z = np.load(cache); blobs, counts = z["b"], z["c"]
    else:
        blobs, counts, _ = synth.make_stress_stream_chunked(rig, F, M, seed=SEED, threads=16)   # (bench.py's stream)
        np.savez(cache, b=blobs, c=counts)
    core = capi.MocapCore(0)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    d_b = torch.from_numpy(blobs).to(dev); d_c = torch.from_numpy(counts).to(dev)
    out = devcheck.FrameOutputs(F, K, C, dev)
    out.run(core, M, d_b, d_c, synth.STRESS_GATE_PX, 1 << 20); torch.cuda.synchronize()          # warm-up (allocations)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out.run(core, M, d_b, d_c, synth.STRESS_GATE_PX, 1 << 20); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    st = out.status.cpu().numpy(); info = out.info.cpu().numpy()
    print(name, "frames", F, "ms per call", [round(t, 3) for t in ts], "median", round(sorted(ts)[len(ts) // 2], 3), "spread", round(max(ts) - min(ts), 3),
          "| flagged by the first pass", int(info[0]), "re-run", int(info[1]), "left flagged", int((st != 0).sum()),
          "of them intractable", int(((st & capi.ST_INTRACTABLE) != 0).sum()), "| points", int(out.n_out.cpu().numpy()[st == 0].sum()),
          "first-pass kernel", core.last_frame_kernel(), flush=True)
    del core, d_b, d_c, out
