"""Timing for DESIGN.md 3.7i: the tracker kernel per frame in a 10 000-frame batch, and the one-frame live call."""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "low-cost-mocap_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
from mocap_core import capi, synth
import body_track_reference as br

core = capi.MocapCore(0)
dev = torch.device("cuda", 0)
out = {}
# ---- (a) 10 000 frames, two bodies, K_max = 32
rng = np.random.default_rng(1)
bodies = [br.make_body(rng, 5), br.make_body(rng, 6)]
F, K, B = 10000, 32, 2
t, xyz, n_pts, _ = br.path_scene(rng, bodies, F, K, 8, br._PATHS[:2])
core.set_rigid_bodies(bodies, tol=0.01, max_rms=0.005)
core.set_body_tracker()
d_t = torch.from_numpy(t).to(dev); d_xyz = torch.from_numpy(np.nan_to_num(xyz, nan=1e6)).to(dev); d_n = torch.from_numpy(n_pts).to(dev)
i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
bt = [i32(F, B), i32(F, B), i32(F, B), torch.zeros((F, B, 8), dtype=torch.int8, device=dev), f64(F, B, 9), f64(F, B, 3), f64(F, B), i32(F, B), i32(F, B), i32(F)]
rb = [i32(F, B), i32(F, B), torch.zeros((F, B, 8), dtype=torch.int8, device=dev), f64(F, B, 9), f64(F, B, 3), f64(F, B), f64(F, B), i32(F, B)]
torch.cuda.synchronize()
def both():
    core.reset_body_tracker()
    core.synchronize()
    t0 = time.perf_counter()
    core.track_bodies_dev(F, d_t.data_ptr(), K, d_xyz.data_ptr(), d_n.data_ptr(), B, *[x.data_ptr() for x in bt])
    core.synchronize()
    return time.perf_counter() - t0
def search():
    core.synchronize()
    t0 = time.perf_counter()
    core.locate_rigid_bodies_dev(F, K, d_xyz.data_ptr(), d_n.data_ptr(), B, *[x.data_ptr() for x in rb])
    core.synchronize()
    return time.perf_counter() - t0
for _ in range(2):
    both(); search()
tb, ts = [], []
for _ in range(7):
    tb.append(both()); ts.append(search())
src = bt[1].cpu().numpy()
out["batch"] = {"frames": F, "search_plus_tracker_ms": sorted(tb)[3] * 1e3, "search_ms": sorted(ts)[3] * 1e3,
                "tracker_us_per_frame": (sorted(tb)[3] - sorted(ts)[3]) / F * 1e6, "all_ms": [round(x * 1e3, 3) for x in tb],
                "sources": np.bincount(src.ravel(), minlength=4).tolist()}
print(json.dumps(out["batch"]), flush=True)
# the rigid-body kernel alone at its own bench shape (100 000 frames, two bodies): the shared pose header must not have slowed it
F2 = 100000
reps = F2 // F
d_xyz2 = d_xyz.repeat(reps, 1, 1).contiguous(); d_n2 = d_n.repeat(reps).contiguous()
rb2 = [i32(F2, B), i32(F2, B), torch.zeros((F2, B, 8), dtype=torch.int8, device=dev), f64(F2, B, 9), f64(F2, B, 3), f64(F2, B), f64(F2, B), i32(F2, B)]
torch.cuda.synchronize()
tt = []
for i in range(7):
    core.synchronize(); t0 = time.perf_counter()
    core.locate_rigid_bodies_dev(F2, K, d_xyz2.data_ptr(), d_n2.data_ptr(), B, *[x.data_ptr() for x in rb2])
    core.synchronize(); tt.append(time.perf_counter() - t0)
out["search_100k_ms"] = sorted(tt[2:])[2] * 1e3
print(json.dumps({"search_100k_ms": out["search_100k_ms"]}), flush=True)
# ---- (b) the one-frame live call
rig = synth.ring_rig(4)
q = [br.make_body(np.random.default_rng(5), 4), br.make_body(np.random.default_rng(6), 4)]
def plant(sampled):
    o = sampled.copy()
    for f in range(o.shape[0]):
        o[f, :4] = (br._rot([0, 0, 1], 0.03 * f) @ q[0].T).T + np.array([0.1 + 0.004 * f, -0.2, 0.3])
        o[f, 4:8] = (br._rot([0, 1, 0], 0.02 * f) @ q[1].T).T + np.array([-0.3, 0.2 + 0.004 * f, -0.1])
    return o
NF = 64
blobs, counts, _ = synth.make_blob_stream(rig, NF, 10, seed=23, noise_px=0.02, dropout=0.0, truncate=False, world=plant)
tl = 70.0 + np.arange(NF) / 60.0
core.set_cameras(rig["K"], rig["R"], rig["t"])
core.set_rigid_bodies(q, tol=0.01, max_rms=0.005)
core.set_body_tracker()
def live(tracked, f):
    t0 = time.perf_counter()
    if tracked:
        r = core.track_frame_bodies_tracked(blobs[f:f + 1], counts[f:f + 1], tl[f:f + 1], K_max=32, O_max=4)
    else:
        r = core.track_frame_bodies(blobs[f:f + 1], counts[f:f + 1], K_max=32, O_max=4)
    return time.perf_counter() - t0, r
for f in range(NF):
    live(True, f); live(False, f)
a, b, srcs = [], [], []
for rep in range(6):
    core.reset_body_tracker()
    for f in range(NF):
        x, r = live(True, f); a.append(x); srcs.append(r["source"][0].tolist())
        y, _ = live(False, f); b.append(y)
out["live"] = {"calls": len(a), "tracked_p50_us": float(np.median(a)) * 1e6, "bodies_p50_us": float(np.median(b)) * 1e6,
               "tracked_p90_us": float(np.percentile(a, 90)) * 1e6, "bodies_p90_us": float(np.percentile(b, 90)) * 1e6,
               "sources": np.bincount(np.array(srcs).ravel(), minlength=4).tolist()}
print(json.dumps(out["live"]), flush=True)



