"""GPU: the evaluation path of the search kernels (csrc/frame_bb.hip, csrc/mocap_device.hpp) after round 11.

Round 11 took instructions and waits out of the path a candidate takes, none of which may show in a result:
  * score_point: the pairwise partial sums are born in the first group of four cameras (a view's pair is its two squares, or
    zeros when the camera is not seen) and that group is no longer guarded by the limit;
  * a group's DLT sum starts from camera 0's table record (the table holds 0.0 + contribution) instead of from zeros;
  * the barriers between the search's rounds wait for LDS alone (block_sync_lds_only): a round no longer waits for its
    winner-record stores, and the prefetched frame is waited for once, at the search's entry.

What can go wrong: a record read before its store landed or a prefetch buffer read before it is complete (every workgroup must
swap its buffer several times: more frames than 3 x the resident workgroups), a view that is not seen (left-to-right sum),
camera 0 not in the group (the sum starts from the record of zeros), layouts with no group of four, a tail behind the groups,
two-word records, and the matching's two ways to the provisional roots (pre-matched up to 64 and while their staging rows
fit the layout; the chain over the cameras beyond).  Every case compares every bit of n_out, status, corr, xyz and err
(mocap_core.devcheck.compare_bitwise) and n_cand with the exhaustive walk on a second context
(set_options(exhaustive_walk=True)); the hand-built cases assert on the CPU, with the oracle's matching, that their frames
are at the edge they are named for.

Streams: seed 1, gate 5 px, G_cap 2^20.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from mocap_core import capi, devcheck, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE, G_CAP = 5.0, 1 << 20
RIGS = {"identical K": lambda C: synth.ring_rig(C), "per-camera K": lambda C: synth.calibrated_ring_rig(C, 1)}
KERNELS = {"identical K": "frame_bb_kernel<CW=%d>", "per-camera K": "frame_bb_kernel<CW=%d, per-camera K>"}


class _env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    cores = {}

    def make(walk=False, f32=True):
        """One context per (walk, float32 rounding)."""
        if (walk, f32) not in cores:
            c = capi.MocapCore(0)
            c.set_stream(stream.cuda_stream)
            c.set_options(f32_rounding=f32, exhaustive_walk=walk)
            cores[walk, f32] = c
        return cores[walk, f32]
    yield dev, make
    torch.cuda.synchronize(dev)
    for c in cores.values():
        c.close()


def _to_dev(dev, blobs, counts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(blobs)).to(dev), torch.from_numpy(np.ascontiguousarray(counts)).to(dev)


def _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points, f32=True):
    import torch
    dev, make = gpu
    walk = make(walk=True, f32=f32)
    walk.set_cameras(rig["K"], rig["R"], rig["t"])
    ref = devcheck.FrameOutputs(d_b.shape[0], K_max, C, dev)
    ref.run(walk, M, d_b, d_c, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert walk.last_frame_kernel().startswith("frame_kernel<"), walk.last_frame_kernel()
    assert int((ref.status != 0).sum().item()) * 100 <= ref.F, "more than 1 % of the walk's frames flagged"
    assert int(ref.n_out.sum().item()) >= min_points, (int(ref.n_out.sum().item()), min_points)
    return ref


def _search_equals(gpu, rig, ref, M, d_b, d_c, kernel, runs=1, run_env=None, f32=True):
    """`runs` passes of the shipped search into fresh buffers: each equal to the walk, hence to each other."""
    import torch
    dev, make = gpu
    core = make(f32=f32)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    outs = []
    with _env(run_env):
        for _ in range(runs):
            out = devcheck.FrameOutputs(ref.F, ref.K, ref.C, dev)
            out.run(core, M, d_b, d_c, GATE, G_CAP)
            outs.append(out)
    torch.cuda.synchronize(dev)
    assert core.last_frame_kernel() == kernel, core.last_frame_kernel()
    for rep, out in enumerate(outs):
        cmp = devcheck.compare_bitwise(out, ref)
        assert cmp["frames_differing"] == 0, (rep, cmp)
        assert torch.equal(out.n_cand, ref.n_cand), rep


# ------------------------------------------------------------------------------------------------ 1. buffer swaps

@pytest.mark.parametrize("K_max", [48, 64])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_every_workgroup_swaps_its_prefetch_buffer(gpu, rig_name, K_max):
    """F = 3 x (CUs x 5) + 7 frames of the bench's 8 x 16 stream -- five workgroups per CU is the most any layout keeps resident,
    so every workgroup takes at least three frames -- ten passes, each equal to the walk."""
    import torch
    dev, _ = gpu
    F = 3 * torch.cuda.get_device_properties(dev).multi_processor_count * 5 + 7
    rig = RIGS[rig_name](8)
    blobs, counts, _ = synth.make_blob_stream(rig, F, 16, seed=1)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, 8, 16, K_max, d_b, d_c, min_points=F)
    _search_equals(gpu, rig, ref, 16, d_b, d_c, KERNELS[rig_name] % 1, runs=10)


# ------------------------------------------------------------------------------------------------ 2. hand-built frames

def n_provisional(Ftab, blobs_f, counts_f):
    """Blobs of cameras 1 .. C-1 that no camera-0 root claims (helpers.py:391 by value): the kernel's n_prov of the frame."""
    from oracle import mocap_oracle as mo
    C = blobs_f.shape[0]
    n = 0
    for i in range(1, C):
        n_i = int(counts_f[i])
        if n_i == 0:
            continue
        px, py = blobs_f[i, :n_i, 0].astype(np.float64), blobs_f[i, :n_i, 1].astype(np.float64)
        claimed = np.zeros(n_i, dtype=bool)
        for rb in range(int(counts_f[0])):
            a, b, c = mo.epiline(Ftab[0, i], blobs_f[0, rb])
            d = np.abs(a * px + b * py + c) / np.sqrt(a ** 2 + b ** 2)
            idx = [k for k in range(n_i) if d[k] < GATE]
            if idx:
                k0 = min(idx, key=lambda k: (d[k], k))
                claimed |= (px == px[k0]) & (py == py[k0])
        n += int((~claimed).sum())
    return n


def _frames_with_n_prov(rig, C, M, target, n_frames=6):
    """-> blobs, counts: frames of the seed-1 stream cut down, blob by blob from the last camera backwards, until exactly
    `target` blobs of cameras 1 .. C-1 are left unclaimed by the camera-0 roots (asserted).  A large target starts from one
    camera-0 root (nearly every other blob is provisional), a small one from clean frames of two well separated markers."""
    from oracle import mocap_oracle as mo
    Ftab = mo.fundamental_table(rig["K"], rig["R"], rig["t"])
    if target <= 1:
        blobs, counts, _ = synth.make_blob_stream(rig, 64, 2, seed=1, m_max=M, dropout=0.0, min_sep=0.6)
    else:
        blobs, counts, _ = synth.make_blob_stream(rig, 4 * n_frames, M, seed=1, dropout=0.0)
        counts[:, 0] = np.minimum(counts[:, 0], 1)
    got_b, got_c = [], []
    for f in range(blobs.shape[0]):
        b, c = blobs[f].copy(), counts[f].copy()
        if c[0] < 1:
            continue
        n = n_provisional(Ftab, b, c)
        if target == 1 and n == 0 and c[C - 1] < M:
            # one blob more in the last camera, away from every camera-0 root's line
            for xy in ((3.0, 5.0), (600.0, 7.0), (5.0, 440.0), (610.0, 450.0), (320.0, 3.0)):
                b[C - 1, c[C - 1]] = xy
                c[C - 1] += 1
                n = n_provisional(Ftab, b, c)
                if n == 1:
                    break
                c[C - 1] -= 1
                b[C - 1, c[C - 1]] = np.nan
                n = 0
        cam = C - 1
        while n > target:              # (a blob less changes n_prov by 0 or -1: the walk down cannot jump over the target)
            if c[cam] > 1:
                c[cam] -= 1
                b[cam, c[cam]] = np.nan
                n = n_provisional(Ftab, b, c)
            cam = cam - 1 if cam > 1 else C - 1
            if all(c[i] <= 1 for i in range(1, C)):
                break
        if n == target:
            got_b.append(b)
            got_c.append(c)
        if len(got_b) == n_frames:
            break
    assert len(got_b) >= 2, "n_prov = %d: the stream gave %d such frames" % (target, len(got_b))
    blobs, counts = np.stack(got_b), np.stack(got_c)
    assert all(n_provisional(Ftab, blobs[f], counts[f]) == target for f in range(blobs.shape[0]))
    return blobs, counts


# n_prov at 8 x 16 / 48 slots: the pre-matched path ends where the staging rows stop fitting the layout's scratch (200 bytes a
# provisional root, 8 000 bytes: 40), long before 64 -- 63, 64 and 65 all take the chain there; at 4 x 32 / 128 slots (164 bytes
# a root, 12 800 bytes) it is the limit of 64 itself that decides.
@pytest.mark.parametrize("C,M,K_max,target", [(8, 16, 48, t) for t in (0, 1, 40, 41, 63, 64, 65)] + [(4, 32, 128, t) for t in (63, 64, 65)])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_provisional_roots_at_the_edges(gpu, rig_name, C, M, K_max, target):
    dev, _ = gpu
    rig = RIGS[rig_name](C)
    blobs, counts = _frames_with_n_prov(rig, C, M, target)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=blobs.shape[0])
    _search_equals(gpu, rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1)
    if C == 8:
        _search_equals(gpu, rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1, run_env={"MOCAP_BB_FIXED_LAYOUT": "0"})


def _views(name, rig):
    """-> blobs, counts (8 x 16, 96 frames), a predicate on a frame's (roots, hits) that says the frame is what the case names."""
    blobs, counts, _ = synth.make_blob_stream(rig, 96, 12, seed=1, m_max=16)
    if name == "two views only":
        keep = np.zeros(8, dtype=bool)
        keep[[0, 5]] = True
        counts[:48, ~keep] = 0
        keep[:] = False
        keep[[3, 6]] = True                     # ... and a pair without camera 0
        counts[48:, ~keep] = 0
        return blobs, counts, lambda roots, hits: any(sum(1 for h in hr if h) == 1 for hr in hits)
    if name == "a camera with no blobs":
        counts[:, 3] = 0                        # seven views at most: the left-to-right sum, camera 3's pair of squares zeros
        counts[1::2, 6] = 0
        return blobs, counts, lambda roots, hits: any(rc == 0 and sum(1 for h in hr if h) >= 5 for (rc, _), hr in zip(roots, hits))
    assert name == "camera 0 empty"
    counts[:, 0] = 0                            # every root is created at camera 1 or later: sums start from the record of zeros
    return blobs, counts, lambda roots, hits: bool(roots) and all(rc >= 1 for rc, _ in roots) and any(any(h for h in hr) for hr in hits)


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("name", ["two views only", "a camera with no blobs", "camera 0 empty"])
def test_views_that_are_not_there(gpu, name, rig_name):
    from oracle import mocap_oracle as mo
    dev, _ = gpu
    rig = RIGS[rig_name](8)
    blobs, counts, want = _views(name, rig)
    Ftab = mo.fundamental_table(rig["K"], rig["R"], rig["t"])
    for f in (0, 1, 50, 51):
        assert want(*mo.match_frame(blobs[f].astype(np.float64), counts[f], Ftab, gate_px=GATE)), (name, f)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, 8, 16, 48, d_b, d_c, min_points=blobs.shape[0])
    _search_equals(gpu, rig, ref, 16, d_b, d_c, KERNELS[rig_name] % 1)
    _search_equals(gpu, rig, ref, 16, d_b, d_c, KERNELS[rig_name] % 1, run_env={"MOCAP_BB_FIXED_LAYOUT": "0"})


# ------------------------------------------------------------------------------------------------ 3. runtime layouts

@pytest.mark.parametrize("f32", [True, False], ids=["float32 rounding", "no float32 rounding"])
@pytest.mark.parametrize("C,cw", [(3, 1), (5, 1), (12, 2)], ids=["3 cameras: no group of four", "5 cameras: the tail loop", "12 cameras: two-word records"])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_runtime_layouts(gpu, rig_name, C, cw, f32):
    """M = 8 markers, 500 frames, with and without MOCAP_OPT_F32_ROUNDING.  (3 x 8 would go to the one-wave kernel of tiny
    frames: its blob arrays are padded to 12 slots per camera with the counts left as they are, which changes no result.)"""
    dev, _ = gpu
    M, F = 8, 500
    rig = RIGS[rig_name](C)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    Mw = M
    if C * M <= 32:
        Mw = 12
        wide = np.full((F, C, Mw, 2), np.nan, dtype=blobs.dtype)
        wide[:, :, :M] = blobs
        blobs = wide
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, Mw, 48, d_b, d_c, min_points=F // 2, f32=f32)
    _search_equals(gpu, rig, ref, Mw, d_b, d_c, KERNELS[rig_name] % cw, f32=f32)


# ------------------------------------------------------------------------------------------------ 4. the live call

@pytest.mark.parametrize("rig_name", list(RIGS))
def test_one_frame_per_call(gpu, rig_name):
    """F = 1, the live call: one workgroup, no second frame to prefetch; twelve frames one by one."""
    dev, _ = gpu
    rig = RIGS[rig_name](8)
    blobs, counts, _ = synth.make_blob_stream(rig, 12, 16, seed=1)
    for f in range(12):
        d_b, d_c = _to_dev(dev, blobs[f:f + 1], counts[f:f + 1])
        ref = _walk(gpu, rig, 8, 16, 48, d_b, d_c, min_points=1)
        _search_equals(gpu, rig, ref, 16, d_b, d_c, KERNELS[rig_name] % 1)


# ------------------------------------------------------------------------------------------------ 5. the self-check build

_EIGCHECK_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import torch
from mocap_core import capi, synth
core = capi.MocapCore(0)
dev = torch.device("cuda:0")
rig = synth.ring_rig(8)
F, C, M, K = 2000, 8, 16, 48
blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
core.set_cameras(rig["K"], rig["R"], rig["t"])
d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev); err = torch.empty((F, K), dtype=torch.float64, device=dev)
corr = torch.empty((F, K, C), dtype=torch.int16, device=dev); n_out = torch.zeros(F, dtype=torch.int32, device=dev)
status = torch.zeros(F + 2, dtype=torch.int32, device=dev)          # + the self-check build's two counters
core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, xyz.data_ptr(), err.data_ptr(),
                           corr.data_ptr(), n_out.data_ptr(), status.data_ptr())
core.synchronize()
assert core.last_frame_kernel().startswith("frame_bb_kernel")
s = status.cpu().numpy()
print("CHECKED", int(s[F]), int(s[F + 1]))
"""


def test_self_check_build_on_two_thousand_frames():
    """lib/libmocap_core_eigcheck.so on 2 000 frames of 8 x 16: every candidate whose evaluation was cut short and every
    candidate of every dropped block is evaluated in full on the device against the bound it was cut on.  Neither check
    reports a violation (no EIGCHECK line of either kind), and the two counters show that both checks did run."""
    lib = os.path.join(ROOT, "low-cost-mocap_amd", "lib", "libmocap_core_eigcheck.so")
    assert os.path.exists(lib), "build it with `make -C low-cost-mocap_amd all` (__graft_entry__.build does)"
    code = _EIGCHECK_CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "low-cost-mocap_amd")}
    env = dict(os.environ, MOCAP_CORE_LIB=lib)
    for k in ("MOCAP_BB_PL", "MOCAP_BB_PL_MIN", "MOCAP_BB_NB_MAX", "MOCAP_BB_FIXED_LAYOUT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "EIGCHECK candidate" not in p.stdout and "EIGCHECK block" not in p.stdout, p.stdout[:2000]
    checked = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKED")][-1].split()
    assert int(checked[1]) > 1000 and int(checked[2]) > 100000, checked   # cut candidates, candidates of dropped blocks
