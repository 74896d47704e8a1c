"""GPU: the exact branch-and-bound search on rigs with one intrinsic matrix PER CAMERA (csrc/frame_bb.hip,
frame_bb_calib_kernel).

The reference takes the intrinsics of a view by the position of its camera among the cameras the group sees
(helpers.py:305-307, :231-237), so a view's matrix depends on which cameras below it saw the root: position = camera for a
camera-0 root seen everywhere, lower after a camera that saw nothing, and K[0] with the pose of camera rc for a root created at
a later camera rc.  Every case below is checked for actually containing such views, then compared with the C oracle (indices
exact) and, on the device, bit for bit with the exhaustive walk (csrc/frame_kernel.hip on the same tables).
"""
import os

import numpy as np
import pytest

from conftest import load_golden
from mocap_core import capi, devcheck, synth

pytestmark = pytest.mark.gpu

XYZ_RTOL = 1e-5        # contract (reference-run goldens)
XYZ_RTOL_TIGHT = 1e-9  # against the C restatement (tests/test_gpu_parity.py)
ERR_RTOL = 1e-3


def _ctx(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.MocapCore(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _position_census(corr, n_out):
    """From correspondence indices [F][K][C]: (views whose position among the group's cameras is below their camera number,
    groups whose root camera is not camera 0)."""
    valid = np.arange(corr.shape[1])[None, :] < n_out[:, None]
    seen = (corr >= 0) & valid[:, :, None]
    pos = np.cumsum(seen, axis=2) - seen                      # seen cameras below c
    low = seen & (pos < np.arange(corr.shape[2])[None, None, :])
    late_root = valid & seen.any(axis=2) & ~seen[:, :, 0]
    return int(low.sum()), int(late_root.sum())


def _corr_xy(blobs_f, corr):
    K, C = corr.shape
    out = np.full((K, C, 2), np.nan)
    for r in range(K):
        for c in range(C):
            if corr[r, c] >= 0:
                out[r, c] = blobs_f[c, corr[r, c]]
    return out


def _assert_equals_oracle(res, ref, F):
    assert not res["status"].any()
    assert np.array_equal(res["n_out"], ref["n_out"])
    assert np.array_equal(res["n_cand"], ref["n_cand"])
    kk = res["corr"].shape[1]
    for f in range(F):
        k = int(ref["n_out"][f])
        assert k <= kk
        assert np.array_equal(res["corr"][f, :k], ref["corr"][f, :k]), f"frame {f}"
    valid = np.arange(kk)[None, :] < ref["n_out"][:, None]
    np.testing.assert_allclose(res["xyz"][valid], ref["xyz"][:, :kk][valid], rtol=XYZ_RTOL_TIGHT, atol=1e-12)
    np.testing.assert_allclose(res["err"][valid], ref["err"][:, :kk][valid], rtol=ERR_RTOL, atol=1e-12)


def test_routing_calibrated_rigs_take_the_search(core):
    blobs, counts, _ = synth.make_blob_stream(synth.ring_rig(8), 32, 16, seed=3)
    rig = synth.calibrated_ring_rig(8, seed=1)
    assert all(not np.array_equal(rig["K"][0], k) for k in rig["K"][1:])
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.match_triangulate(blobs, counts)
    kern = core.last_frame_kernel()
    assert kern.startswith("frame_bb_kernel") and kern not in ("frame_bb_kernel<CW=1>", "frame_bb_kernel<CW=2>"), kern
    # one skewed matrix: the eigenvalue bounds do not hold, the general kernel keeps the batch
    skew = rig["K"].copy()
    skew[0, 0, 1] = 0.5
    core.set_cameras(skew, rig["R"], rig["t"])
    core.match_triangulate(blobs, counts)
    assert core.last_frame_kernel().startswith("frame_kernel<"), core.last_frame_kernel()
    # identical intrinsics: the kernel and the name they always had
    same = synth.ring_rig(8)
    core.set_cameras(same["K"], same["R"], same["t"])
    core.match_triangulate(blobs, counts)
    assert core.last_frame_kernel() == "frame_bb_kernel<CW=1>"
    # the exhaustive walk stays the exhaustive walk
    walk = capi.MocapCore(0)
    try:
        walk.set_options(exhaustive_walk=True)
        walk.set_cameras(rig["K"], rig["R"], rig["t"])
        walk.match_triangulate(blobs, counts)
        assert walk.last_frame_kernel() == "frame_kernel<256>"
    finally:
        walk.close()
    off = _ctx({"MOCAP_EVAL_BB": "0"})
    try:
        off.set_cameras(rig["K"], rig["R"], rig["t"])
        off.match_triangulate(blobs, counts)
        assert off.last_frame_kernel() == "frame_kernel<256>"
    finally:
        off.close()


@pytest.mark.parametrize("C,M,F,seed,dropout,vga", [(8, 16, 1500, 31, 0.0, False), (8, 16, 1500, 32, 0.25, False),
                                                    (6, 10, 800, 33, 0.05, False), (3, 20, 800, 34, 0.05, False),
                                                    (16, 8, 100, 39, 0.05, False), (8, 16, 300, 36, 0.05, True)])
def test_calibrated_frame_path_vs_c_oracle(core, C, M, F, seed, dropout, vga):
    from oracle import c_oracle
    rig = (synth.calibrated_ring_rig(C, seed=seed, K=synth.VGA_K, image_size=(640, 480)) if vga
           else synth.calibrated_ring_rig(C, seed=seed))
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=seed, dropout=dropout)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    res = core.match_triangulate_auto(blobs, counts)
    kern = core.last_frame_kernel()
    assert kern == ("frame_bb_kernel<CW=1, per-camera K>" if C <= 8 else "frame_bb_kernel<CW=2, per-camera K>"), kern
    ref = c_oracle.COracle(rig["K"], rig["R"], rig["t"]).match_triangulate(blobs, counts)
    low, late = _position_census(ref["corr"], ref["n_out"])
    print(f"C={C} M={M} dropout={dropout}: views below their camera's position {low}, groups rooted after camera 0 {late}")
    assert low > 0 and late > 0, (low, late)       # the stream exercises positions other than position = camera
    _assert_equals_oracle(res, ref, F)


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    cores = []

    def make(**opts):
        c = capi.MocapCore(0)
        c.set_stream(stream.cuda_stream)
        if opts:
            c.set_options(**opts)
        cores.append(c)
        return c
    yield dev, make
    torch.cuda.synchronize(dev)
    for c in cores:
        c.close()


def _walk_vs_search(gpu, F, K_max, seed, reps, env=None):
    import torch
    dev, make = gpu
    C, M, G_CAP, GATE = 8, 16, 1 << 20, 5.0
    rig = synth.calibrated_ring_rig(C, seed=1)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=seed)
    d_blobs, d_counts = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    shipped, walk = make(), make(exhaustive_walk=True)
    for c in (shipped, walk):
        c.set_cameras(rig["K"], rig["R"], rig["t"])
    ref = devcheck.FrameOutputs(F, K_max, C, dev)
    ref.run(walk, M, d_blobs, d_counts, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert walk.last_frame_kernel() == "frame_kernel<256>"
    assert int((ref.status != 0).sum().item()) == 0 and int(ref.n_out.sum().item()) > 20 * F
    out = devcheck.FrameOutputs(F, K_max, C, dev)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        for rep in range(reps):
            out.zero_()
            out.run(shipped, M, d_blobs, d_counts, GATE, G_CAP)
            cmp = devcheck.compare_bitwise(out, ref)
            assert cmp["frames_differing"] == 0, (rep, cmp)
            assert int((out.status != 0).sum().item()) == 0
            assert torch.equal(out.n_cand, ref.n_cand)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert shipped.last_frame_kernel() == "frame_bb_kernel<CW=1, per-camera K>"


def test_calibrated_100k_frames_equal_the_exhaustive_walk_bit_for_bit(gpu):
    """The bench workload's shape and seed on the calibrated rig: every output bit of every frame, three repetitions."""
    _walk_vs_search(gpu, 100_000, 48, seed=1, reps=3)


def test_calibrated_runtime_layout_equals_the_exhaustive_walk_bit_for_bit(gpu):
    """K_max = 96 lands in the runtime-layout instantiation; MOCAP_BB_FIXED_LAYOUT=0 sends K_max = 48 there as well."""
    _walk_vs_search(gpu, 20_000, 96, seed=2, reps=3)
    _walk_vs_search(gpu, 20_000, 48, seed=2, reps=3, env={"MOCAP_BB_FIXED_LAYOUT": "0"})


def test_calibrated_golden_through_the_search_kernel():
    """frames_c3_calibK: what the reference itself returned on its calibrated matrices, through the search (256 lanes asked
    for, bound tests on every frame)."""
    c = _ctx({"MOCAP_FRAME_THREADS": "256", "MOCAP_BB_MIN_G": "0"})
    try:
        g = load_golden("frames_c3_calibK")
        c.set_cameras(g["K"], g["R"], g["t"])
        res = c.match_triangulate_auto(g["blobs"], g["counts"])
        assert c.last_frame_kernel().startswith("frame_bb_kernel"), c.last_frame_kernel()
        assert not res["status"].any()
        assert np.array_equal(res["n_out"], g["ref_n"])
        for f in range(g["blobs"].shape[0]):
            k = int(g["ref_n"][f])
            assert np.array_equal(_corr_xy(g["blobs"][f], res["corr"][f, :k]), g["ref_corr_xy"][f, :k], equal_nan=True)
            if k:
                np.testing.assert_allclose(res["xyz"][f, :k], g["ref_xyz"][f, :k], rtol=XYZ_RTOL, atol=0)
                np.testing.assert_allclose(res["err"][f, :k], g["ref_err"][f, :k], rtol=ERR_RTOL, atol=1e-12)
    finally:
        c.close()


def _adversarial(case):
    """-> (rig the cameras are set from, blobs, counts)"""
    rig = synth.calibrated_ring_rig(8, seed=7)
    blobs, counts, _ = synth.make_blob_stream(rig, 300, 16, seed=41, dropout=0.1)
    if case == "camera 0 empty":                       # every root is created at a later camera: K[0] with that camera's pose
        counts[:, 0] = 0
        blobs[:, 0] = np.nan
    elif case == "middle camera empty":                # every camera behind it sits one position lower
        counts[:, 3] = 0
        blobs[:, 3] = np.nan
    elif case == "duplicate blobs":                    # bit-equal errors: the first minimum wins
        ok = counts[:, 5] >= 3
        blobs[ok, 5, 2] = blobs[ok, 5, 0]
    elif case == "swapped intrinsics":                 # the stream was projected with K[1] and K[6] the other way round
        rig["K"][[1, 6]] = rig["K"][[6, 1]]
    else:
        raise ValueError(case)
    return rig, blobs, counts


@pytest.mark.parametrize("case", ["camera 0 empty", "middle camera empty", "duplicate blobs", "swapped intrinsics"])
def test_calibrated_adversarial_frames_vs_c_oracle(core, case):
    from oracle import c_oracle
    rig, blobs, counts = _adversarial(case)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    res = core.match_triangulate_auto(blobs, counts)
    assert core.last_frame_kernel() == "frame_bb_kernel<CW=1, per-camera K>"
    ref = c_oracle.COracle(rig["K"], rig["R"], rig["t"]).match_triangulate(blobs, counts)
    assert int(ref["n_out"].sum()) > 1000
    if case == "camera 0 empty":
        valid = np.arange(ref["corr"].shape[1])[None, :] < ref["n_out"][:, None]
        assert (ref["corr"][valid][:, 0] < 0).all()
    if case == "swapped intrinsics":
        # the premise: which matrix a view is given decides correspondences -- the same frames on the unswapped rig differ
        plain = synth.calibrated_ring_rig(8, seed=7)
        other = c_oracle.COracle(plain["K"], plain["R"], plain["t"]).match_triangulate(blobs, counts)
        kk = min(ref["corr"].shape[1], other["corr"].shape[1])
        assert not (np.array_equal(ref["n_out"], other["n_out"]) and np.array_equal(ref["corr"][:, :kk], other["corr"][:, :kk]))
    _assert_equals_oracle(res, ref, blobs.shape[0])


def test_calibrated_self_check_build_reports_no_violation():
    """lib/libmocap_core_eigcheck.so on the 8 x 16 stream with 25 % dropout: every candidate the search cut short and every
    candidate of every dropped block evaluated in full on the device -- no EIGCHECK line, and the counters show the checks ran."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "low-cost-mocap_amd", "lib", "libmocap_core_eigcheck.so")
    assert os.path.exists(lib), "build it with `make -C low-cost-mocap_amd all` (__graft_entry__.build does)"
    code = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import torch
from mocap_core import capi, synth
core = capi.MocapCore(0)
dev = torch.device("cuda:0")
C, M, F, K = 8, 16, 1500, 64
rig = synth.calibrated_ring_rig(C, seed=32)
blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=32, dropout=0.25)
core.set_cameras(rig["K"], rig["R"], rig["t"])
d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev); err = torch.empty((F, K), dtype=torch.float64, device=dev)
corr = torch.empty((F, K, C), dtype=torch.int16, device=dev); n_out = torch.zeros(F, dtype=torch.int32, device=dev)
status = torch.zeros(F + 2, dtype=torch.int32, device=dev)          # + the self-check build's two counters
core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, xyz.data_ptr(), err.data_ptr(),
                           corr.data_ptr(), n_out.data_ptr(), status.data_ptr())
core.synchronize()
assert core.last_frame_kernel() == "frame_bb_kernel<CW=1, per-camera K>", core.last_frame_kernel()
s = status.cpu().numpy()
assert not s[:F].any()
print("CHECKED", int(s[F]), int(s[F + 1]))
""" % (root, os.path.join(root, "low-cost-mocap_amd"))
    env = dict(os.environ, MOCAP_CORE_LIB=lib, MOCAP_BB_MIN_G="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "EIGCHECK" not in p.stdout, p.stdout[:2000]
    checked = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKED")][-1].split()
    print(p.stdout[-300:])
    assert int(checked[1]) > 0 and int(checked[2]) > 0, checked   # cut candidates, candidates of dropped blocks: the checks ran
