"""GPU: the winners' records of the search kernels (csrc/frame_bb.hip, phase E).

The lane that evaluates a candidate leaves its point in a per-(wave, root slot) record of the workgroup's workspace, and the
output stage reads the record of the winning slot instead of solving for the point again.  What can go wrong is new: a record
of an EARLIER frame (a workgroup reuses its addresses frame after frame) or of an earlier evaluation round (a slot is re-won)
read in place of the current one, a record read before its store has landed, the wrong wave's record.  So every case runs
more frames than there are resident workgroups and frames with several evaluation rounds, and compares every output bit with
the exhaustive walk on a second context (set_options(exhaustive_walk=True): every candidate group triangulated and
reprojected, no bound, no record), on the device (mocap_core/devcheck.py).  Each case checks that at most 1 % of the frames
are flagged in the walk's own output, so that it cannot pass on frames without points.

Streams: seed 1, gate 5 px; checked with the oracle's matcher: no frame has more than 2^20 groups or more than 41 roots.
"""
import os

import numpy as np
import pytest

from mocap_core import capi, devcheck, synth

pytestmark = pytest.mark.gpu

GATE, G_CAP = 5.0, 1 << 20


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


@pytest.fixture(scope="module")
def bench_stream(gpu):
    """4 096 frames of the bench's 8 x 16 stream, on the device (shared, never written)."""
    import torch
    dev, _ = gpu
    rig = synth.ring_rig(8)
    blobs, counts, _ = synth.make_blob_stream(rig, 4096, 16, seed=1)
    return rig, torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)


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


def _pair(gpu, rig, world=None):
    _, make = gpu
    shipped, walk = make(), make(exhaustive_walk=True)
    for c in (shipped, walk):
        c.set_cameras(rig["K"], rig["R"], rig["t"])
        if world is not None:
            c.set_world_transform(world)
    return shipped, walk


def _walk_reference(dev, walk, C, M, F, K_max, d_blobs, d_counts):
    import torch
    ref = devcheck.FrameOutputs(F, K_max, C, dev)
    ref.run(walk, M, d_blobs, d_counts, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert walk.last_frame_kernel().startswith("frame_kernel<"), walk.last_frame_kernel()
    flagged = int((ref.status != 0).sum().item())
    assert flagged * 100 <= F, (flagged, F)                # at most 1 % flagged frames in the walk's own output
    assert int(ref.n_out.sum().item()) > F                 # ... and points to compare
    return ref


def _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, kernel, runs, env=None):
    """`runs` passes of the shipped search into FRESH output buffers: each equal to the walk, all equal to each other."""
    import torch
    outs = []
    with _env(env):
        for rep in range(runs):
            out = devcheck.FrameOutputs(ref.F, ref.K, ref.C, dev)
            out.run(shipped, M, d_blobs, d_counts, GATE, G_CAP)
            outs.append(out)
    torch.cuda.synchronize(dev)
    assert shipped.last_frame_kernel() == kernel, shipped.last_frame_kernel()
    for rep, out in enumerate(outs):
        cmp = devcheck.compare_bitwise(out, ref)
        assert cmp["frames_differing"] == 0, (rep, cmp)
        assert torch.equal(out.n_cand, ref.n_cand)
    for rep, out in enumerate(outs[1:]):
        cmp = devcheck.compare_bitwise(out, outs[0])
        assert cmp["frames_differing"] == 0, (rep + 1, cmp)


@pytest.mark.parametrize("K_max,env", [(48, None), (64, None), (48, {"MOCAP_BB_FIXED_LAYOUT": "0"})],
                         ids=["48-slot layout", "64-slot layout", "runtime layout"])
def test_bench_stream_three_runs_equal_each_other_and_the_walk(gpu, bench_stream, K_max, env):
    dev, _ = gpu
    rig, d_blobs, d_counts = bench_stream
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, 8, 16, 4096, K_max, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>", 3, env)


def test_frames_of_many_evaluation_rounds_equal_the_walk(gpu):
    """8 x 24: 95 % of these frames have more than 256 blocks (median 726), so slots are won again over several rounds and
    their records overwritten."""
    import torch
    dev, _ = gpu
    C, M, F, K_max = 8, 24, 1024, 64
    rig = synth.ring_rig(C)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_blobs, d_counts = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, F, K_max, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=1>", 1)


def test_per_camera_intrinsics_equal_the_walk(gpu):
    import torch
    dev, _ = gpu
    C, M, F, K_max = 8, 16, 2048, 48
    rig = synth.calibrated_ring_rig(C, 1)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_blobs, d_counts = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, F, K_max, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=1, per-camera K>", 1)


def test_twelve_cameras_equal_the_walk(gpu):
    """More than eight cameras: two words of blob indices per group (CW = 2), the output rows written camera by camera."""
    import torch
    dev, _ = gpu
    C, M, F, K_max = 12, 8, 1024, 48
    rig = synth.ring_rig(C)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_blobs, d_counts = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, F, K_max, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=2>", 1)


def test_world_transform_on_the_stored_point_equals_the_walk(gpu, bench_stream):
    dev, _ = gpu
    rig, d_blobs, d_counts = bench_stream
    F = 1024
    W = np.array(synth.APP_TSX_TO_WORLD, dtype=np.float64)
    shipped, walk = _pair(gpu, rig, world=W)
    ref = _walk_reference(dev, walk, 8, 16, F, 48, d_blobs[:F], d_counts[:F])
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs[:F], d_counts[:F], "frame_bb_kernel<CW=1>", 1)
    plain, _ = _pair(gpu, rig)                              # the epilogue did run: the points differ from the camera frame's
    cam = devcheck.FrameOutputs(F, 48, 8, dev)
    cam.run(plain, 16, d_blobs[:F], d_counts[:F], GATE, G_CAP)
    assert devcheck.compare_bitwise(cam, ref)["fields"]["xyz"] > F // 2


def test_second_pass_right_behind_the_first_and_the_empty_second_pass(gpu, bench_stream):
    """G_cap = 64 flags frames: the re-submit's second pass (another layout, queues of its own) runs right behind the first on
    the same context and workspace.  Then a call that flags nothing -- every workgroup of the second pass leaves before it
    touches a queue counter -- and at once the G_cap = 64 call again: the counters behind the early return were left as the
    next launch needs them."""
    import torch
    dev, make = gpu
    rig, d_blobs, d_counts = bench_stream
    C, M, F, K_max = 8, 16, 4096, 48
    core = make()
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    want = devcheck.FrameOutputs(F, K_max, C, dev)
    want.run(core, M, d_blobs, d_counts, GATE, G_CAP, auto=False)
    torch.cuda.synchronize(dev)
    assert int((want.status != 0).sum().item()) == 0 and int(want.n_out.sum().item()) > F

    def capped():
        out = devcheck.FrameOutputs(F, K_max, C, dev)
        out.run(core, M, d_blobs, d_counts, GATE, 64)
        return out

    first = capped()
    nothing = devcheck.FrameOutputs(F, K_max, C, dev)
    nothing.run(core, M, d_blobs, d_counts, GATE, G_CAP)    # flags nothing: the second pass finds an empty list
    again = capped()
    torch.cuda.synchronize(dev)
    flagged, rerun = first.info.cpu().tolist()
    assert flagged >= 1 and rerun == flagged, (flagged, rerun)
    assert nothing.info.cpu().tolist() == [0, 0]
    assert again.info.cpu().tolist() == [flagged, rerun]
    for name, out in (("capped", first), ("nothing flagged", nothing), ("capped again", again)):
        cmp = devcheck.compare_bitwise(out, want)
        assert cmp["frames_differing"] == 0, (name, cmp)
