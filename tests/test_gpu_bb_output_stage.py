"""GPU: the output stage of the search kernels (csrc/frame_bb.hip, phase E) writes from the winner's record alone.

The lane that evaluates a candidate leaves the point AND the group's packed blob bytes in the (wave, root slot) record of the
workgroup's workspace; phase E builds the correspondence row from those bytes (0xFF -> -1) and no longer decodes the winning
candidate index, so it reads nothing of the frame's matching state.  What can go wrong is new: a row built from another
slot's, another round's or another FRAME's bytes (a workgroup reuses its records frame after frame), a -1 in the wrong place,
the second packed word (more than eight cameras), a frame without a search between two with one, a write outside the frame's
n_out slots.

Every case compares every field of every frame bit for bit (mocap_core.devcheck.compare_bitwise) with the exhaustive walk on a
second context (set_options(exhaustive_walk=True)).  The search's output buffers are pre-filled with a sentinel byte pattern;
the slots at and beyond a frame's n_out must still hold it afterwards (only n_out slots are written).  The walk's
own output may flag at most 1 % of the frames that were not emptied on purpose; on the bench stream it must also hold more
points than frames (the tiny shapes of case 1 have at most one or two points per frame: more points than half the frames).

Streams: seed 1, gate 5 px, G_cap 2^20.  Shapes whose C x M is at most 32 would take the one-wave kernel of tiny frames: their
blob arrays are padded to a wider M with the counts left as they are, which changes no result.
"""
import os

import numpy as np
import pytest

from mocap_core import capi, devcheck, synth

pytestmark = pytest.mark.gpu

GATE, G_CAP = 5.0, 1 << 20
SENTINEL = 0xA5
F_BENCH = 4097          # a few frames per resident workgroup (1 280 on 256 CUs) plus an odd one


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
def bench_np():
    """4 097 frames of the bench's 8 x 16 stream (host arrays, never written)."""
    rig = synth.ring_rig(8)
    blobs, counts, _ = synth.make_blob_stream(rig, F_BENCH, 16, seed=1)
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return rig, blobs, counts


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


@pytest.fixture(scope="module")
def bench_pair(gpu, bench_np):
    """One shipped and one exhaustive-walk context on the bench rig, shared by every case on that rig."""
    return _pair(gpu, bench_np[0])


def _to_dev(dev, blobs, counts):
    import torch
    return torch.from_numpy(np.array(blobs)).to(dev), torch.from_numpy(np.array(counts)).to(dev)   # (copies: the shared arrays are read-only)


def _walk_reference(dev, walk, C, M, K_max, d_blobs, d_counts, kept=None, bench=True):
    """The exhaustive walk's result.  kept: frames that were not emptied on purpose (default: all)."""
    import torch
    F = d_blobs.shape[0]
    ref = devcheck.FrameOutputs(F, K_max, C, dev)
    ref.run(walk, M, d_blobs, d_counts, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert walk.last_frame_kernel().startswith("frame_kernel<"), walk.last_frame_kernel()
    kept = F if kept is None else int(kept)
    flagged = int((ref.status != 0).sum().item())
    points = int(ref.n_out.sum().item())
    assert flagged * 100 <= kept, (flagged, kept)          # at most 1 % flagged frames in the walk's own output
    assert points > (kept if bench else kept // 2), (points, kept)   # ... and points to compare
    return ref


def _sentinel_outputs(F, K_max, C, dev):
    import torch
    out = devcheck.FrameOutputs(F, K_max, C, dev)
    for t in (out.xyz, out.err, out.corr):
        t.view(torch.uint8).fill_(SENTINEL)
    return out


def _untouched_beyond_n_out(out):
    """Slots k >= n_out of every frame still hold the sentinel bytes (a flagged frame reports n_out = 0: none of its slots is written)."""
    import torch
    F, K, C = out.F, out.K, out.C
    beyond = torch.arange(K, device=out.xyz.device)[None, :] >= out.n_out.clamp(0, K)[:, None]
    for name, t, width in (("xyz", out.xyz, 24), ("err", out.err, 8), ("corr", out.corr, 2 * C)):
        raw = t.view(torch.uint8).reshape(F, K, width)
        dirty = ((raw != SENTINEL).any(dim=2) & beyond).any(dim=1)
        assert int(dirty.sum().item()) == 0, (name, torch.nonzero(dirty)[:8, 0].tolist())


def _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, kernel, runs=1, env=None, g_cap=G_CAP):
    """`runs` passes of the shipped search into FRESH sentinel-filled buffers: each equal to the walk, all equal to each other."""
    import torch
    outs = []
    with _env(env):
        for rep in range(runs):
            out = _sentinel_outputs(ref.F, ref.K, ref.C, dev)
            out.run(shipped, M, d_blobs, d_counts, GATE, g_cap)
            outs.append(out)
    torch.cuda.synchronize(dev)
    assert shipped.last_frame_kernel() == kernel, shipped.last_frame_kernel()
    for rep, out in enumerate(outs):
        cmp = devcheck.compare_bitwise(out, ref)
        assert cmp["frames_differing"] == 0, (rep, cmp)
        assert torch.equal(out.n_cand, ref.n_cand), rep
        _untouched_beyond_n_out(out)
    for rep, out in enumerate(outs[1:]):
        cmp = devcheck.compare_bitwise(out, outs[0])
        assert cmp["frames_differing"] == 0, (rep + 1, cmp)
    return outs


def _padded(blobs, counts, M):
    """The same frames in blob arrays M wide (the counts say how many entries of a camera are blobs)."""
    F, C, m, _ = blobs.shape
    wide = np.zeros((F, C, M, 2), dtype=blobs.dtype)
    wide[:, :, :m] = blobs
    return wide, counts.copy()


# ------------------------------------------------------------------------------------------------ 1. rows from bytes

def test_one_root_one_candidate(gpu):
    """2 cameras x 1 blob: one root, one candidate, a row of two entries."""
    dev, _ = gpu
    C, M, F, K_max = 2, 17, 256, 8
    rig = synth.ring_rig(C)
    blobs, counts = _padded(*synth.make_blob_stream(rig, F, 1, seed=1)[:2], M)
    d_blobs, d_counts = _to_dev(dev, blobs, counts)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, K_max, d_blobs, d_counts, bench=False)
    assert int(ref.n_out.max().item()) == 1
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=1>")


def test_root_created_at_camera_one_leads_with_minus_one(gpu):
    """3 cameras, camera 0 sees nothing: every root is created at camera 1 and its row begins with -1."""
    import torch
    dev, _ = gpu
    C, M, F, K_max = 3, 12, 256, 16
    rig = synth.ring_rig(C)
    blobs, counts = _padded(*synth.make_blob_stream(rig, F, 4, seed=1)[:2], M)
    counts[:, 0] = 0
    d_blobs, d_counts = _to_dev(dev, blobs, counts)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, K_max, d_blobs, d_counts, bench=False)
    valid = torch.arange(K_max, device=dev)[None, :] < ref.n_out[:, None]
    assert bool((ref.corr[..., 0][valid] == -1).all()) and bool((ref.corr[..., 1][valid] >= 0).all())
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=1>")


def test_minus_one_in_the_middle_of_the_sixteen_byte_row(gpu, bench_np, bench_pair):
    """8 x 16 with camera 3's count forced to zero: -1 in the middle of the row that is one 16-byte store."""
    import torch
    dev, _ = gpu
    rig, blobs, counts = bench_np
    F, K_max = 1024, 48
    counts = counts[:F].copy()
    counts[:, 3] = 0
    d_blobs, d_counts = _to_dev(dev, blobs[:F], counts)
    shipped, walk = bench_pair
    ref = _walk_reference(dev, walk, 8, 16, K_max, d_blobs, d_counts)
    valid = torch.arange(K_max, device=dev)[None, :] < ref.n_out[:, None]
    assert bool((ref.corr[..., 3][valid] == -1).all())
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>")


def test_sixteen_cameras_use_the_second_packed_word(gpu):
    """16 cameras x 4 blobs: two words of blob bytes per record, camera byte 15 in use, rows written camera by camera."""
    import torch
    dev, _ = gpu
    C, M, F, K_max = 16, 4, 512, 32
    rig = synth.ring_rig(C)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_blobs, d_counts = _to_dev(dev, blobs, counts)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, K_max, d_blobs, d_counts)
    valid = torch.arange(K_max, device=dev)[None, :] < ref.n_out[:, None]
    assert bool((ref.corr[..., 15][valid] >= 0).any())      # camera 15's byte carries blob indices
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=2>")


def test_per_camera_intrinsics(gpu):
    dev, _ = gpu
    C, M, F, K_max = 8, 16, 1024, 48
    rig = synth.calibrated_ring_rig(C, 1)
    blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
    d_blobs, d_counts = _to_dev(dev, blobs, counts)
    shipped, walk = _pair(gpu, rig)
    ref = _walk_reference(dev, walk, C, M, K_max, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, M, d_blobs, d_counts, "frame_bb_kernel<CW=1, per-camera K>")


# ------------------------------------------------------------------------ 2. consecutive frames of one workgroup

def _variant(bench_np, name):
    """-> blobs, counts, frames that were not emptied"""
    _, blobs, counts = bench_np
    counts = counts.copy()
    F = counts.shape[0]
    if name == "plain":
        return blobs, counts, F
    if name == "every second frame empty":        # a frame without a search follows every frame with one
        counts[1::2] = 0
        return blobs, counts, F - len(range(1, F, 2))
    assert name == "every third frame camera 0 alone"   # roots and no candidates
    counts[2::3, 1:] = 0
    return blobs, counts, F - len(range(2, F, 3))


LAYOUTS = [(48, None), (64, None), (48, {"MOCAP_BB_FIXED_LAYOUT": "0"})]
LAYOUT_IDS = ["48-slot layout", "64-slot layout", "runtime layout"]


@pytest.fixture(scope="module")
def walk_refs(gpu, bench_np, bench_pair):
    """The walk's results per (variant, K_max), computed once and shared (never written)."""
    dev, _ = gpu
    cache = {}

    def get(name, K_max):
        if (name, K_max) not in cache:
            blobs, counts, kept = _variant(bench_np, name)
            d_blobs, d_counts = _to_dev(dev, blobs, counts)
            _, walk = bench_pair
            cache[name, K_max] = (d_blobs, d_counts, _walk_reference(dev, walk, 8, 16, K_max, d_blobs, d_counts, kept=kept))
        return cache[name, K_max]
    return get


@pytest.mark.parametrize("K_max,env", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("F", [1, 2, 3])
def test_batches_of_one_two_and_three_frames(gpu, bench_np, bench_pair, K_max, env, F):
    """A workgroup's first frame is also its last; the frames after it belong to other workgroups.  (The points-per-frame
    condition is asserted on the 4 097-frame batches; these few frames hold points: n_out > 0 in the walk.)"""
    import torch
    dev, _ = gpu
    rig, blobs, counts = bench_np
    d_blobs, d_counts = _to_dev(dev, blobs[:F], counts[:F])
    shipped, walk = bench_pair
    ref = devcheck.FrameOutputs(F, K_max, 8, dev)
    ref.run(walk, 16, d_blobs, d_counts, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert int((ref.status != 0).sum().item()) == 0 and int(ref.n_out.sum().item()) > F
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>", env=env)


@pytest.mark.parametrize("K_max,env", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["plain", "every second frame empty", "every third frame camera 0 alone"])
def test_consecutive_frames_of_a_workgroup(gpu, bench_pair, walk_refs, name, K_max, env):
    dev, _ = gpu
    d_blobs, d_counts, ref = walk_refs(name, K_max)
    shipped, _ = bench_pair
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>", env=env)


def test_world_transform_on_consecutive_frames(gpu, bench_np):
    dev, _ = gpu
    rig, blobs, counts = bench_np
    d_blobs, d_counts = _to_dev(dev, blobs, counts)
    W = np.array(synth.APP_TSX_TO_WORLD, dtype=np.float64)
    shipped, walk = _pair(gpu, rig, world=W)
    ref = _walk_reference(dev, walk, 8, 16, 48, d_blobs, d_counts)
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>")


# ------------------------------------------------------------------------------------------------ 3. run to run

def test_five_passes_equal_each_other_and_the_walk(gpu, bench_pair, walk_refs):
    """A record overwritten before it was read, or a row written from another frame's bytes, depends on timing."""
    dev, _ = gpu
    d_blobs, d_counts, ref = walk_refs("plain", 48)
    shipped, _ = bench_pair
    _runs_equal_walk(dev, shipped, ref, 16, d_blobs, d_counts, "frame_bb_kernel<CW=1>", runs=5)


# ------------------------------------------------------------------------------------------------ 4. two launches

def test_second_pass_right_behind_the_first(gpu, bench_pair, walk_refs):
    """G_cap = 64 flags frames: the re-submit's second pass (another layout, the same workspace) is queued right behind the
    first pass, whose last frames' outputs must be written before it exits.  Both passes' results equal the walk."""
    import torch
    dev, _ = gpu
    d_blobs, d_counts, ref = walk_refs("plain", 48)
    shipped, _ = bench_pair
    outs = []
    for rep in range(2):
        out = _sentinel_outputs(ref.F, ref.K, ref.C, dev)
        out.run(shipped, 16, d_blobs, d_counts, GATE, 64)
        outs.append(out)
    torch.cuda.synchronize(dev)
    for rep, out in enumerate(outs):
        flagged, rerun = out.info.cpu().tolist()
        assert flagged >= 1 and rerun == flagged, (rep, flagged, rerun)
        cmp = devcheck.compare_bitwise(out, ref)
        assert cmp["frames_differing"] == 0, (rep, cmp)
        _untouched_beyond_n_out(out)
