"""GPU: the search kernels' fixed layouts (8 cameras x 16 blobs, 48 or 64 root slots) after round 14 (csrc/frame_bb.hip).

Round 14 changed HOW three pieces of a frame's serial path get their values, none of which may show in a result:
  * the search's decodes (fetch_candidate, block_pk) read a root's row of `act` and of `nh` as one 64-bit word each and take a
    digit's camera and hit count by shift and mask; only the digit's `hits` byte is still a dependent read;
  * phase C builds a root's shared bytes, its act row, its counts and its block size in registers from the nh word and seven
    independent reads -- the bytes of cameras at or below the root's own camera, which nothing writes for that root, are
    masked out of the word -- and decides the G_cap overflow on the full product;
  * the pair loop of stages 0 and 1 keeps the closest hit while it walks the camera's blobs: position 0 needs no pass, a list
    of one claims itself, the last hit left of any list is placed without a distance.

What can go wrong: a stale byte below a root's camera read as a hit count, a digit taken from the wrong byte of a word, the
sixteenth hit of a camera (count - 1 = 15 in the digit's byte), seven digits (the whole word), an overflow that the loop found
at an early camera and the product must find as well, block sizes under every rule the block-size tests sweep, lists of one,
two, three and more hits in either stage, ties between equal blobs and between different blobs at the same distance.  Every
case compares every bit of n_out, status, corr, xyz and err (mocap_core.devcheck.compare_bitwise) and n_cand with the
exhaustive walk on a second context; the hand-built cases assert on the CPU, with the oracle's matching, that their frames are
at the edge they are named for.

Streams: seed 1, gate 5 px, G_cap 2^20 (the walk alone flags under 1 % of these streams' frames: asserted in _walk).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_bb_eval_path as ep
from mocap_core import capi, synth
from test_gpu_bb_eval_path import GATE, KERNELS, RIGS, ROOT, _env, _frames_with_n_prov, _search_equals, _to_dev, _walk, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

C, M = 8, 16
F_STREAM = 4096   # more than three buffer swaps per resident workgroup (256 CUs x 5 workgroups = 1 280 at the most)
LAYOUTS = [(K_max, f32) for K_max in (48, 64) for f32 in (True, False)]


@functools.lru_cache(maxsize=None)
def _rig(rig_name):
    return RIGS[rig_name](C)


@functools.lru_cache(maxsize=None)
def _stream(rig_name, F, markers, dropout=0.05):
    blobs, counts, _ = synth.make_blob_stream(_rig(rig_name), F, markers, seed=1, dropout=dropout, m_max=M)
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return blobs, counts


@functools.lru_cache(maxsize=None)
def _clean(rig_name, F=64):
    """Frames of two well separated markers, nothing dropped: every root has one hit per camera."""
    blobs, counts, _ = synth.make_blob_stream(_rig(rig_name), F, 2, seed=1, m_max=M, dropout=0.0, min_sep=0.6)
    blobs.setflags(write=False)
    counts.setflags(write=False)
    return blobs, counts


@functools.lru_cache(maxsize=None)
def _ftab(rig_name):
    from oracle import mocap_oracle as mo
    rig = _rig(rig_name)
    return mo.fundamental_table(rig["K"], rig["R"], rig["t"])


def _match(rig_name, blobs_f, counts_f):
    from oracle import mocap_oracle as mo
    return mo.match_frame(blobs_f.astype(np.float64), counts_f, _ftab(rig_name), gate_px=GATE)


def _check(gpu, rig_name, blobs, counts, layouts=LAYOUTS, min_points=None, make=None):
    """The search on every layout equal to the walk.  make: the search's contexts (default: the module's)."""
    dev, _ = gpu
    rig = _rig(rig_name)
    d_b, d_c = _to_dev(dev, blobs, counts)
    for K_max, f32 in layouts:
        ref = _walk(gpu, rig, C, M, K_max, d_b, d_c, min_points=blobs.shape[0] // 2 if min_points is None else min_points, f32=f32)
        _search_equals(gpu if make is None else (dev, make), rig, ref, M, d_b, d_c, KERNELS[rig_name] % 1, f32=f32)


# ------------------------------------------------------------------------------------------------ 1. the bench's stream

@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_bench_stream_equals_the_walk(gpu, rig_name, K_max, f32):
    blobs, counts = _stream(rig_name, F_STREAM, M)
    _check(gpu, rig_name, blobs, counts, layouts=[(K_max, f32)], min_points=F_STREAM)


# ------------------------------------------------------------------------------------------------ 2. hand-built hit lists

def _with_copies(rig_name, cams, offsets, root_cam=0, want=24):
    """Clean frames in which the first root created at camera `root_cam` (the cameras before it emptied) gets, in every camera
    of `cams`, copies of its closest blob moved by `offsets` [(dx, dy)]: 1 + len(offsets) hits there when they stay inside the
    gate (a frame where they do not is left out).  A camera without room for the copies keeps the closest blob alone.
    -> blobs, counts, the root's (camera, blob) per frame."""
    b0, c0 = _clean(rig_name)
    got_b, got_c, got_r = [], [], []
    for f in range(b0.shape[0]):
        bf, cf = b0[f].copy(), c0[f].copy()
        cf[:root_cam] = 0
        roots, hits = _match(rig_name, bf, cf)
        mine = [r for r, (rc, _) in enumerate(roots) if rc == root_cam]
        if not mine or any(len(hits[mine[0]][c]) != 1 for c in range(root_cam + 1, C)):
            continue
        r0, root = mine[0], roots[mine[0]]
        for c in cams:
            base = bf[c, hits[r0][c][0]].copy()
            if cf[c] + len(offsets) > M:
                bf[c, 0], cf[c] = base, 1
                bf[c, 1:] = np.nan
            for dx, dy in offsets:
                bf[c, cf[c]] = base + np.array([dx, dy], dtype=np.float32)
                cf[c] += 1
        roots, hits = _match(rig_name, bf, cf)
        if roots[r0] != root or any(len(hits[r0][c]) != 1 + len(offsets) for c in cams):   # (the copies only add roots behind it)
            continue
        if any(len(hits[r0][c]) != 1 for c in range(root_cam + 1, C) if c not in cams):
            continue
        got_b.append(bf)
        got_c.append(cf)
        got_r.append(roots[r0])
        if len(got_b) == want:
            break
    assert len(got_b) >= 4, (cams, offsets, root_cam, len(got_b))
    return np.stack(got_b), np.stack(got_c), got_r


def _steps(n, step=0.2):
    return [(np.float32(step * (j + 1)), np.float32(0.0)) for j in range(n)]


def _root_hits(rig_name, bf, cf, root):
    roots, hits = _match(rig_name, bf, cf)
    return hits[roots.index(root)]


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("k", [0, 1, 3, 7])
def test_roots_with_k_multi_hit_cameras(gpu, rig_name, k):
    """A camera-0 root with two hits in cameras 1 .. k and one in the others: k digits -- none, one, three, and seven: every
    byte of the act row and every count of the nh word is a digit's."""
    blobs, counts, roots = _with_copies(rig_name, list(range(1, k + 1)), _steps(1, 1.0))
    for f in range(blobs.shape[0]):
        hr = _root_hits(rig_name, blobs[f], counts[f], roots[f])
        assert [len(h) for h in hr] == [0] + [2] * k + [1] * (C - 1 - k), (f, hr)
    _check(gpu, rig_name, blobs, counts)


@pytest.mark.parametrize("rig_name", list(RIGS))
def test_a_camera_with_sixteen_hits(gpu, rig_name):
    """All sixteen blobs of camera 4 are hits of one root: the largest count a byte of the nh word and a digit hold."""
    blobs, counts, roots = _with_copies(rig_name, [4], _steps(15))
    for f in range(blobs.shape[0]):
        assert len(_root_hits(rig_name, blobs[f], counts[f], roots[f])[4]) == M, f
    _check(gpu, rig_name, blobs, counts)


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("n_hits", [1, 2, 3, 5])
@pytest.mark.parametrize("stage", [0, 1])
def test_hit_lists_of_every_length(gpu, rig_name, stage, n_hits):
    """A pair with exactly 1, 2, 3 and more than 3 hits: of a camera-0 root (stage 0) and of a root created at camera 1, i.e. a
    provisional root's pair (stage 1).  One hit claims itself, two need no second distance, three order two, five keep the
    selection loop busy."""
    blobs, counts, roots = _with_copies(rig_name, [stage + 1], _steps(n_hits - 1, 0.5), root_cam=stage)
    for f in range(blobs.shape[0]):
        assert roots[f][0] == stage
        assert len(_root_hits(rig_name, blobs[f], counts[f], roots[f])[stage + 1]) == n_hits, f
    _check(gpu, rig_name, blobs, counts)


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("stage", [0, 1])
def test_two_blobs_with_equal_coordinates(gpu, rig_name, stage):
    """The closest blob twice: equal distances (index order decides) and a claim by value that takes both."""
    blobs, counts, roots = _with_copies(rig_name, [stage + 1], [(np.float32(0.0), np.float32(0.0))], root_cam=stage)
    for f in range(blobs.shape[0]):
        h = _root_hits(rig_name, blobs[f], counts[f], roots[f])[stage + 1]
        assert len(h) == 2 and h[0] < h[1] and (blobs[f, stage + 1, h[0]] == blobs[f, stage + 1, h[1]]).all(), (f, h)
    _check(gpu, rig_name, blobs, counts)


def _equal_distance_frames(rig_name, dy, root_cam):
    """Clean frames plus, in camera root_cam + 1, two DIFFERENT blobs at the same distance from the first root's line: (1e-30, y)
    and (2e-30, y) with y where the line meets x = 0, moved by dy -- the products a x vanish in the sum (a x + b y) + c, so
    both distances have the same bits, with and without the float32 roundings, whatever the line."""
    from oracle import mocap_oracle as mo
    b0, c0 = _clean(rig_name)
    cam = root_cam + 1
    got_b, got_c, got_r = [], [], []
    for f in range(b0.shape[0]):
        bf, cf = b0[f].copy(), c0[f].copy()
        cf[:root_cam] = 0
        roots, hits = _match(rig_name, bf, cf)
        mine = [r for r, (rc, _) in enumerate(roots) if rc == root_cam]
        if not mine or len(hits[mine[0]][cam]) != 1:
            continue
        root = roots[mine[0]]
        a, b, c = mo.epiline(_ftab(rig_name)[root_cam, cam], bf[root_cam, root[1]])
        if abs(b) < 0.2:
            continue
        y = np.float32(-c / b + dy)
        bf[cam, cf[cam]] = (np.float32(1e-30), y)
        bf[cam, cf[cam] + 1] = (np.float32(2e-30), y)
        cf[cam] += 2
        px, py = bf[cam, :cf[cam], 0].astype(np.float64), bf[cam, :cf[cam], 1].astype(np.float64)
        d = np.abs(a * px + b * py + c) / np.sqrt(a ** 2 + b ** 2)
        roots2, hits2 = _match(rig_name, bf, cf)
        if root not in roots2 or d[-1] != d[-2] or not d[-1] < GATE:
            continue
        h = hits2[roots2.index(root)][cam]
        if len(h) != 3:
            continue
        # the pair next to each other in index order; first when dy = 0 (closer than the marker's own blob, which has noise)
        i = h.index(cf[cam] - 2)
        if h[i + 1:i + 2] != [cf[cam] - 1] or (dy == 0.0) != (i == 0):
            continue
        got_b.append(bf)
        got_c.append(cf)
        got_r.append(root)
    assert len(got_b) >= 4, (rig_name, dy, root_cam, len(got_b))
    return np.stack(got_b), np.stack(got_c), got_r


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("where", ["closest", "behind the closest"])
@pytest.mark.parametrize("stage", [0, 1])
def test_two_different_blobs_at_equal_distance(gpu, rig_name, stage, where):
    """Equal distance bits, different coordinates: the smaller index comes first, and as the closest hit it claims itself only
    (the other blob of the pair stays free to become a root).  Once as the list's minimum (the walk's strict <), once behind
    the closest hit (the selection loop's strict <)."""
    blobs, counts, _ = _equal_distance_frames(rig_name, 0.0 if where == "closest" else 3.0, stage)
    _check(gpu, rig_name, blobs, counts)


# ------------------------------------------------------------------------------------------------ 3. stale bytes below a root's camera

@pytest.mark.parametrize("K_max,f32", LAYOUTS)
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_roots_at_cameras_3_and_6_in_slots_camera_0_roots_filled(gpu, rig_name, K_max, f32):
    """Frames of twelve markers, every fourth with cameras 0 .. 2 emptied and every fourth with cameras 0 .. 5 emptied: a
    workgroup takes frames of all kinds in turn (4 096 frames, at most 1 280 resident workgroups), so the roots created at
    cameras 3 and 6 sit in slots whose nh and hits bytes of cameras 1 .. 3 and 1 .. 6 an earlier frame's camera-0 roots wrote."""
    b, c = (a.copy() for a in _stream(rig_name, F_STREAM, 12))
    idx = np.arange(F_STREAM)
    c[idx % 4 == 1, :3] = 0
    c[idx % 4 == 3, :6] = 0
    for f in range(8):
        roots, hits = _match(rig_name, b[f], c[f])
        if f % 2 == 0:   # camera-0 roots that leave counts in the bytes of cameras 1 .. 6
            assert sum(1 for (rc, _), hr in zip(roots, hits) if rc == 0 and all(hr[i] for i in range(1, 7))) >= 4, f
        else:
            first = 3 if f % 4 == 1 else 6
            assert roots and roots[0][0] == first and any(rc == first and any(hr) for (rc, _), hr in zip(roots, hits)), f
    _check(gpu, rig_name, b, c, layouts=[(K_max, f32)], min_points=F_STREAM // 2)


# ------------------------------------------------------------------------------------------------ 4. G_cap and the block sizes

@pytest.mark.parametrize("rig_name", list(RIGS))
def test_a_root_over_a_small_g_cap(gpu, rig_name, monkeypatch):
    """G_cap = 7 and roots with 2 x 2 x 2 candidates: the product passes the cap at camera 3 with four single-hit cameras behind
    it (the loop's running product starts again at 1 there and ends at 1), and at the root's last camera.  256 frames, two of
    them over the cap: the walk flags those two (under 1 %) and the search must flag the same."""
    early = _with_copies(rig_name, [1, 2, 3], _steps(1, 1.0), want=4)
    late = _with_copies(rig_name, [5, 6, 7], _steps(1, 1.0), want=4)
    def n_cand_max(bf, cf):
        return max(int(np.prod([max(1, len(h)) for h in hr])) for hr in _match(rig_name, bf, cf)[1])
    b0, c0 = _clean(rig_name, 512)
    under = [f for f in range(512) if n_cand_max(b0[f], c0[f]) <= 7][:256]   # (two markers on one epipolar plane: 2 x 2 x 2 x ... by themselves)
    assert len(under) == 256
    blobs, counts = b0[under].copy(), c0[under].copy()
    blobs[100], counts[100] = early[0][0], early[1][0]
    blobs[200], counts[200] = late[0][0], late[1][0]
    for f, (_, _, roots), cams in ((100, early, (1, 2, 3)), (200, late, (5, 6, 7))):
        hr = _root_hits(rig_name, blobs[f], counts[f], roots[0])
        assert [c for c in range(C) if len(hr[c]) == 2] == list(cams) and all(len(hr[c]) == 1 for c in range(1, C) if c not in cams), (f, hr)
    assert n_cand_max(blobs[100], counts[100]) == 8 and n_cand_max(blobs[200], counts[200]) == 8
    monkeypatch.setattr(ep, "G_CAP", 7)
    _check(gpu, rig_name, blobs, counts, min_points=200)


@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("nb_max", [1, 8])
@pytest.mark.parametrize("pl_min", [2, 16])
def test_block_size_rules_on_the_bench_stream(gpu, rig_name, pl_min, nb_max):
    """MOCAP_BB_PL_MIN x MOCAP_BB_NB_MAX as tests/test_gpu_bb_block_size.py sweeps them (read when a context is created): the
    sizing code takes its counts from the digits' word."""
    import torch
    dev, shared = gpu
    cores = {}

    def make(walk=False, f32=True):
        if walk:
            return shared(walk=True, f32=f32)
        if f32 not in cores:
            with _env({"MOCAP_BB_PL_MIN": str(pl_min), "MOCAP_BB_NB_MAX": str(nb_max)}):
                cores[f32] = capi.MocapCore(0)
            cores[f32].set_stream(torch.cuda.current_stream(dev).cuda_stream)
            cores[f32].set_options(f32_rounding=f32, exhaustive_walk=False)
        return cores[f32]
    blobs, counts = _stream(rig_name, F_STREAM, M)
    try:
        _check(gpu, rig_name, blobs, counts, layouts=[(48, True), (64, False)], min_points=F_STREAM, make=make)
    finally:
        torch.cuda.synchronize(dev)
        for c in cores.values():
            c.close()


# ------------------------------------------------------------------------------------------------ 5. the old chain

@pytest.mark.parametrize("rig_name", list(RIGS))
def test_a_frame_that_falls_back_to_the_old_chain(gpu, rig_name):
    """65 provisional roots: more than a wave, the frame takes the chain over the cameras (match_pairs), whose rows phase C and the
    search read as words all the same."""
    blobs, counts = _frames_with_n_prov(_rig(rig_name), C, M, 65)
    _check(gpu, rig_name, blobs, counts, min_points=blobs.shape[0])


# ------------------------------------------------------------------------------------------------ 6. the measuring and self-check builds

_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(root)r, %(pkg)r]
import torch
from mocap_core import capi, synth
core = capi.MocapCore(0)
dev = torch.device("cuda:0")
rig = synth.ring_rig(8)
F, C, M, K, EXTRA = %(frames)d, 8, 16, 48, 11
blobs, counts, _ = synth.make_blob_stream(rig, F, M, seed=1)
core.set_cameras(rig["K"], rig["R"], rig["t"])
d_b, d_c = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
xyz = torch.full((F, K, 3), float("nan"), dtype=torch.float64, device=dev); err = torch.full((F, K), float("nan"), dtype=torch.float64, device=dev)
corr = torch.full((F, K, C), -2, dtype=torch.int16, device=dev); n_out = torch.zeros(F, dtype=torch.int32, device=dev)
status = torch.zeros(F + EXTRA, dtype=torch.int32, device=dev)          # + the builds' counters (unused by the product library)
n_cand = torch.zeros(F, dtype=torch.int32, device=dev)
core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, xyz.data_ptr(), err.data_ptr(),
                           corr.data_ptr(), n_out.data_ptr(), status.data_ptr(), n_cand.data_ptr())
core.synchronize()
assert core.last_frame_kernel().startswith("frame_bb_kernel")
np.savez(%(out)r, xyz=xyz.cpu().numpy().view(np.uint64), err=err.cpu().numpy().view(np.uint64), corr=corr.cpu().numpy(),
         n_out=n_out.cpu().numpy(), status=status.cpu().numpy(), n_cand=n_cand.cpu().numpy())
"""


def test_phase_clock_and_self_check_builds_equal_the_product_library(tmp_path):
    """lib/libmocap_core_phaseclocks.so and lib/libmocap_core_eigcheck.so against the product library on 4 096 frames of the
    bench's stream, each in a process of its own into buffers filled alike: every byte of xyz, err, corr, n_out, n_cand and of
    the frames' status is the same; both builds' counters behind the status array counted, and the self-check printed nothing."""
    libdir = os.path.join(ROOT, "low-cost-mocap_amd", "lib")
    got = {}
    for name in ("libmocap_core.so", "libmocap_core_phaseclocks.so", "libmocap_core_eigcheck.so"):
        lib = os.path.join(libdir, name)
        assert os.path.exists(lib), "build it with `make -C low-cost-mocap_amd all` (__graft_entry__.build does)"
        out = str(tmp_path / (name + ".npz"))
        code = _CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "low-cost-mocap_amd"), "frames": F_STREAM, "out": out}
        env = dict(os.environ, MOCAP_CORE_LIB=lib)
        for k in ("MOCAP_BB_PL", "MOCAP_BB_PL_MIN", "MOCAP_BB_NB_MAX", "MOCAP_BB_FIXED_LAYOUT"):
            env.pop(k, None)
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        assert "EIGCHECK" not in p.stdout, p.stdout[:2000]
        got[name] = dict(np.load(out))
    prod = got["libmocap_core.so"]
    assert int(prod["n_out"].sum()) >= F_STREAM and (prod["status"][F_STREAM:] == 0).all()
    for name, counters in (("libmocap_core_phaseclocks.so", 11), ("libmocap_core_eigcheck.so", 2)):
        other = got[name]
        for field in ("xyz", "err", "corr", "n_out", "n_cand"):
            assert np.array_equal(prod[field], other[field]), (name, field)
        assert np.array_equal(prod["status"][:F_STREAM], other["status"][:F_STREAM]), name
        assert (other["status"][F_STREAM:F_STREAM + counters] > 0).all(), (name, other["status"][F_STREAM:])
