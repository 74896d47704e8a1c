"""GPU: the search kernels' blocks (csrc/frame_bb.hip) -- a size per root, bounds from the root's base, a one-float cache.

Round 10 changed three things about the blocks of the branch and bound, none of which may show in a result:
  * the size can be the root's own (phase C): digits open while a block holds fewer than bb_pl_min candidates, and further, up
    to bb_pl = 16, while more than bb_nb_max blocks would be left (MOCAP_BB_PL_MIN / MOCAP_BB_NB_MAX; MOCAP_BB_PL = one size for
    every root, as before).  The shipped default is 16 / 1 -- one size, as before: every finer setting measured slower
    (profiles/r10_block_size_ab.txt) --, so the cases below run the swept settings next to it;
  * a block's blob bytes and DLT matrix start from what the root's blocks share (pkbase, block_pk / block_matrix) instead of
    a walk over all cameras;
  * the seed pass leaves ONE float per block for the test pass (csrc/bb_fold.hpp), and a surviving block rebuilds its bytes.

Every GPU case compares every bit of n_out, status, corr, xyz and err (mocap_core.devcheck.compare_bitwise) with the
exhaustive walk on a second context (set_options(exhaustive_walk=True)).  The hand-built cases assert, with the oracle's
matching on the CPU (oracle.mocap_oracle.match_frame) and a restatement of the kernel's partition rule, that their frames
really are at the edge they are named for.  The folded cache word is checked on the CPU by a stand-alone program
(tests/native/bb_fold_check.cpp) -- the only case here that needs no GPU.

Streams: seed 1, gate 5 px, G_cap 2^20.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from mocap_core import capi, devcheck, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE, G_CAP = 5.0, 1 << 20
PL_CAP = 16
SWEPT = [(pl_min, nb_max) for pl_min in (2, 4, 8) for nb_max in (8, 16, 32, 64)]


def _defaults():
    """(bb_pl_min, bb_nb_max) the library ships with (csrc/ctx.hpp)."""
    src = open(os.path.join(ROOT, "low-cost-mocap_amd", "csrc", "ctx.hpp")).read()
    return tuple(int(re.search(r"int %s = (\d+);" % n, src).group(1)) for n in ("bb_pl_min", "bb_nb_max"))


# ------------------------------------------------------------------------------------------------ the rule, restated

def partition(digits, pl_min, nb_max, cap=PL_CAP):
    """Hit counts of a root's multi-hit cameras (ascending camera) -> (candidates per block, blocks): phase C's rule."""
    nb = 1
    for n in digits:
        nb *= n
    pl, nl = 1, 0
    while nl < len(digits) and (pl < pl_min or (pl < cap and nb > nb_max)):
        pl *= digits[nl]
        nb //= digits[nl]
        nl += 1
    return pl, nb


def frame_structure(rig, blobs_f, counts_f, pl_min, nb_max, cap=PL_CAP):
    """Per root with candidates: dict(rc, counts per later camera, candidates, pl, nb) -- the oracle's matching + the rule."""
    from oracle import mocap_oracle as mo
    C = len(rig["R"])
    Ftab = mo.fundamental_table(rig["K"], rig["R"], rig["t"])
    roots, hits = mo.match_frame(blobs_f.astype(np.float64), counts_f, Ftab, gate_px=GATE)
    out = []
    for r, (rc, _) in enumerate(roots):
        n = [len(hits[r][c]) if c > rc else 0 for c in range(C)]
        if sum(1 for x in n if x) < 1:
            continue          # one view: no candidates (helpers.py:413-414)
        total = int(np.prod([x for x in n if x], dtype=np.int64))
        pl, nb = partition([x for x in n if x > 1], pl_min, nb_max, cap)
        out.append({"rc": rc, "n": n, "candidates": total, "pl": pl, "nb": nb})
    return out


def test_partition_rule_restated():
    """The restated rule on hand-counted roots (no GPU)."""
    assert partition([], 4, 32) == (1, 1)                          # one candidate
    assert partition([2, 2], 4, 32) == (4, 1)                      # opens to pl_min
    assert partition([2, 3, 2], 4, 32) == (6, 2)                   # 12 candidates: stops at >= 4 with 2 blocks left
    assert partition([3, 3, 3, 3, 3, 3, 3], 4, 32) == (27, 81)     # 2 187 candidates: coarse blocks, still more than nb_max
    assert partition([2, 2, 2, 2, 2, 2, 2], 4, 32) == (4, 32)      # 128 candidates: 32 blocks of 4
    assert partition([2, 2, 2, 2, 2, 2, 2], 16, 1) == (16, 8)      # MOCAP_BB_PL = 16: pl_min = cap
    assert partition([5, 7], 2, 8) == (5, 7)


# ------------------------------------------------------------------------------------------------ the folded cache word

def test_folded_cache_word_never_drops_what_the_double_test_keeps(tmp_path):
    """csrc/bb_fold.hpp on the CPU: s1, tr and y drawn from the ranges the bench frames produce (s1 1e-8 .. 1e2, tr 1e4 .. 1e9,
    y 1e-6 .. 1e6) and far around them, plus the extremes -- s1 2e-12 tr near and above 1, s1 above the float range and in the
    float denormals, y = +inf, 0.  Wherever the float word says "dropped", the double expression s1 fma(2e-12, tr, y) < 1 says
    so too: zero exceptions (the program counts them and prints how many draws were dropped at all)."""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "bb_fold_check")
    src = os.path.join(ROOT, "tests", "native", "bb_fold_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "low-cost-mocap_amd", "csrc"), src, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(r"draws (\d+) dropped_by_word (\d+) dropped_by_double (\d+) violations (\d+)", res.stdout)
    assert m, res.stdout
    draws, by_word, by_double, violations = map(int, m.groups())
    assert violations == 0 and draws >= 4_000_000 and by_word * 5 >= draws
    # ... and the word still drops: on the plain draws from the bench's ranges, all but a 2^-20 sliver of what the double test drops
    b_draws, b_word, b_double = map(int, re.search(r"bench_draws (\d+) dropped_by_word (\d+) dropped_by_double (\d+)", res.stdout).groups())
    assert b_draws >= 1_000_000 and b_double * 3 >= b_draws and b_word * 10_000 >= 9_999 * b_double, (b_draws, b_word, b_double)


# ------------------------------------------------------------------------------------------------ GPU plumbing

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

    def make(env=None, walk=False):
        """One context per (environment at creation, walk) -- the block rule is read when the context is created."""
        key = (tuple(sorted((env or {}).items())), walk)
        if key not in cores:
            with _env(env):
                c = capi.MocapCore(0)
            c.set_stream(stream.cuda_stream)
            if walk:
                c.set_options(exhaustive_walk=True)
            cores[key] = c
        return cores[key]
    yield dev, make
    torch.cuda.synchronize(dev)
    for c in cores.values():
        c.close()


def _to_dev(dev, blobs, counts):
    import torch
    return torch.from_numpy(np.array(blobs)).to(dev), torch.from_numpy(np.array(counts)).to(dev)


def _walk(gpu, rig, C, M, K_max, d_blobs, d_counts, min_points=None, g_cap=G_CAP):
    import torch
    dev, make = gpu
    walk = make(walk=True)
    walk.set_cameras(rig["K"], rig["R"], rig["t"])
    ref = devcheck.FrameOutputs(d_blobs.shape[0], K_max, C, dev)
    ref.run(walk, M, d_blobs, d_counts, GATE, g_cap)
    torch.cuda.synchronize(dev)
    assert walk.last_frame_kernel().startswith("frame_kernel<"), walk.last_frame_kernel()
    F = ref.F
    assert int((ref.status != 0).sum().item()) * 100 <= F, "more than 1 % of the walk's frames flagged"
    assert int(ref.n_out.sum().item()) >= (F if min_points is None else min_points)
    return ref


def _search_equals(gpu, rig, ref, M, d_blobs, d_counts, env=None, run_env=None, kernel="frame_bb_kernel", runs=1, g_cap=G_CAP):
    import torch
    dev, make = gpu
    core = make(env=env)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    first = None
    with _env(run_env):
        for rep in range(runs):
            out = devcheck.FrameOutputs(ref.F, ref.K, ref.C, dev)
            out.run(core, M, d_blobs, d_counts, GATE, g_cap)
            torch.cuda.synchronize(dev)
            assert core.last_frame_kernel().startswith(kernel), core.last_frame_kernel()
            cmp = devcheck.compare_bitwise(out, ref)
            assert cmp["frames_differing"] == 0, (env, run_env, rep, cmp)
            assert torch.equal(out.n_cand, ref.n_cand), (env, rep)
            if first is None:
                first = out
    return first


RIGS = {"identical K": lambda C: synth.ring_rig(C), "per-camera K": lambda C: synth.calibrated_ring_rig(C, 1)}
KERNELS = {"identical K": "frame_bb_kernel<CW=%d>", "per-camera K": "frame_bb_kernel<CW=%d, per-camera K>"}


@pytest.fixture(scope="module")
def bench_refs(gpu):
    """2 000 frames of the bench stream on either rig, on the device, with the walk's result per K_max: computed once, never written."""
    dev, _ = gpu
    cache = {}

    def get(rig_name, K_max):
        if rig_name not in cache:
            rig = RIGS[rig_name](8)
            blobs, counts, _ = synth.make_blob_stream(rig, 2000, 16, seed=1)
            cache[rig_name] = (rig,) + _to_dev(dev, blobs, counts)
        if (rig_name, K_max) not in cache:
            rig, d_b, d_c = cache[rig_name]
            cache[rig_name, K_max] = _walk(gpu, rig, 8, 16, K_max, d_b, d_c)
        return cache[rig_name] + (cache[rig_name, K_max],)
    return get


# ------------------------------------------------------------------------------------------------ 1. the default rule

@pytest.mark.gpu
@pytest.mark.parametrize("run_env", [None, {"MOCAP_BB_FIXED_LAYOUT": "0"}], ids=["fixed layout", "runtime layout"])
@pytest.mark.parametrize("K_max", [48, 64])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_default_rule_on_the_bench_stream(gpu, bench_refs, rig_name, K_max, run_env):
    rig, d_b, d_c, ref = bench_refs(rig_name, K_max)
    _search_equals(gpu, rig, ref, 16, d_b, d_c, run_env=run_env, kernel=KERNELS[rig_name] % 1)


@pytest.mark.gpu
@pytest.mark.parametrize("C,M,K_max,cw", [(4, 4, 16, 1), (6, 8, 48, 1), (9, 8, 64, 2)])
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_default_rule_on_other_shapes(gpu, rig_name, C, M, K_max, cw):
    """500 frames each; 9 cameras take two packed words.  (4 x 4 would go to the one-wave kernel of tiny frames: its blob arrays
    are padded to 12 slots per camera with the counts left as they are, which changes no result.)"""
    dev, _ = gpu
    rig = RIGS[rig_name](C)
    blobs, counts, _ = synth.make_blob_stream(rig, 500, M, seed=1)
    Mw = M
    if C * M <= 32:
        Mw = 12
        wide = np.zeros((500, C, Mw, 2), dtype=blobs.dtype)
        wide[:, :, :M] = blobs
        blobs = wide
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, C, Mw, K_max, d_b, d_c, min_points=250)
    _search_equals(gpu, rig, ref, Mw, d_b, d_c, kernel=KERNELS[rig_name] % cw)


# ------------------------------------------------------------------------------------------------ 2. hand-built frames

def _cluster_world(n_cluster, scale):
    """The first n_cluster markers of every frame pulled together around their centroid (a few pixels apart in every camera)."""
    def edit(s):
        s = s.copy()
        c = s[:, :n_cluster].mean(axis=1, keepdims=True)
        s[:, :n_cluster] = c + (s[:, :n_cluster] - c) * scale
        return s
    return edit


MODELLED_RULE = (4, 32)     # the per-root rule the round-10 model proposed; the shipped default is _defaults()


def _hand_built(name, rig, rule=None):
    """-> blobs, counts (8 cameras x 16 slots), what a frame's structure must show under `rule` = (pl_min, nb_max) (default:
    the shipped one): a predicate on frame_structure's rows"""
    pl_min, nb_max = rule or _defaults()
    mk = lambda F, M, **kw: synth.make_blob_stream(rig, F, M, seed=1, m_max=16, **kw)[:2]   # noqa: E731
    if name == "one hit in every camera":
        blobs, counts = mk(96, 2, dropout=0.0, min_sep=0.6)
        return blobs, counts, lambda rows: any(r["rc"] == 0 and r["n"][1:] == [1] * 7 for r in rows)
    if name == "root created at the last-but-one camera":
        blobs, counts = mk(96, 12)
        counts[:, :6] = 0
        return blobs, counts, lambda rows: bool(rows) and all(r["rc"] == 6 for r in rows) and any(r["n"][7] > 1 for r in rows)
    if name == "no hit between cameras with several":
        blobs, counts = mk(128, 16)
        counts[:, 3] = 0
        counts[1::2, 5] = 0
        counts[2::3, 0] = 0      # ... and roots created at camera 1
        return blobs, counts, lambda rows: any(r["n"][2] > 1 and r["n"][3] == 0 and r["n"][4] > 1 for r in rows)
    if name == "coincident and near-coincident blobs":
        blobs, counts = mk(128, 12)
        for cam in (2, 6, 7):
            ok = counts[:, cam] >= 4
            blobs[ok, cam, 2] = blobs[ok, cam, 0]                        # the same pixel: tied errors, tied bounds
            blobs[ok, cam, 3] = blobs[ok, cam, 0] + np.float32(2.0 ** -12)  # ... and one a hair away
        return blobs, counts, lambda rows: any(r["nb"] > 1 for r in rows)
    if name == "more than nb_max blocks at sixteen candidates":
        blobs, counts = mk(64, 12, world=_cluster_world(3, 0.02), min_sep=0.05)
        return blobs, counts, lambda rows: any(r["pl"] >= PL_CAP and r["nb"] > nb_max for r in rows)
    if name == "more blocks than lanes":
        blobs, counts = mk(64, 12, world=_cluster_world(3, 0.02), min_sep=0.05)
        return blobs, counts, lambda rows: sum(r["nb"] for r in rows) > 256
    if name == "more blocks than any cache":
        blobs, counts = mk(48, 10, world=_cluster_world(4, 0.02), min_sep=0.05)
        return blobs, counts, lambda rows: sum(r["nb"] for r in rows) > 1024     # (the cache's cap, BBLayout)
    assert name == "at most pl_min candidates per root"
    blobs, counts = mk(128, 3, min_sep=0.5)
    return blobs, counts, lambda rows: bool(rows) and all(r["candidates"] <= pl_min for r in rows) and any(r["candidates"] > 1 for r in rows)


HAND_BUILT = ["one hit in every camera", "root created at the last-but-one camera", "no hit between cameras with several",
              "coincident and near-coincident blobs", "more than nb_max blocks at sixteen candidates", "more blocks than lanes",
              "more blocks than any cache", "at most pl_min candidates per root"]


def _assert_at_the_edge(name, rig, blobs, counts, want, rule, look_at=24):
    pl_min, nb_max = rule
    hit = [f for f in range(min(look_at, blobs.shape[0])) if want(frame_structure(rig, blobs[f], counts[f], pl_min, nb_max))]
    assert hit, name + ": none of the first frames has the structure the case is named for"


@pytest.mark.gpu
@pytest.mark.parametrize("rig_name", list(RIGS))
@pytest.mark.parametrize("name", HAND_BUILT)
def test_hand_built_frames(gpu, name, rig_name):
    dev, _ = gpu
    rig = RIGS[rig_name](8)
    """Each case under the shipped rule and under the modelled per-root rule (where "nb_max" and "pl_min" bite: 32 and 4), in the
    fixed and the runtime layout; the frames are at the named edge under either rule (asserted on the CPU)."""
    blobs, counts, want = _hand_built(name, rig)
    _assert_at_the_edge(name, rig, blobs, counts, want, _defaults())
    _assert_at_the_edge(name, rig, blobs, counts, _hand_built(name, rig, MODELLED_RULE)[2], MODELLED_RULE)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, 8, 16, 48, d_b, d_c, min_points=blobs.shape[0] // 2)
    per_root = {"MOCAP_BB_PL_MIN": str(MODELLED_RULE[0]), "MOCAP_BB_NB_MAX": str(MODELLED_RULE[1])}
    for env in (None, per_root):
        _search_equals(gpu, rig, ref, 16, d_b, d_c, env=env, kernel=KERNELS[rig_name] % 1)
        _search_equals(gpu, rig, ref, 16, d_b, d_c, env=env, run_env={"MOCAP_BB_FIXED_LAYOUT": "0"}, kernel=KERNELS[rig_name] % 1)


# ------------------------------------------------------------------------------------------------ 3. the partition never shows

PARTITIONS = [None, {"MOCAP_BB_PL": "2"}, {"MOCAP_BB_PL": "16"}] + [{"MOCAP_BB_PL_MIN": str(a), "MOCAP_BB_NB_MAX": str(b)} for a, b in SWEPT]


@pytest.mark.gpu
@pytest.mark.parametrize("rig_name", list(RIGS))
def test_every_partition_gives_the_same_bits(gpu, bench_refs, rig_name):
    """The rule unset, MOCAP_BB_PL = 2 and 16, every swept (pl_min, nb_max): each equal to the walk, hence to each other."""
    import torch
    rig, d_b, d_c, ref = bench_refs(rig_name, 48)
    first = None
    for env in PARTITIONS:
        out = _search_equals(gpu, rig, ref, 16, d_b, d_c, env=env, kernel=KERNELS[rig_name] % 1)
        if first is None:
            first = out
        else:
            assert devcheck.compare_bitwise(out, first)["frames_differing"] == 0, env
            assert torch.equal(out.n_cand, first.n_cand), env


# ------------------------------------------------------------------------------------------------ 4. determinism

@pytest.mark.gpu
def test_thirty_passes_of_twenty_thousand_frames(gpu):
    """The default rule, 30 repetitions of 20 000 bench frames: each equal to the first (and the first to the walk)."""
    import torch
    dev, make = gpu
    rig = synth.ring_rig(8)
    blobs, counts, _ = synth.make_blob_stream(rig, 20_000, 16, seed=1)
    d_b, d_c = _to_dev(dev, blobs, counts)
    ref = _walk(gpu, rig, 8, 16, 48, d_b, d_c)
    core = make()
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    outs = [devcheck.FrameOutputs(20_000, 48, 8, dev) for _ in range(2)]
    outs[0].run(core, 16, d_b, d_c, GATE, G_CAP)
    torch.cuda.synchronize(dev)
    assert devcheck.compare_bitwise(outs[0], ref)["frames_differing"] == 0
    for rep in range(1, 30):
        outs[1].zero_().run(core, 16, d_b, d_c, GATE, G_CAP)
        torch.cuda.synchronize(dev)
        cmp = devcheck.compare_bitwise(outs[1], outs[0])
        assert cmp["frames_differing"] == 0 and torch.equal(outs[1].n_cand, outs[0].n_cand), (rep, cmp)


# ------------------------------------------------------------------------------------------------ 5. the self-check build

_EIGCHECK_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%(root)r, %(pkg)r, %(tests)r]
import torch
from mocap_core import capi, synth
import test_gpu_bb_block_size as t
core = capi.MocapCore(0)
dev = torch.device("cuda:0")
tot = [0, 0]
batches = []
for rig_name in t.RIGS:
    rig = t.RIGS[rig_name](8)
    b, c, _ = synth.make_blob_stream(rig, 300, 16, seed=1)
    batches.append((rig, b, c))
    for name in t.HAND_BUILT:
        b, c, _ = t._hand_built(name, rig)
        batches.append((rig, b[:32], c[:32]))
for rig, blobs, counts in batches:
    F, C, M = blobs.shape[:3]
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    K = 48
    d_b, d_c = torch.from_numpy(np.array(blobs)).to(dev), torch.from_numpy(np.array(counts)).to(dev)
    xyz = torch.empty((F, K, 3), dtype=torch.float64, device=dev); err = torch.empty((F, K), dtype=torch.float64, device=dev)
    corr = torch.empty((F, K, C), dtype=torch.int16, device=dev); n_out = torch.zeros(F, dtype=torch.int32, device=dev)
    status = torch.zeros(F + 2, dtype=torch.int32, device=dev)          # + the self-check build's two counters
    core.match_triangulate_dev(F, M, d_b.data_ptr(), d_c.data_ptr(), 5.0, K, 1 << 20, xyz.data_ptr(), err.data_ptr(),
                               corr.data_ptr(), n_out.data_ptr(), status.data_ptr())
    core.synchronize()
    assert core.last_frame_kernel().startswith("frame_bb_kernel")
    s = status.cpu().numpy()
    tot[0] += int(s[F]); tot[1] += int(s[F + 1])
print("CHECKED", tot[0], tot[1])
"""


@pytest.mark.gpu
def test_self_check_build_with_the_default_rule():
    """lib/libmocap_core_eigcheck.so with the default rule on 300 bench frames and the hand-built frames of either rig: every
    candidate of every dropped block is evaluated in full on the device against the bound the block was dropped on -- no EIGCHECK
    line, and the counters show that cut candidates and dropped blocks' candidates were in fact re-evaluated."""
    lib = os.path.join(ROOT, "low-cost-mocap_amd", "lib", "libmocap_core_eigcheck.so")
    assert os.path.exists(lib), "build it with `make -C low-cost-mocap_amd all` (__graft_entry__.build does)"
    code = _EIGCHECK_CHILD % {"root": ROOT, "pkg": os.path.join(ROOT, "low-cost-mocap_amd"), "tests": os.path.join(ROOT, "tests")}
    env = dict(os.environ, MOCAP_CORE_LIB=lib)
    for k in ("MOCAP_BB_PL", "MOCAP_BB_PL_MIN", "MOCAP_BB_NB_MAX"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "EIGCHECK" not in p.stdout, p.stdout[:2000]
    checked = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKED")][-1].split()
    assert int(checked[1]) > 1000 and int(checked[2]) > 100000, checked   # cut candidates, candidates of dropped blocks
