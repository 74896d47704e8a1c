"""The "point consolidation" contract of include/mocap_core.h in plain Python / NumPy: the sorted walk (the definition), the
priority rounds the device runs (so that the two can be compared), the in-place compaction, and the helpers the CPU and GPU tests
share (random rows with chains, the figures of merit on a synthetic stream).  No floating-point arithmetic decides anything: the
key is (-views, the error's 64 bits as an unsigned integer, index)."""
import numpy as np

ST_SKIP = 1 | 2 | 4          # MOCAP_ST_ROOT_OVERFLOW | MOCAP_ST_CAND_OVERFLOW | MOCAP_ST_HIT_OVERFLOW
MAX_POINTS = 256
NEAR = 0.02                  # a point is "at" a true marker when its nearest true marker is less than 2 cm away


def keys(err, corr):
    """key(k) of every point as a tuple of Python ints: (-views, bits(err) as u64, k)."""
    corr = np.asarray(corr)
    bits = np.ascontiguousarray(err, dtype=np.float64).view(np.uint64)
    return [(-int((corr[k] >= 0).sum()), int(bits[k]), k) for k in range(corr.shape[0])]


def select_sorted(err, corr):
    """The definition: the points in ascending key; a point is kept iff it conflicts with no point kept before it, i.e. iff none
    of its blobs belongs to a kept point.  Returns the kept indices in ascending index."""
    corr = np.asarray(corr)
    kept, taken = [], set()
    for _, _, k in sorted(keys(err, corr)):
        mine = {(c, int(b)) for c, b in enumerate(corr[k]) if b >= 0}
        if not (mine & taken):
            kept.append(k)
            taken |= mine
    return sorted(kept)


def select_rounds(err, corr, want_rounds=False):
    """The device's form: ranks, an owner table per (camera, blob), rounds until no point is undecided."""
    corr = np.asarray(corr)
    n, C = corr.shape
    rank = [0] * n                                 # the number of keys below the point's own
    for r, (_, _, k) in enumerate(sorted(keys(err, corr))):
        rank[k] = r
    mine = [[(c, int(b)) for c, b in enumerate(corr[k]) if b >= 0] for k in range(n)]
    state = [0] * n                                # 0 undecided, 1 kept, 2 dropped
    rounds = 0
    while any(s == 0 for s in state):
        rounds += 1
        owner = {}
        for k in range(n):
            if state[k] == 0:
                for e in mine[k]:
                    owner[e] = min(owner.get(e, n), rank[k])
        kept_rank = set()
        for k in range(n):
            if state[k] == 0 and all(owner[e] == rank[k] for e in mine[k]):
                state[k] = 1
                kept_rank.add(rank[k])
        for k in range(n):
            if state[k] == 0 and any(owner[e] in kept_rank for e in mine[k]):
                state[k] = 2
    kept = [k for k in range(n) if state[k] == 1]
    return (kept, rounds) if want_rounds else kept


def longest_chain(err, corr):
    """Rounds the frame needs = the longest chain of decisions."""
    return select_rounds(err, corr, want_rounds=True)[1]


def processed(n, status, corr_f, K_max):
    if status & ST_SKIP or n < 0 or n > K_max:
        return False
    rows = corr_f[:n]
    return not ((rows < -1) | (rows > 255)).any()


def consolidate(xyz, err, corr, n_pts, status=None, select=select_sorted):
    """The staged call on copies of the arrays: {"xyz", "err", "corr", "n_pts", "src" (-1 where not written), "n_in"}."""
    xyz = np.array(xyz, dtype=np.float64)
    err = np.array(err, dtype=np.float64)
    corr = np.array(corr, dtype=np.int16)
    n_pts = np.array(n_pts, dtype=np.int32)
    F, K_max = err.shape
    status = np.zeros(F, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
    src = np.full((F, K_max), -1, dtype=np.int32)
    n_in = np.full(F, -1, dtype=np.int32)
    for f in range(F):
        n = int(n_pts[f])
        if not processed(n, int(status[f]), corr[f], K_max):
            continue
        kept = select(err[f, :n], corr[f, :n])
        m = len(kept)
        xyz[f, :m] = xyz[f, kept]           # (fancy indexing copies first: the rows move as if all reads came before the stores)
        err[f, :m] = err[f, kept]
        corr[f, :m] = corr[f, kept]
        src[f, :m] = kept
        n_in[f] = n
        n_pts[f] = m
    return {"xyz": xyz, "err": err, "corr": corr, "n_pts": n_pts, "src": src, "n_in": n_in}


def shares_a_blob(corr_rows):
    """True when two of the rows conflict."""
    rows = np.asarray(corr_rows)
    for c in range(rows.shape[1]):
        col = rows[:, c]
        col = col[col >= 0]
        if len(np.unique(col)) != len(col):
            return True
    return False


def random_rows(rng, F, C, K_max, blob_range, n_pts=None, p_none=0.3, err_levels=0, chain=0):
    """Random frames in the frame path's layout.  Blob indices are drawn from 0 .. blob_range) so that points collide; with
    err_levels > 0 the errors come from that many values (ties in the error bits).  chain > 0 (C >= 2): that many points of every
    frame, at random slots, form a chain -- two views each, consecutive links share one blob (of the range's upper end), the
    errors ascend along it -- which alone takes chain / 2 rounds.  Slots from n_pts on hold a sentinel."""
    n = rng.integers(0, K_max + 1, F).astype(np.int32) if n_pts is None else np.asarray(n_pts, dtype=np.int32)
    corr = rng.integers(0, blob_range, (F, K_max, C)).astype(np.int16)
    corr[rng.random((F, K_max, C)) < p_none] = -1
    err = rng.random((F, K_max)) if not err_levels else rng.integers(0, err_levels, (F, K_max)) / 8.0
    xyz = rng.normal(0, 1, (F, K_max, 3))
    for f in range(F if chain else 0):
        L = min(chain, int(n[f]))
        for i, k in enumerate(rng.permutation(int(n[f]))[:L]):
            corr[f, k] = -1
            corr[f, k, 0], corr[f, k, 1] = 255 - (i + 1) // 2, 255 - i // 2
            err[f, k] = (i + 1) / 1024.0
    beyond = np.arange(K_max)[None, :] >= n[:, None]
    corr[beyond] = -7
    err[beyond] = 1e6
    xyz[beyond] = 1e6
    return xyz, err, corr, n


# ---------------------------------------------------------------- the figures of merit on a synthetic stream
def drift_stream(n_frames=150, drift=True, seed=1):
    """The 8 x 16 stream as bench.py makes it (integer pixels, 0.3 px noise, 5 % dropout), sixteen markers at least 15 cm apart on
    a slow Lissajous path (drift=False: standing still): rig, blobs, counts, stamps, true markers [F][16][3] (camera-0
    coordinates, the frame path's without a world transform)."""
    from mocap_core import synth
    rig = synth.ring_rig(8)
    amp = 0.05 if drift else 0.0
    path = lambda s: s[:1] + amp * np.sin(np.arange(len(s))[:, None, None] / 60.0 * np.array([2.0, 3.0, 4.0]))   # noqa: E731
    blobs, counts, truth = synth.make_blob_stream(rig, n_frames, 16, seed=seed, min_sep=0.15, world=path, noise_px=0.3, dropout=0.05,
                                                  truncate=True)
    return rig, blobs, counts, 50.0 + np.arange(n_frames) / 60.0, truth["points_cam0"]


def points_per_marker(points, markers):
    """How many of a frame's points sit at each true marker (nearest marker, less than NEAR away), and how many at none."""
    at = np.zeros(len(markers), dtype=int)
    far = 0
    for p in np.asarray(points).reshape(-1, 3):
        d = np.sqrt(((markers - p) ** 2).sum(axis=1))
        j = int(np.argmin(d))
        if d[j] < NEAR:
            at[j] += 1
        else:
            far += 1
    return at, far
