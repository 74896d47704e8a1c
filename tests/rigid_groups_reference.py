"""The "rigid groups" contract of include/mocap_core.h in plain Python and NumPy, in the order the header writes.

    tree_sum_scalar(values)                  THE reduction tree over frames, in Python floats with the tree written as loops
    tree_sum(V)                              the same over the last axis of an array (reshape and add halves)
    rigid_groups_scalar(traj, ...)           THE statement: every pair, every sum, union-find, all in Python floats
    rigid_groups(traj, ...)                  the same, the pair statistics vectorised over pairs and tiles; asserted equal to the scalar
                                             form bit for bit in tests/test_rigid_groups_reference_cpu.py; the device is compared with
                                             this one
    pair_stats_mp(traj)                      dist and spread of every pair with 50 digits (mpmath), for the accuracy figure
    make_scene, chain, flight_scene          sessions: planted bodies among loose and static markers; the propagation's worst case;
                                             the frame-major flight of the end-to-end test
"""
import math

import numpy as np

INF = float("inf")
NAN = float("nan")
TILE, WAVE = 256, 64
INT_OUT = ("cnt", "group_of", "gsize", "ghead", "gconf")
F64_OUT = ("dist", "spread", "travel", "gspread")


def same_bits(a, b):
    """Two float arrays equal bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def same(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in INT_OUT) and int(a["n_groups"]) == int(b["n_groups"])
            and all(same_bits(a[k], b[k]) for k in F64_OUT))


# ---------------------------------------------------------------------------------------------------------------------- the tree
def _halve(v):
    """The six halving steps of one wave: v[l] = v[l] + v[l + off], off = 32 .. 1 -> v[0]."""
    v = list(v)
    off = WAVE // 2
    while off:
        for l in range(off):
            v[l] = v[l] + v[l + off]
        off //= 2
    return v[0]


def tree_sum_scalar(values):
    """values: one Python float per frame (+0.0 where the frame does not count) -> SUM by the contract's tree."""
    F = len(values)
    P = (F + TILE - 1) // TILE
    tiles = []
    for T in range(P):
        lanes = [values[TILE * T + l] if TILE * T + l < F else 0.0 for l in range(TILE)]
        w = [_halve(lanes[WAVE * k:WAVE * k + WAVE]) for k in range(TILE // WAVE)]
        s = w[0]
        for k in range(1, TILE // WAVE):
            s = s + w[k]
        tiles.append(s)
    c = (P + WAVE - 1) // WAVE
    lanes = []
    for l in range(WAVE):
        acc = 0.0
        for e in range(c * l, min(c * l + c, P)):
            acc = acc + tiles[e]
        lanes.append(acc)
    return _halve(lanes)


def _halve_np(V):
    off = WAVE // 2
    while off:
        V = V[..., :off] + V[..., off:2 * off]
        off //= 2
    return V[..., 0]


def tree_sum(V):
    """The same tree over the last axis of V (values >= +0.0, NaN or inf: the padding is +0.0)."""
    V = np.asarray(V, dtype=np.float64)
    F = V.shape[-1]
    P = (F + TILE - 1) // TILE
    pad = np.zeros(V.shape[:-1] + (P * TILE - F,))
    W = _halve_np(np.concatenate([V, pad], axis=-1).reshape(V.shape[:-1] + (P, TILE // WAVE, WAVE)))
    tiles = W[..., 0]
    for k in range(1, TILE // WAVE):
        tiles = tiles + W[..., k]
    c = (P + WAVE - 1) // WAVE
    X = np.concatenate([tiles, np.zeros(V.shape[:-1] + (c * WAVE - P,))], axis=-1).reshape(V.shape[:-1] + (WAVE, c))
    acc = np.zeros(V.shape[:-1] + (WAVE,))
    for e in range(c):
        acc = acc + X[..., e]
    return _halve_np(acc)


# ---------------------------------------------------------------------------------------------------------------------- pair statistics
def present_mask(traj):
    return np.isfinite(np.asarray(traj, dtype=np.float64)).all(axis=2)


def pair_stats_scalar(traj):
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    pres = present_mask(traj)
    cnt = np.zeros((R, R), dtype=np.int32)
    dist, spread = np.full((R, R), NAN), np.full((R, R), NAN)
    for p in range(R):
        for q in range(p, R):
            D, n = [], 0
            for f in range(F):
                if pres[p, f] and pres[q, f]:
                    dx, dy, dz = (float(traj[p, f, k]) - float(traj[q, f, k]) for k in range(3))
                    D.append(math.sqrt((dx * dx + dy * dy) + dz * dz))
                    n += 1
                else:
                    D.append(None)
            cnt[p, q] = cnt[q, p] = n
            if n:
                mean = tree_sum_scalar([0.0 if d is None else d for d in D]) / n
                sq = []
                for d in D:
                    e = 0.0 if d is None else d - mean
                    sq.append(0.0 if d is None else e * e)
                s = tree_sum_scalar(sq) / n
                dist[p, q] = dist[q, p] = mean
                spread[p, q] = spread[q, p] = math.sqrt(s) if s == s else NAN
    return cnt, dist, spread


def pair_stats(traj):
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    pres = present_mask(traj)
    cnt = np.zeros((R, R), dtype=np.int32)
    dist, spread = np.full((R, R), NAN), np.full((R, R), NAN)
    with np.errstate(all="ignore"):
        for p in range(R):
            both = pres[p][None, :] & pres[p:]
            d = np.where(both[:, :, None], traj[p][None] - traj[p:], 0.0)
            D = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            n = both.sum(axis=1)
            mean = tree_sum(np.where(both, D, 0.0)) / n
            e = D - mean[:, None]
            s = np.sqrt(tree_sum(np.where(both, e * e, 0.0)) / n)
            cnt[p, p:] = cnt[p:, p] = n
            dist[p, p:] = dist[p:, p] = np.where(n > 0, mean, NAN)
            spread[p, p:] = spread[p:, p] = np.where(n > 0, s, NAN)
    return cnt, dist, spread


def travel_of(traj):
    traj = np.asarray(traj, dtype=np.float64)
    pres = present_mask(traj)
    out = np.full(traj.shape[0], NAN)
    for r in range(traj.shape[0]):
        if pres[r].any():
            x = traj[r][pres[r]]
            e = [float(x[:, k].max()) - float(x[:, k].min()) for k in range(3)]
            s = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            out[r] = math.sqrt(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------- groups
def edges_of(cnt, dist, spread, travel, min_common, tol, max_dist, min_travel):
    R = cnt.shape[0]
    with np.errstate(invalid="ignore"):
        elig = (np.diag(cnt) >= min_common) & (travel >= min_travel)
        edge = (elig[:, None] & elig[None, :] & ~np.eye(R, dtype=bool) & (cnt >= min_common) & (spread <= tol) & (dist <= max_dist))
    return elig, edge


def groups_of(cnt, dist, spread, travel, min_common, tol, max_dist, min_travel):
    """Connected components by a plain union-find, numbered by their lowest row, and the per-group figures."""
    R = cnt.shape[0]
    _, edge = edges_of(cnt, dist, spread, travel, min_common, tol, max_dist, min_travel)
    parent = list(range(R))

    def find(r):
        while parent[r] != r:
            r = parent[r]
        return r

    for p in range(R):
        for q in range(p + 1, R):
            if edge[p, q]:
                a, b = find(p), find(q)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = [find(r) for r in range(R)]
    heads = sorted({roots[r] for r in range(R) if edge[r].any()})
    number = {h: g for g, h in enumerate(heads)}
    group_of = np.array([number[roots[r]] if edge[r].any() else -1 for r in range(R)], dtype=np.int32)
    gsize, ghead, gconf = (np.full(R, -1, dtype=np.int32) for _ in range(3))
    gspread = np.full(R, NAN)
    for g, h in enumerate(heads):
        rows = [r for r in range(R) if group_of[r] == g]
        gsize[g], ghead[g] = len(rows), h
        gconf[g] = sum(1 for i, p in enumerate(rows) for q in rows[i + 1:] if cnt[p, q] >= min_common and not spread[p, q] <= tol)
        gspread[g] = max(float(spread[p, q]) for p in rows for q in rows if edge[p, q])
    return {"group_of": group_of, "gsize": gsize, "ghead": ghead, "gconf": gconf, "gspread": gspread, "n_groups": len(heads)}


def _finish(stats, traj, min_common, tol, max_dist, min_travel):
    cnt, dist, spread = stats
    travel = travel_of(traj)
    out = {"cnt": cnt, "dist": dist, "spread": spread, "travel": travel}
    out.update(groups_of(cnt, dist, spread, travel, min_common, tol, max_dist, min_travel))
    return out


def rigid_groups_scalar(traj, min_common, tol, max_dist=INF, min_travel=0.0):
    return _finish(pair_stats_scalar(traj), traj, min_common, tol, max_dist, min_travel)


def rigid_groups(traj, min_common, tol, max_dist=INF, min_travel=0.0):
    return _finish(pair_stats(traj), traj, min_common, tol, max_dist, min_travel)


def rows_of_groups(res):
    """[[rows]] per group, in group order."""
    return [np.flatnonzero(res["group_of"] == g).tolist() for g in range(int(res["n_groups"]))]


# ---------------------------------------------------------------------------------------------------------------------- 50 digits
def pair_stats_mp(traj, digits=50):
    """-> (dist, spread) [R][R] as nested lists of mpmath numbers (None where no frame is shared): exact sums of the float64 inputs."""
    import mpmath as mp
    traj = np.asarray(traj, dtype=np.float64)
    R, F, _ = traj.shape
    pres = present_mask(traj)
    dist, spread = [[None] * R for _ in range(R)], [[None] * R for _ in range(R)]
    with mp.workdps(digits):
        X = [[[mp.mpf(float(v)) for v in traj[r, f]] if pres[r, f] else None for f in range(F)] for r in range(R)]
        for p in range(R):
            for q in range(p, R):
                D = [mp.sqrt(sum((a - b) ** 2 for a, b in zip(X[p][f], X[q][f]))) for f in range(F) if pres[p, f] and pres[q, f]]
                if D:
                    mean = mp.fsum(D) / len(D)
                    dist[p][q] = dist[q][p] = mean
                    spread[p][q] = spread[q][p] = mp.sqrt(mp.fsum((d - mean) ** 2 for d in D) / len(D))
    return dist, spread


# ---------------------------------------------------------------------------------------------------------------------- sessions
def random_rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rodrigues(w):
    """Rotation matrices of the rotation vectors w [F][3]."""
    th = np.linalg.norm(w, axis=1)
    k = w / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((w.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def template(rng, N, size=0.12, min_sep=0.06):
    """N markers of a body: random in a cube of +- size, no two closer than min_sep."""
    while True:
        q = rng.uniform(-size, size, (N, 3))
        d = np.linalg.norm(q[:, None] - q[None], axis=2) + np.eye(N)
        if d.min() >= min_sep:
            return q - q.mean(axis=0)


def rigid_motion(rng, tau, amplitude=1.0, spin=None):
    """A seeded rigid motion over the times tau [F] (seconds from 0): free flight of the origin (constant acceleration, scaled by
    `amplitude`) and a rotation vector that swings with two frequencies per axis (scaled by `spin`, default = amplitude)
    -> (Rm [F][3][3], c [F][3])."""
    spin = amplitude if spin is None else spin
    p0 = rng.uniform(-1.0, 1.0, 3)
    v0 = amplitude * rng.uniform(-0.6, 0.6, 3)
    a0 = amplitude * rng.uniform(-1.0, 1.0, 3)
    c = p0 + v0 * tau[:, None] + 0.5 * a0 * tau[:, None] ** 2
    f1, f2, ph = rng.uniform(0.3, 0.9, 3), rng.uniform(1.0, 2.0, 3), rng.uniform(0, 2 * np.pi, (2, 3))
    w = spin * (1.2 * np.sin(2 * np.pi * f1 * tau[:, None] + ph[0]) + 0.5 * np.sin(2 * np.pi * f2 * tau[:, None] + ph[1]))
    return _rodrigues(w) @ random_rotation(rng), c


def make_scene(seed, F, bodies=(4, 5), n_loose=2, n_static=1, sigma=0.0005, dropout=0.05, amplitude=1.0, rate=120.0, shuffle=True):
    """Rows of a gathered session: the markers of the planted bodies under seeded rigid motions, loose markers in flights of their
    own, static markers, `sigma` of noise on every sample, a fraction `dropout` of the samples NaN.
    -> (traj [R][F][3], owner [R]: the body of each row, -1 = loose, -2 = static), the rows shuffled."""
    rng = np.random.default_rng(seed)
    tau = np.arange(F) / rate
    rows, owner = [], []
    for b, N in enumerate(bodies):
        q = template(rng, N)
        Rm, c = rigid_motion(rng, tau, amplitude)
        for m in range(N):
            rows.append(np.einsum("fij,j->fi", Rm, q[m]) + c)
            owner.append(b)
    for _ in range(n_loose):
        rows.append(rigid_motion(rng, tau, amplitude)[1])
        owner.append(-1)
    for _ in range(n_static):
        rows.append(np.tile(rng.uniform(-1.0, 1.0, 3), (F, 1)))
        owner.append(-2)
    traj = np.array(rows) + sigma * rng.standard_normal((len(rows), F, 3))
    traj[rng.uniform(size=traj.shape[:2]) < dropout] = np.nan
    order = rng.permutation(len(rows)) if shuffle else np.arange(len(rows))
    return traj[order], np.array(owner)[order]


def chain(R, F=120, seed=3, segment=0.1):
    """Rows on a polyline in the plane z = 0 with fixed segment lengths and joint angles that move, each at its own frequency:
    only consecutive rows are rigid -- R - 1 edges in one line, the propagation's worst case -- and every other pair's distance
    varies by centimetres: a conflict.  No noise, no dropout.  -> traj [R][F][3]; groups with tol = 1e-6, min_common = 2."""
    rng = np.random.default_rng(seed)
    tau = np.arange(F) / 120.0
    # the bending angle at each joint: around 0.5 rad, swinging by 0.3 rad; headings accumulate
    bend = 0.5 * rng.choice([-1.0, 1.0], R)[:, None] + 0.3 * np.sin(2 * np.pi * rng.uniform(0.5, 3.0, R)[:, None] * tau[None] + rng.uniform(0, 6.28, R)[:, None])
    heading = np.cumsum(bend, axis=0)
    step = segment * np.stack([np.cos(heading), np.sin(heading), np.zeros_like(heading)], axis=2)      # [R][F][3]
    traj = np.cumsum(step, axis=0)
    traj[:, :, 2] = 0.05 * tau[None]
    return traj


CHAIN = dict(min_common=2, tol=1e-6, max_dist=INF, min_travel=0.0)


# the end-to-end flight: a 4-marker and a 5-marker body in different free flights, two loose markers, one static marker
FLIGHT_BODIES = (4, 5)
FLIGHT_TRACKER = dict(gate=0.05, max_missed=6, vel_alpha=0.5, T_max=32)
FLIGHT_STITCH = dict(fit_frames=8, max_dt=0.5, gate=0.03, gate_rate=0.3)
FLIGHT_TABLE = dict(min_hits=1, min_len=10)
FLIGHT_GROUPS = dict(tol=0.003, min_common=50)


def flight_scene(seed=41, F=400, K=16, sigma=0.0005, amplitude=0.6, spin=0.15):
    """400 frames at 120 Hz (20 % jitter), frame-major as the frame path writes them: slots shuffled per frame, `sigma` of noise,
    every marker hidden once for 10 .. 25 frames -- longer than the tracker's max_missed = 6, so its id splits.
    -> t [F], xyz [F][K][3], n_pts [F], slot_of [M][F] (-1 = hidden), owner [M], templates [[N][3]], truth [M][F][3]."""
    rng = np.random.default_rng(seed)
    t = 1.0 + np.cumsum((1.0 + 0.2 * rng.uniform(-1.0, 1.0, F)) / 120.0)
    tau = t - t[0]
    truth, owner, templates = [], [], []
    for b, N in enumerate(FLIGHT_BODIES):
        q = template(rng, N)
        templates.append(q)
        Rm, c = rigid_motion(rng, tau, amplitude, spin)     # a slow swing: a hidden marker still comes back inside the stitcher's gate
        c = c + np.array([3.0 * b, 0.0, 0.0])                   # the two bodies fly in halls of their own: no marker meets another
        for m in range(N):
            truth.append(np.einsum("fij,j->fi", Rm, q[m]) + c)
            owner.append(b)
    for i in range(2):
        truth.append(rigid_motion(rng, tau, amplitude)[1] + np.array([0.0, 4.0 + 3.0 * i, 0.0]))
        owner.append(-1)
    truth.append(np.tile(np.array([-3.0, -3.0, 0.0]), (F, 1)))
    owner.append(-2)
    truth = np.array(truth)
    M = truth.shape[0]
    seen = np.ones((M, F), dtype=bool)
    for m in range(M):
        f0, L = int(rng.integers(40, F - 60)), int(rng.integers(10, 26))
        seen[m, f0:f0 + L] = False
    xyz = np.full((F, K, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    slot_of = np.full((M, F), -1)
    for f in range(F):
        order = rng.permutation(np.nonzero(seen[:, f])[0])
        n_pts[f] = order.size
        for j, m in enumerate(order):
            xyz[f, j] = truth[m, f] + sigma * rng.standard_normal(3)
            slot_of[m, f] = j
    return t, xyz, n_pts, slot_of, np.array(owner), templates, truth


def fresh_frames(seed, templates, n_frames=60, K=16, sigma=0.0005, dropout=0.3):
    """Fresh frames of the two planted bodies for the locator: a random pose per frame and body, the bodies 3 m apart, markers dropped
    with probability `dropout`, slots shuffled.  -> xyz [F][K][3], n_pts [F], shown [bodies][F][N] bool."""
    rng = np.random.default_rng(seed)
    xyz = np.full((n_frames, K, 3), np.nan)
    n_pts = np.zeros(n_frames, dtype=np.int32)
    shown = [np.zeros((n_frames, q.shape[0]), dtype=bool) for q in templates]
    for f in range(n_frames):
        pts = []
        for b, q in enumerate(templates):
            Rm, c = random_rotation(rng), rng.uniform(-0.5, 0.5, 3) + np.array([3.0 * b, 0.0, 0.0])
            for m in range(q.shape[0]):
                if rng.random() >= dropout:
                    shown[b][f, m] = True
                    pts.append(Rm @ q[m] + c + sigma * rng.standard_normal(3))
        for j, src in enumerate(rng.permutation(len(pts))):
            xyz[f, j] = pts[src]
        n_pts[f] = len(pts)
    return xyz, n_pts, shown
