"""The "track stitching" contract of include/mocap_core.h in plain Python and NumPy, in the scalar order the header writes.

    stitch_scalar(t, traj, fit_frames, max_dt, gate, gate_rate) -> {"ext", "next", "prev", "cost", "chain", "row_of", "n_chains", "table"}
                                             THE statement: end_model, pair_cost and the greedy walk over the sorted (c, p, q), all in
                                             Python floats, one rounding per operation
    stitch(...)                              the same, the end models vectorised over the rows (the window walked in ascending g by a
                                             Python loop) and the pair costs over (p, q); compared with stitch_scalar bit for bit in
                                             tests/test_track_stitch_reference_cpu.py; the device is compared with this one
    associate_rounds(table)                  the device's scheme, rounds of mutually best pairs: the same links, and the round count
    cut_session, flight_session, ladder      sessions: rows cut into fragments, a tracked flight with long occlusions, the
                                             association's worst case
"""
import numpy as np

import track_smooth_reference as ts

INF = float("inf")
NAN = float("nan")
INT_OUT = ("ext", "next", "prev", "chain", "row_of")


# ---------------------------------------------------------------------------------------------------------------------- extents
def extents(t, traj):
    """-> (ext int32 [R][3], present [R][F])"""
    pres = ts.present_mask(t, traj)
    ext = np.zeros((pres.shape[0], 3), dtype=np.int32)
    for r, row in enumerate(pres):
        f = np.flatnonzero(row)
        ext[r] = (f[0], f[-1], f.size) if f.size else (-1, -1, 0)
    return ext, pres


# ---------------------------------------------------------------------------------------------------------------------- end models
def window_of(e, fit_frames, F, head):
    return (e, min(e + fit_frames, F - 1)) if head else (max(e - fit_frames, 0), e)


def end_model(t, row, pres_row, e, fit_frames, head):
    """The model of one end of one row in Python floats -> [pos x 3, vel x 3, t_e]; e = the end frame (present)."""
    lo, hi = window_of(e, fit_frames, len(t), head)
    te = float(t[e])
    gs = [g for g in range(lo, hi + 1) if pres_row[g]]
    s = [float(t[g]) - te for g in gs]
    h = 0.0
    for v in s:
        h = abs(v) if abs(v) > h else h
    pos, vel = [float(v) for v in row[e]], [0.0, 0.0, 0.0]
    if len(gs) >= 2:
        S0 = S1 = S2 = 0.0
        B0, B1 = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for g, v in zip(gs, s):
            u = ts._div(v, h)
            S0 = S0 + 1.0
            S1 = S1 + u
            S2 = S2 + u * u
            for k in range(3):
                B0[k] = B0[k] + float(row[g][k])
                B1[k] = B1[k] + u * float(row[g][k])
        det = S0 * S2 - S1 * S1
        if det > 0.0 and det < INF:
            pos = [ts._div(S2 * B0[k] - S1 * B1[k], det) for k in range(3)]
            vel = [ts._div(ts._div(S0 * B1[k] - S1 * B0[k], det), h) for k in range(3)]
    return pos + vel + [te]


def end_models(t, traj, ext, pres, fit_frames):
    """Vectorised over the rows -> (tail [R][7], head [R][7]); NaN for an empty row."""
    t = np.asarray(t, dtype=np.float64)
    R, F, _ = traj.shape
    full = ext[:, 2] != 0
    out = []
    with np.errstate(all="ignore"):
        for head in (False, True):
            e = np.where(full, ext[:, 0] if head else ext[:, 1], 0).astype(np.int64)
            lo = e if head else np.maximum(e - fit_frames, 0)
            hi = np.minimum(e + fit_frames, F - 1) if head else e
            te = t[e]
            rows = np.arange(R)

            def at(i):
                g = np.minimum(lo + i, F - 1)
                ok = full & (lo + i <= hi) & pres[rows, g]
                return ok, np.where(ok, t[g], 0.0) - np.where(ok, te, 0.0), np.where(ok[:, None], traj[rows, g], 0.0)

            m = np.zeros(R, dtype=np.int64)
            h = np.zeros(R)
            for i in range(fit_frames + 1):
                ok, s, _ = at(i)
                m += ok
                h = np.where(ok & (np.abs(s) > h), np.abs(s), h)
            S0, S1, S2 = np.zeros(R), np.zeros(R), np.zeros(R)
            B0, B1 = np.zeros((R, 3)), np.zeros((R, 3))
            for i in range(fit_frames + 1):
                ok, s, x = at(i)
                u = s / h
                S0 = np.where(ok, S0 + 1.0, S0)
                S1 = np.where(ok, S1 + u, S1)
                S2 = np.where(ok, S2 + u * u, S2)
                B0 = np.where(ok[:, None], B0 + x, B0)
                B1 = np.where(ok[:, None], B1 + u[:, None] * x, B1)
            det = S0 * S2 - S1 * S1
            fit = (m >= 2) & (det > 0.0) & (det < np.inf)
            pos = np.where(fit[:, None], (S2[:, None] * B0 - S1[:, None] * B1) / det[:, None], traj[rows, e])
            vel = np.where(fit[:, None], ((S0[:, None] * B1 - S1[:, None] * B0) / det[:, None]) / h[:, None], 0.0)
            model = np.concatenate([pos, vel, te[:, None]], axis=1)
            model[~full] = np.nan
            out.append(model)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------- pair costs
def pair_cost(T, H, b_p, a_q, max_dt, gate, gate_rate):
    """p -> q in Python floats: the cost c, or +inf for a pair that is not admissible (p != q and both non-empty is the caller's)."""
    if not b_p < a_q:
        return INF
    dt = H[6] - T[6]
    g = gate + gate_rate * dt
    g2 = g * g
    d = [H[k] - (T[k] + T[3 + k] * dt) for k in range(3)]
    e = [T[k] - (H[k] - H[3 + k] * dt) for k in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    c = 0.5 * (d2 + e2)
    return c if dt <= max_dt and c < g2 else INF


def cost_table(tail, head, ext, max_dt, gate, gate_rate):
    """Vectorised over (p, q) -> [R][R], +inf = not admissible."""
    R = ext.shape[0]
    with np.errstate(all="ignore"):
        T, H = tail[:, None, :], head[None, :, :]
        dt = H[..., 6] - T[..., 6]
        g = gate + gate_rate * dt
        g2 = g * g
        d = H[..., :3] - (T[..., :3] + T[..., 3:6] * dt[..., None])
        e = T[..., :3] - (H[..., :3] - H[..., 3:6] * dt[..., None])
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        e2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        c = 0.5 * (d2 + e2)
        full = ext[:, 2] != 0
        ok = (full[:, None] & full[None, :] & ~np.eye(R, dtype=bool) & (ext[:, 1][:, None] < ext[:, 0][None, :])
              & (dt <= max_dt) & (c < g2))
    return np.where(ok, c, np.inf)


# ---------------------------------------------------------------------------------------------------------------------- association
def associate_sorted(table):
    """THE rule: the admissible pairs in ascending (c, p, q); a pair commits iff p has no successor and q no predecessor yet."""
    R = table.shape[0]
    nxt, prv, cost = np.full(R, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32), np.full(R, np.nan)
    p, q = np.nonzero(table < np.inf)
    for i in np.lexsort((q, p, table[p, q])):
        if nxt[p[i]] < 0 and prv[q[i]] < 0:
            nxt[p[i]], prv[q[i]], cost[p[i]] = q[i], p[i], table[p[i], q[i]]
    return nxt, prv, cost


def associate_rounds(table):
    """Rounds of mutually best pairs under the same order -> (next, prev, cost, rounds that committed)."""
    R = table.shape[0]
    nxt, prv, cost = np.full(R, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32), np.full(R, np.nan)
    rounds = 0
    while True:
        free = np.where((nxt < 0)[:, None] & (prv < 0)[None, :], table, np.inf)
        succ, pred = free.argmin(axis=1), free.argmin(axis=0)          # argmin: the lowest index of equal costs
        hit = [p for p in range(R) if free[p, succ[p]] < np.inf and pred[succ[p]] == p]
        if not hit:
            return nxt, prv, cost, rounds
        rounds += 1
        for p in hit:
            nxt[p], prv[succ[p]], cost[p] = succ[p], p, table[p, succ[p]]


def finish(ext, nxt, prv, cost, table=None):
    R = ext.shape[0]
    chain = np.arange(R, dtype=np.int32)
    for r in range(R):
        while prv[chain[r]] >= 0:
            chain[r] = prv[chain[r]]
    heads = [r for r in range(R) if chain[r] == r and ext[r, 2] != 0]
    number = {r: i for i, r in enumerate(heads)}
    row_of = np.array([number[chain[r]] if ext[r, 2] != 0 else -1 for r in range(R)], dtype=np.int32)
    return {"ext": ext, "next": nxt, "prev": prv, "cost": cost, "chain": chain, "row_of": row_of, "n_chains": len(heads), "table": table}


# ---------------------------------------------------------------------------------------------------------------------- the statement
def stitch_scalar(t, traj, fit_frames, max_dt, gate, gate_rate):
    t, traj = np.asarray(t, dtype=np.float64), np.asarray(traj, dtype=np.float64)
    R = traj.shape[0]
    ext, pres = extents(t, traj)
    tail = [end_model(t, traj[r], pres[r], int(ext[r, 1]), fit_frames, False) if ext[r, 2] else None for r in range(R)]
    head = [end_model(t, traj[r], pres[r], int(ext[r, 0]), fit_frames, True) if ext[r, 2] else None for r in range(R)]
    pairs, table = [], np.full((R, R), np.inf)
    for p in range(R):
        for q in range(R):
            if p != q and ext[p, 2] and ext[q, 2]:
                c = pair_cost(tail[p], head[q], int(ext[p, 1]), int(ext[q, 0]), max_dt, gate, gate_rate)
                if c < INF:
                    pairs.append((c, p, q))
                    table[p, q] = c
    nxt, prv, cost = np.full(R, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32), np.full(R, np.nan)
    for c, p, q in sorted(pairs):
        if nxt[p] < 0 and prv[q] < 0:
            nxt[p], prv[q], cost[p] = q, p, c
    out = finish(ext, nxt, prv, cost, table)
    out["tail"], out["head"] = tail, head
    return out


def stitch(t, traj, fit_frames, max_dt, gate, gate_rate):
    t, traj = np.asarray(t, dtype=np.float64), np.asarray(traj, dtype=np.float64)
    ext, pres = extents(t, traj)
    tail, head = end_models(t, traj, ext, pres, fit_frames)
    table = cost_table(tail, head, ext, max_dt, gate, gate_rate)
    out = finish(ext, *associate_sorted(table), table)
    out["tail"], out["head"] = tail, head
    return out


def same(a, b):
    """Two results equal: the integers exactly, cost bit for bit (any NaN equal to any NaN)."""
    return (all(np.array_equal(a[k], b[k]) for k in INT_OUT) and int(a["n_chains"]) == int(b["n_chains"])
            and ts.same_bits(a["cost"], b["cost"]))


def chains_of(res):
    """[[rows of a chain in time order]] in the order of row_of."""
    out = []
    for r in range(len(res["next"])):
        if res["row_of"][r] >= 0 and res["chain"][r] == r:
            out.append([r])
            while res["next"][out[-1][-1]] >= 0:
                out[-1].append(int(res["next"][out[-1][-1]]))
    return out


# ---------------------------------------------------------------------------------------------------------------------- sessions
def cut_session(traj, cuts, seed=None):
    """Rows cut into fragments: traj [M][F][3]; cuts = [(m, f, L)]: row m is hidden on the frames f .. f + L - 1, what follows becomes a
    row of its own.  -> (rows [M + len(cuts)][F][3], owner [rows]: the m of each).  seed shuffles the order of the rows."""
    M, F, _ = traj.shape
    frags = []
    for m in range(M):
        start = 0
        for _, f, L in sorted(c for c in cuts if c[0] == m):
            assert start < f and f + L < F, (m, f, L)
            frags.append((m, start, f))
            start = f + L
        frags.append((m, start, F))
    if seed is not None:
        frags = [frags[i] for i in np.random.default_rng(seed).permutation(len(frags))]
    rows = np.full((len(frags), F, 3), np.nan)
    for r, (m, lo, hi) in enumerate(frags):
        rows[r, lo:hi] = traj[m, lo:hi]
    return rows, np.array([m for m, _, _ in frags])


def flight_session(seed=77, F=400, K=8, sigma=0.0005):
    """Four markers in free flight (constant acceleration), 120 Hz with 20 % jitter, `sigma` of noise, shuffled slots, a few dropouts of
    1 .. 4 frames, and every marker hidden once or twice for 10 .. 25 frames: longer than a tracker's max_missed = 6, so its id splits.
    -> t [F], xyz [F][K][3], n_pts [F], slot_of [4][F] (-1 = hidden), hidden = [(marker, first frame, frames)]."""
    M = 4
    rng = np.random.default_rng(seed)
    t = 1.0 + np.cumsum((1.0 + 0.2 * rng.uniform(-1.0, 1.0, F)) / 120.0)
    tau = (t - t[0])[None, :, None]
    p0 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.2], [0.0, 1.0, 0.8], [1.0, 1.0, 1.5]])[:, None, :]
    v0 = np.array([0.4, -0.3, 0.5]) + 0.1 * rng.uniform(-1.0, 1.0, (M, 1, 3))
    a0 = np.array([0.3, 0.5, -1.0]) + 0.1 * rng.uniform(-1.0, 1.0, (M, 1, 3))
    truth = p0 + v0 * tau + 0.5 * a0 * tau * tau
    hidden = [(0, 100, 15), (1, 60, 20), (1, 250, 12), (2, 180, 25), (3, 120, 10), (3, 300, 18)]
    seen = np.ones((M, F), dtype=bool)
    for m, f, L in hidden:
        seen[m, f:f + L] = False
    for m in range(M):
        for f in rng.choice(np.arange(20, F - 20, 12), 6, replace=False):
            if seen[m, f - 8:f + 12].all():                       # short dropouts stay clear of the long ones
                seen[m, f:f + int(rng.integers(1, 5))] = False
    xyz = np.full((F, K, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    slot_of = np.full((M, F), -1)
    for f in range(F):
        order = rng.permutation(np.nonzero(seen[:, f])[0])
        n_pts[f] = order.size
        for j, m in enumerate(order):
            xyz[f, j] = truth[m, f] + sigma * rng.standard_normal(3)
            slot_of[m, f] = j
    return t, xyz, n_pts, slot_of, hidden


FLIGHT_TRACKER = dict(gate=0.05, max_missed=6, vel_alpha=0.5, T_max=16)
FLIGHT_STITCH = dict(fit_frames=8, max_dt=0.5, gate=0.03, gate_rate=0.3)
FLIGHT_TABLE = dict(min_hits=1, min_len=10)


def flight_truth(ids, slot_of):
    """The track ids each marker went through, in time order: [[ids]] per marker."""
    out = []
    for m in range(slot_of.shape[0]):
        seq = [int(ids[f, slot_of[m, f]]) for f in range(slot_of.shape[1]) if slot_of[m, f] >= 0]
        out.append([i for n, i in enumerate(seq) if n == 0 or i != seq[n - 1]])
    return out


def ladder(R, fit_frames=1):
    """The association's worst case, one commit per round.  Row r has two samples, a head sample at frame 3 r and a tail sample at frame
    3 r + 2, more than fit_frames = 1 apart: both end models are that sample with v = 0, and c(p -> q) = |head_q - tail_p|^2 exactly in
    x alone.  tail_p = 1e-4 p and head_q = L - 1.37e-4 q with L above both ramps: the cost falls strictly with p and with q, so every
    free row's best successor is the LAST row without a predecessor, whose best predecessor is the row just before it -- the only
    mutual pair of the round.  R - 1 rounds, one chain 0 -> 1 -> ... -> R - 1 committed from its far end.
    -> t [3 R], traj [R][3 R][3]; stitch with fit_frames 1, max_dt inf, gate 1.0, gate_rate 0."""
    assert fit_frames == 1
    F = 3 * R
    t = 10.0 + np.arange(F) / 128.0
    traj = np.full((R, F, 3), np.nan)
    L = 0.25 + 2.37e-4 * R
    for r in range(R):
        traj[r, 3 * r] = (L - 1.37e-4 * r, 0.0, 0.0)
        traj[r, 3 * r + 2] = (1e-4 * r, 0.0, 0.0)
    return t, traj


LADDER = dict(fit_frames=1, max_dt=INF, gate=1.0, gate_rate=0.0)
