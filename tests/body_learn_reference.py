"""Plain statement of the rigid-body learning contract of include/mocap_core.h ("rigid-body learning"), for the tests.

  - gather():        the valid-frame rule and the slot each selected marker is present at
  - learn():         the contract in float64 NumPy: reference frame, rounds, pair statistics.  Sums over frames are sequential
                     (np.cumsum), poses by numpy's eigh on Horn's matrix; it is NOT meant to match the device's reduction
                     tree bit for bit, only to state the same mathematics in the same number format
  - learn_mp():      the same statement with 50 significant digits (mpmath; the pose is rigid_body_reference.pose_mp)
  - field_errors():  worst |value - 50-digit value| per continuous field
  - make_capture():  a planted template under a random rigid motion per frame, with noise, per-marker dropout, clutter with
                     other ids, shuffled slots, and optionally a "foreign" id that moves on its own
  - displace():      one marker of some frames moved off the body
  - align():         Kabsch alignment of a learned template to the planted one

Both learn() and learn_mp() return the keys of MocapCore.learn_rigid_body plus "frame_rms" [iters][F]: the rms of every posed
frame per round (NaN / None where the frame was not posed), which the tests need to keep the gate away from a tie."""
import math

import numpy as np

import rigid_body_reference as rb

MAX_MARKERS = 8
ST_NO_REF, ST_MARKER_UNSEEN = 1, 2
FIELDS = ("markers", "marker_rms", "pair_mean", "pair_std", "rms")          # continuous outputs
DISCRETE = ("marker_frames", "pair_frames", "frames_used", "frames_valid", "ref_frame", "status")


def gather(xyz, n_pts, ids, sel, status=None):
    """-> slots [F][N] (the lowest slot j < n_pts[f] with ids[f][j] == sel[m] and a finite point, -1 = absent), valid [F]."""
    xyz = np.asarray(xyz, dtype=np.float64)
    F, K_max, _ = xyz.shape
    n_pts = np.asarray(n_pts).reshape(F)
    valid = (n_pts >= 0) & (n_pts <= K_max)
    if status is not None:
        valid &= np.asarray(status).reshape(F) == 0
    slots = np.full((F, len(sel)), -1, dtype=np.int64)
    for f in np.nonzero(valid)[0]:
        n = int(n_pts[f])
        ok = np.isfinite(xyz[f, :n]).all(axis=1)
        for m, s in enumerate(sel):
            hit = np.nonzero((ids[f, :n] == s) & ok)[0]
            if hit.size:
                slots[f, m] = hit[0]
    return slots, valid


def _seq(a, axis=0):
    """Sequential sum along `axis` (np.sum is pairwise)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(a.shape[:axis] + a.shape[axis + 1:])
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def _empty(N, iters, F):
    return {"markers": np.zeros((N, 3)), "marker_rms": np.zeros(N), "marker_frames": np.zeros(N, dtype=np.int64),
            "pair_mean": np.zeros((N, N)), "pair_std": np.zeros((N, N)), "pair_frames": np.zeros((N, N), dtype=np.int64),
            "frames_used": 0, "frames_valid": 0, "ref_frame": -1, "rms": 0.0, "status": ST_NO_REF,
            "frame_rms": np.full((iters, F), np.nan)}


def _reference_frame(slots, valid, ref_frame):
    complete = valid & (slots >= 0).all(axis=1)
    if ref_frame < 0:
        idx = np.nonzero(complete)[0]
        return int(idx[0]) if idx.size else -1
    return int(ref_frame) if complete[ref_frame] else -1


def _pose_batch(Q, P):
    """Q [c][3] against P [n][c][3] -> R [n][3][3], t [n][3], rms [n]; the contract's route with numpy's eigh."""
    c = Q.shape[0]
    inv = 1.0 / c
    qb = _seq(Q) * inv
    pb = _seq(P, axis=1) * inv
    mq, wp = Q - qb, P - pb[:, None, :]
    S = np.zeros((P.shape[0], 3, 3))
    for m in range(c):
        S = S + mq[m][None, :, None] * wp[:, m][:, None, :]
    H = np.empty((P.shape[0], 4, 4))
    rows = rb._horn_matrix([[S[:, i, j] for j in range(3)] for i in range(3)])
    for i in range(4):
        for j in range(4):
            H[:, i, j] = rows[i][j]
    w, V = np.linalg.eigh(H)
    q = V[:, :, -1]
    q = q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    Rl = rb._quat_to_R(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    R = np.stack([np.stack(row, axis=-1) for row in Rl], axis=-2)
    t = pb - np.einsum("nij,j->ni", R, qb)
    r = np.einsum("nij,mj->nmi", R, mq) - wp
    rms = np.sqrt(_seq((r * r).reshape(P.shape[0], -1), axis=1) * inv)
    return R, t, rms


def learn(xyz, n_pts, ids, sel, status=None, ref_frame=-1, iters=4, max_rms=float("inf")):
    xyz = np.asarray(xyz, dtype=np.float64)
    ids = np.asarray(ids)
    F, N = xyz.shape[0], len(sel)
    slots, valid = gather(xyz, n_pts, ids, sel, status)
    present = slots >= 0
    out = _empty(N, iters, F)
    ref = _reference_frame(slots, valid, ref_frame)
    if ref < 0:
        return out
    out.update(status=0, ref_frame=ref, frames_valid=int(valid.sum()))
    pts = np.where(present[:, :, None], xyz[np.arange(F)[:, None], np.maximum(slots, 0)], 0.0)      # [F][N][3]
    for i in range(N):
        for j in range(i + 1, N):
            both = present[:, i] & present[:, j]
            c = int(both.sum())
            if c:
                d = pts[both, i] - pts[both, j]
                D = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                mean = _seq(D) / c
                out["pair_mean"][i, j] = out["pair_mean"][j, i] = mean
                out["pair_std"][i, j] = out["pair_std"][j, i] = math.sqrt(_seq((D - mean) ** 2) / c)
                out["pair_frames"][i, j] = out["pair_frames"][j, i] = c
    Q = pts[ref] - _seq(pts[ref]) * (1.0 / N)
    masks = (present * (1 << np.arange(N))).sum(axis=1)
    for r in range(iters):
        Y, cnt, e2 = np.zeros((F, N, 3)), np.zeros((F, N)), np.zeros((F, N))
        used, rms2 = np.zeros(F), np.zeros(F)
        for mask in np.unique(masks):
            sub = [m for m in range(N) if mask >> m & 1]
            if len(sub) < 3:
                continue
            fr = np.nonzero(masks == mask)[0]
            R, t, rms = _pose_batch(Q[sub], pts[fr][:, sub])
            out["frame_rms"][r, fr] = rms
            ok = rms <= max_rms
            fr, R, t, rms = fr[ok], R[ok], t[ok], rms[ok]
            y = np.einsum("nji,nmj->nmi", R, pts[fr][:, sub] - t[:, None, :])
            e = y - Q[sub][None]
            Y[fr[:, None], np.array(sub)[None, :]] = y
            cnt[fr[:, None], np.array(sub)[None, :]] = 1.0
            e2[fr[:, None], np.array(sub)[None, :]] = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
            used[fr], rms2[fr] = 1.0, rms * rms
        sy, sc, se = _seq(Y), _seq(cnt), _seq(e2)
        Qn = Q.copy()
        for m in range(N):
            if sc[m] > 0:
                Qn[m] = sy[m] / sc[m]
                out["marker_rms"][m] = math.sqrt(se[m] / sc[m])
            else:
                out["status"] |= ST_MARKER_UNSEEN
                out["marker_rms"][m] = 0.0
        Q = Qn - _seq(Qn) * (1.0 / N)
        n_used = _seq(used)
        out.update(markers=Q.copy(), marker_frames=sc.astype(np.int64), frames_used=int(n_used),
                   rms=math.sqrt(_seq(rms2) / n_used) if n_used > 0 else 0.0)
    return out


def learn_mp(xyz, n_pts, ids, sel, status=None, ref_frame=-1, iters=4, max_rms=float("inf"), digits=50):
    """The same contract with `digits` significant digits: continuous fields as (nested lists of) mpmath numbers."""
    import mpmath as mp
    xyz = np.asarray(xyz, dtype=np.float64)
    F, N = xyz.shape[0], len(sel)
    slots, valid = gather(xyz, n_pts, np.asarray(ids), sel, status)
    out = _empty(N, iters, F)
    out["frame_rms"] = [[None] * F for _ in range(iters)]
    ref = _reference_frame(slots, valid, ref_frame)
    if ref < 0:
        return out
    out.update(status=0, ref_frame=ref, frames_valid=int(valid.sum()))
    with mp.workdps(digits):
        gate = mp.inf if math.isinf(max_rms) else mp.mpf(float(max_rms))
        pt = lambda f, m: [mp.mpf(float(v)) for v in xyz[f, slots[f, m]]]
        z = mp.mpf(0)
        mean = [[z] * N for _ in range(N)]
        std = [[z] * N for _ in range(N)]
        for i in range(N):
            for j in range(i + 1, N):
                fr = [f for f in range(F) if slots[f, i] >= 0 and slots[f, j] >= 0]
                if fr:
                    D = [mp.sqrt(sum((a - b) ** 2 for a, b in zip(pt(f, i), pt(f, j)))) for f in fr]
                    mean[i][j] = mean[j][i] = sum(D) / len(D)
                    std[i][j] = std[j][i] = mp.sqrt(sum((d - mean[i][j]) ** 2 for d in D) / len(D))
                    out["pair_frames"][i, j] = out["pair_frames"][j, i] = len(D)
        P0 = [pt(ref, m) for m in range(N)]
        c0 = [sum(p[k] for p in P0) / N for k in range(3)]
        Q = [[p[k] - c0[k] for k in range(3)] for p in P0]
        mrms = [z] * N
        for r in range(iters):
            sy = [[z, z, z] for _ in range(N)]
            sc, se, n_used, rms2 = [0] * N, [z] * N, 0, z
            for f in range(F):
                sub = [m for m in range(N) if slots[f, m] >= 0]
                if len(sub) < 3:
                    continue
                P = [pt(f, m) for m in sub]
                R, t, rms = _pose_mp_exact([Q[m] for m in sub], P, mp)
                out["frame_rms"][r][f] = rms
                if not rms <= gate:
                    continue
                n_used += 1
                rms2 += rms * rms
                for m, p in zip(sub, P):
                    d = [p[k] - t[k] for k in range(3)]
                    y = [sum(R[j][k] * d[j] for j in range(3)) for k in range(3)]
                    for k in range(3):
                        sy[m][k] += y[k]
                    sc[m] += 1
                    se[m] += sum((y[k] - Q[m][k]) ** 2 for k in range(3))
            Qn = []
            for m in range(N):
                if sc[m]:
                    Qn.append([sy[m][k] / sc[m] for k in range(3)])
                    mrms[m] = mp.sqrt(se[m] / sc[m])
                else:
                    Qn.append(list(Q[m]))
                    mrms[m] = z
                    out["status"] |= ST_MARKER_UNSEEN
            c = [sum(q[k] for q in Qn) / N for k in range(3)]
            Q = [[q[k] - c[k] for k in range(3)] for q in Qn]
            out.update(markers=[list(q) for q in Q], marker_rms=list(mrms), marker_frames=np.array(sc, dtype=np.int64),
                       frames_used=n_used, rms=mp.sqrt(rms2 / n_used) if n_used else z)
        out.update(pair_mean=mean, pair_std=std)
    return out


def _pose_mp_exact(Q, P, mp):
    """rigid_body_reference.pose_mp on operands that already are mpmath numbers (the template of a later round is not a double)."""
    n = len(Q)
    qb = [sum(r[k] for r in Q) / n for k in range(3)]
    pb = [sum(r[k] for r in P) / n for k in range(3)]
    S = [[sum((Q[i][a] - qb[a]) * (P[i][b] - pb[b]) for i in range(n)) for b in range(3)] for a in range(3)]
    E, V = mp.eigsy(mp.matrix(rb._horn_matrix(S)))
    k = max(range(4), key=lambda i: E[i])
    q = [V[i, k] for i in range(4)]
    nq = mp.sqrt(sum(v * v for v in q))
    R = rb._quat_to_R(*[v / nq for v in q])
    t = [pb[i] - sum(R[i][j] * qb[j] for j in range(3)) for i in range(3)]
    ss = mp.mpf(0)
    for i in range(n):
        for r in range(3):
            e = sum(R[r][j] * (Q[i][j] - qb[j]) for j in range(3)) - (P[i][r] - pb[r])
            ss += e * e
    return R, t, mp.sqrt(ss / n)


def gate_margin(exact, max_rms):
    """The smallest |rms - max_rms| / max_rms over every posed frame of every round of a learn_mp result (inf without a gate)."""
    import mpmath as mp
    if math.isinf(max_rms):
        return float("inf")
    with mp.workdps(50):
        g = mp.mpf(float(max_rms))
        m = [abs(v - g) / g for row in exact["frame_rms"] for v in row if v is not None]
        return float(min(m)) if m else float("inf")


def field_errors(got, exact):
    """{field: (worst |got - exact|, largest |exact|)} over FIELDS, evaluated in mpmath; got holds doubles, exact learn_mp's values."""
    import mpmath as mp
    out = {}
    with mp.workdps(50):
        for k in FIELDS:
            g = np.asarray(got[k], dtype=np.float64).reshape(-1)
            e = exact[k]
            flat = [e] if not isinstance(e, (list, np.ndarray)) else [v for row in e for v in (row if isinstance(row, (list, np.ndarray)) else [row])]
            assert len(flat) == g.size, (k, len(flat), g.size)
            out[k] = (float(max(abs(mp.mpf(float(a)) - mp.mpf(b)) for a, b in zip(g, flat))), float(max(abs(mp.mpf(b)) for b in flat)))
    return out


def same_discrete(a, b):
    """The names of the discrete outputs in which two results differ."""
    return [k for k in DISCRETE if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


# ---------------------------------------------------------------- synthetic captures
def make_capture(rng, template, F, K_max, noise=0.0005, dropout=0.0, n_clutter=0, shuffle=True, foreign=False, first_id=10,
                 cube=2.0, complete_first=True):
    """`template` [N][3] under a random rigid motion per frame.  Marker m carries track id first_id + m, clutter points ids from
    1000 up (a fresh one per point and frame), the foreign point (one per frame, a random walk of its own near the body) id first_id + N.  dropout = probability
    that a marker is missing from a frame (frame 0 is kept complete when complete_first).  Slots >= n_pts hold NaN and id -1.
    -> {"xyz", "n_pts", "id", "sel", "foreign_id", "R" [F][3][3], "t" [F][3], "shown" [F][N] bool}."""
    q = np.asarray(template, dtype=np.float64)
    N = q.shape[0]
    xyz = np.full((F, K_max, 3), np.nan)
    ids = np.full((F, K_max), -1, dtype=np.int32)
    n_pts = np.zeros(F, dtype=np.int32)
    Rs, ts, shown = np.zeros((F, 3, 3)), np.zeros((F, 3)), np.zeros((F, N), dtype=bool)
    walk = rng.uniform(-0.1, 0.1, 3)
    for f in range(F):
        R, t = rb.random_rotation(rng), rng.uniform(-cube / 2, cube / 2, 3)
        Rs[f], ts[f] = R, t
        pts, lab = [], []
        for m in range(N):
            if dropout and rng.random() < dropout and not (complete_first and f == 0):
                continue
            shown[f, m] = True
            pts.append(R @ q[m] + t + (rng.normal(0.0, noise, 3) if noise else 0.0))
            lab.append(first_id + m)
        if foreign:
            walk = walk + rng.normal(0.0, 0.02, 3)
            pts.append(t + walk)
            lab.append(first_id + N)
        for c in range(n_clutter):
            pts.append(rng.uniform(-cube / 2, cube / 2, 3))
            lab.append(1000 + f * n_clutter + c)
        n = len(pts)
        assert n <= K_max, (n, K_max)
        order = rng.permutation(n) if shuffle else np.arange(n)
        for slot, src in enumerate(order):
            xyz[f, slot], ids[f, slot] = pts[src], lab[src]
        n_pts[f] = n
    return {"xyz": xyz, "n_pts": n_pts, "id": ids, "sel": [first_id + m for m in range(N)], "foreign_id": first_id + N,
            "R": Rs, "t": ts, "shown": shown}


def displace(cap, frames, marker, offset):
    """Moves one marker by `offset` in those of `frames` that show it (frames a gate on the rms should reject)."""
    for f in frames:
        j = np.nonzero(cap["id"][f, :cap["n_pts"][f]] == cap["sel"][marker])[0]
        if j.size:
            cap["xyz"][f, j[0]] += offset


def align(learned, planted):
    """`learned` [N][3] rotated and shifted onto `planted` by Kabsch -> the aligned copy."""
    R, t, _ = rb.kabsch(learned, planted)
    return (R @ np.asarray(learned).T).T + t
