"""Plain statement of the body-tracker contract of include/mocap_core.h ("body tracker"), for the tests.

  - Tracker:          the state (one slot per body) and one frame of the contract: prediction, guided association in two rounds,
                      the per-frame search as the fall-back (rigid_body_reference.locate), coasting, the update; run() walks a
                      batch and returns the arrays the C ABI writes.  The pose of an assignment is rigid_body_reference.kabsch
                      (SVD), where the device runs Horn / Jacobi: the two agree to a few ulp, which is why the scenes used on the
                      GPU must keep the margins the tracker records (gate, pair keys, rms) -- see margins_ok().
  - symmetric_body(), path_scene(), two_identical_scene(): bodies on smooth paths at 60 Hz with noise, clutter and
                      per-frame visibility masks.

Scalars are Python floats: IEEE double, one rounding per operation, nothing fused -- the arithmetic the contract prescribes
for the predicted markers, d2 and the velocity."""
import math

import numpy as np

from rigid_body_reference import DEFAULT_WORK_CAP, MAX_BODIES, MAX_MARKERS, Model, kabsch, locate, make_body, posable_table  # noqa: F401
from rigid_body_reference import pose_errors, pose_mp  # noqa: F401  (the GPU tests take them from here)

SRC_NONE, SRC_GUIDED, SRC_SEARCH, SRC_COAST = 0, 1, 2, 3
ST_BAD_TIME = 1
MARGIN = 1e-9


def _rel(a, b):
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else math.inf   # (two exact zeros never compete in a scene with noise)


class Tracker:
    def __init__(self, bodies, tol, max_rms, gate, max_missed, vel_alpha, work_cap=DEFAULT_WORK_CAP):
        self.bodies = [b if isinstance(b, Model) else Model(b) for b in bodies]
        self.tol, self.max_rms, self.work_cap = float(tol), float(max_rms), work_cap
        self.g2 = float(gate) * float(gate)
        self.max_missed, self.alpha = int(max_missed), float(vel_alpha)
        self.margin = {"gate": math.inf, "key": math.inf, "rms": math.inf}   # smallest relative distances to a decision
        self.reset()

    def reset(self):
        self.slots = [{"live": 0, "R": [0.0] * 9, "p": [0.0] * 3, "v": [0.0] * 3, "t_seen": 0.0, "missed": 0, "hits": 0}
                      for _ in range(MAX_BODIES)]

    def state(self):
        s = self.slots
        return {"live": np.array([x["live"] for x in s], dtype=np.int32), "R": np.array([x["R"] for x in s]).reshape(-1, 3, 3),
                "p": np.array([x["p"] for x in s]), "v": np.array([x["v"] for x in s]),
                "t_seen": np.array([x["t_seen"] for x in s]), "missed": np.array([x["missed"] for x in s], dtype=np.int32),
                "hits": np.array([x["hits"] for x in s], dtype=np.int32)}

    # ---- step 2, one round: -> assign [N] (point index or -1)
    def associate(self, model, Rc, pc, X, ok_pts):
        pairs = []
        for i in range(model.n):
            q = model.q[i].tolist()
            m = [((Rc[3 * r] * q[0] + Rc[3 * r + 1] * q[1]) + Rc[3 * r + 2] * q[2]) + pc[r] for r in range(3)]
            for j in ok_pts:
                dx, dy, dz = X[j][0] - m[0], X[j][1] - m[1], X[j][2] - m[2]
                d2 = (dx * dx + dy * dy) + dz * dz
                self.margin["gate"] = min(self.margin["gate"], _rel(d2, self.g2))
                if d2 < self.g2:
                    pairs.append((d2, i, j))
        pairs.sort()
        for a, b in zip(pairs, pairs[1:]):
            self.margin["key"] = min(self.margin["key"], _rel(a[0], b[0]))
        assign = [-1] * model.n
        taken = set()
        for d2, i, j in pairs:
            if assign[i] < 0 and j not in taken:
                assign[i] = j
                taken.add(j)
        return assign

    def _fit(self, model, assign, X):
        """-> (R [9], t [3], rms) of a posable assignment, else None."""
        sub = sum(1 << m for m, j in enumerate(assign) if j >= 0)
        if not model.posable[sub]:
            return None
        used = [m for m in range(model.n) if assign[m] >= 0]
        R, t, rms = kabsch(model.q[used], np.array([X[assign[m]] for m in used]))
        return [float(v) for v in R.reshape(9)], [float(v) for v in t], rms

    def frame(self, t, points, n):
        """One frame: points [K_max][3], its first n count.  -> (list of one dict per body, status)."""
        K_max = len(points)
        B = len(self.bodies)
        zero = lambda: {"tracked": 0, "source": SRC_NONE, "n_used": 0, "assign": [0] * MAX_MARKERS, "R": [0.0] * 9,   # noqa: E731
                        "t": [0.0] * 3, "rms": 0.0, "hits": 0, "missed": 0}
        if not math.isfinite(t):
            return [zero() for _ in range(B)], ST_BAD_TIME
        n = 0 if (n < 0 or n > K_max) else int(n)
        X = [[float(v) for v in row] for row in np.asarray(points, dtype=np.float64)]
        finite = [j for j in range(n) if all(math.isfinite(v) for v in X[j])]
        search = locate(points, n, self.bodies, self.tol, self.max_rms, self.work_cap, with_runner_up=False) if B else []
        Cl = set()
        out = []
        for b, model in enumerate(self.bodies):
            s = self.slots[b]
            o = zero()
            live = bool(s["live"])
            dt = t - s["t_seen"]
            ph = [s["p"][k] + s["v"][k] * dt for k in range(3)] if (live and dt > 0) else list(s["p"])
            res = None   # (source, assign, R, t, rms)
            if live:
                ok_pts = [j for j in finite if j not in Cl]
                a1 = self.associate(model, s["R"], ph, X, ok_pts)
                f1 = self._fit(model, a1, X)
                if f1 is not None:
                    self.margin["rms"] = min(self.margin["rms"], _rel(f1[2], self.max_rms))
                if f1 is not None and f1[2] <= self.max_rms:
                    res = (SRC_GUIDED, a1) + f1
                    a2 = self.associate(model, f1[0], f1[1], X, ok_pts)
                    f2 = self._fit(model, a2, X)
                    if f2 is not None:
                        self.margin["rms"] = min(self.margin["rms"], _rel(f2[2], self.max_rms))
                    if f2 is not None and f2[2] <= self.max_rms:
                        res = (SRC_GUIDED, a2) + f2
            if res is None and search[b]["found"] == 1:
                a = [int(v) for v in search[b]["assign"][:model.n]]
                if not any(j in Cl for j in a if j >= 0):
                    res = (SRC_SEARCH, a) + self._fit(model, a, X)
            if res is not None:
                src, a, Rn, tn, rms = res
                if live:
                    if dt > 0:
                        for k in range(3):
                            u = (tn[k] - s["p"][k]) / dt
                            s["v"][k] = s["v"][k] + self.alpha * (u - s["v"][k])
                else:
                    s["v"] = [0.0] * 3
                    s["hits"] = 0
                s.update(R=list(Rn), p=list(tn), t_seen=t, missed=0, hits=s["hits"] + 1, live=1)
                Cl |= {j for j in a if j >= 0}
                o.update(tracked=1, source=src, n_used=sum(1 for j in a if j >= 0), assign=list(a) + [-1] * (MAX_MARKERS - model.n),
                         R=list(Rn), t=list(tn), rms=rms, hits=s["hits"], missed=0)
            elif live:
                s["missed"] += 1
                if s["missed"] > self.max_missed:
                    s["live"] = 0
                else:
                    o.update(tracked=1, source=SRC_COAST, n_used=0, assign=[-1] * MAX_MARKERS, R=list(s["R"]), t=ph, rms=0.0,
                             hits=s["hits"], missed=s["missed"])
            out.append(o)
        return out, 0

    def run(self, t, xyz, n_pts, B_max=None):
        """A batch, frames in order -> the arrays of mocap_track_bodies, [F][B_max]."""
        F = len(t)
        B = len(self.bodies)
        B_max = B if B_max is None else B_max
        o = {"tracked": np.zeros((F, B_max), dtype=np.int32), "source": np.zeros((F, B_max), dtype=np.int32),
             "n_used": np.zeros((F, B_max), dtype=np.int32), "assign": np.zeros((F, B_max, MAX_MARKERS), dtype=np.int8),
             "R": np.zeros((F, B_max, 3, 3)), "t": np.zeros((F, B_max, 3)), "rms": np.zeros((F, B_max)),
             "hits": np.zeros((F, B_max), dtype=np.int32), "missed": np.zeros((F, B_max), dtype=np.int32),
             "status": np.zeros(F, dtype=np.int32)}
        for f in range(F):
            res, st = self.frame(float(t[f]), xyz[f], int(n_pts[f]))
            o["status"][f] = st
            for b, r in enumerate(res):
                for k in ("tracked", "source", "n_used", "rms", "hits", "missed"):
                    o[k][f, b] = r[k]
                o["assign"][f, b] = r["assign"]
                o["R"][f, b] = np.array(r["R"]).reshape(3, 3)
                o["t"][f, b] = r["t"]
        return o

    def margins_ok(self):
        return all(v > MARGIN for v in self.margin.values())


def search_labels(xyz, n_pts, bodies, tol, max_rms):
    """The per-frame search alone over a batch: -> found [F][B], assign [F][B][8] (what mocap_locate_rigid_bodies writes)."""
    models = [b if isinstance(b, Model) else Model(b) for b in bodies]
    F = len(n_pts)
    found = np.zeros((F, len(models)), dtype=np.int32)
    assign = np.zeros((F, len(models), MAX_MARKERS), dtype=np.int8)
    for f in range(F):
        for b, r in enumerate(locate(xyz[f], int(n_pts[f]), models, tol, max_rms, with_runner_up=False)):
            found[f, b] = r["found"]
            assign[f, b] = r["assign"]
    return found, assign


# ---------------------------------------------------------------- bodies and scenes
def symmetric_body(side=0.2, apex=0.1):
    """A square of edge `side` in the plane z = 0 plus an apex above its centre: four labellings a quarter turn apart fit equally."""
    h = side / 2
    return np.array([[h, h, 0.0], [-h, h, 0.0], [-h, -h, 0.0], [h, -h, 0.0], [0.0, 0.0, apex]])


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def path_scene(rng, bodies, F, K_max, n_clutter, paths, visible=None, noise=0.0005, rate=60.0, cube=2.0, t0=100.0):
    """bodies on smooth paths at `rate` Hz.  paths[b] = (centre [3], amplitude [3], angular frequency rad/s, phase, rotation axis
    [3], degrees turned per frame).  visible: None or bool [F][B][N].  Every frame: the visible markers with Gaussian noise,
    n_clutter uniform points in a cube, shuffled.  -> t [F], xyz [F][K_max][3] (NaN beyond n), n_pts [F],
    truth = {"R" [F][B][3][3], "p" [F][B][3], "assign" [F][B][8]}."""
    B = len(bodies)
    t = t0 + np.arange(F) / rate
    xyz = np.full((F, K_max, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    truth = {"R": np.zeros((F, B, 3, 3)), "p": np.zeros((F, B, 3)), "assign": np.full((F, B, MAX_MARKERS), -1, dtype=np.int64)}
    for f in range(F):
        pts, owner = [], []
        for b, q in enumerate(bodies):
            q = np.asarray(q, dtype=np.float64)
            c, amp, w, ph, axis, deg = paths[b]
            s = (t[f] - t0) * w + ph
            p = np.asarray(c, dtype=np.float64) + np.asarray(amp) * np.array([math.sin(s), math.cos(s), math.sin(2 * s)])
            R = _rot(axis, math.radians(deg) * f)
            truth["R"][f, b], truth["p"][f, b] = R, p
            for m in range(q.shape[0]):
                if visible is None or visible[f][b][m]:
                    pts.append(R @ q[m] + p + rng.normal(0.0, noise, 3))
                    owner.append((b, m))
        for _ in range(n_clutter):
            pts.append(rng.uniform(-cube / 2, cube / 2, 3))
            owner.append(None)
        n = len(pts)
        assert n <= K_max, (n, K_max)
        for slot, src in enumerate(rng.permutation(n)):
            xyz[f, slot] = pts[src]
            if owner[src] is not None:
                truth["assign"][f, owner[src][0], owner[src][1]] = slot
        n_pts[f] = n
    return t, xyz, n_pts, truth


def two_identical_scene(rng, body, F, K_max, n_clutter, gap=0.15, speed=0.6, noise=0.0005, rate=60.0):
    """Two copies of one body on straight lines in opposite directions along x, `gap` apart in y, passing each other at mid-session."""
    t0 = 100.0
    t = t0 + np.arange(F) / rate
    xyz = np.full((F, K_max, 3), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    q = np.asarray(body, dtype=np.float64)
    truth = {"R": np.zeros((F, 2, 3, 3)), "p": np.zeros((F, 2, 3)), "assign": np.full((F, 2, MAX_MARKERS), -1, dtype=np.int64)}
    half = (F - 1) / 2 / rate
    for f in range(F):
        pts, owner = [], []
        for b in range(2):
            sgn = 1.0 if b == 0 else -1.0
            p = np.array([sgn * speed * ((t[f] - t0) - half), b * gap, 0.0])
            R = _rot([0.2, 0.3, 1.0], math.radians(1.0) * f * sgn)
            truth["R"][f, b], truth["p"][f, b] = R, p
            for m in range(q.shape[0]):
                pts.append(R @ q[m] + p + rng.normal(0.0, noise, 3))
                owner.append((b, m))
        for _ in range(n_clutter):
            pts.append(rng.uniform(-1.0, 1.0, 3))
            owner.append(None)
        n = len(pts)
        assert n <= K_max, (n, K_max)
        for slot, src in enumerate(rng.permutation(n)):
            xyz[f, slot] = pts[src]
            if owner[src] is not None:
                truth["assign"][f, owner[src][0], owner[src][1]] = slot
        n_pts[f] = n
    return t, xyz, n_pts, truth


def labelling(assign_f, truth_f, N):
    """The marker each assigned marker's point truly belongs to: tuple of N entries (-1 = unassigned or a foreign point) -- equal
    tuples in two frames = the same labelling, whatever the frames' shuffles."""
    inv = {int(slot): m for m, slot in enumerate(truth_f[:N]) if slot >= 0}
    return tuple(inv.get(int(assign_f[m]), -1) if assign_f[m] >= 0 else -1 for m in range(N))


# ---------------------------------------------------------------- the scenes of the GPU tests (tests/test_gpu_body_track.py)
# Each is checked on this reference first (tests/test_body_track_reference_cpu.py): the margins of Tracker.margins_ok() and
# what the scene is there to show.  A scene that fails is rebuilt with another seed, not exempted.
TOL, MAX_RMS = 0.01, 0.005
_PATHS = [((0.1, -0.2, 0.8), (0.3, 0.25, 0.1), 2.0, 0.0, (0.0, 0.0, 1.0), 3.0),
          ((-0.5, 0.4, 1.2), (0.2, 0.3, 0.15), 1.5, 1.0, (1.0, 0.2, 0.1), 2.0),
          ((0.6, 0.5, 0.4), (0.15, 0.2, 0.1), 2.5, 2.0, (0.3, 1.0, 0.2), -2.5)]


def _scene(name):
    """-> {"bodies", "K_max", "settings": (gate, max_missed, vel_alpha), "t", "xyz", "n_pts", "truth"}"""
    if name == "planted1":
        rng = np.random.default_rng(101)
        bodies = [make_body(rng, 5)]
        vis = rng.uniform(size=(60, 1, 8)) < 0.85
        s = path_scene(rng, bodies, 60, 16, 6, _PATHS[:1], visible=vis)
        K, st = 16, (0.03, 10, 0.5)
    elif name == "planted3":
        rng = np.random.default_rng(202)
        bodies = [make_body(rng, 4), make_body(rng, 6), make_body(rng, 8)]
        vis = rng.uniform(size=(60, 3, 8)) < 0.9
        s = path_scene(rng, bodies, 60, 32, 8, _PATHS, visible=vis)
        K, st = 32, (0.03, 10, 0.5)
    elif name == "symmetric":
        rng = np.random.default_rng(312)   # (a seed at which the per-frame search finds the body in frame 0: 120 frames tracked)
        bodies = [symmetric_body()]
        s = path_scene(rng, bodies, 120, 16, 10, _PATHS[:1])
        K, st = 16, (0.03, 10, 0.5)
    elif name == "occlusion":
        rng = np.random.default_rng(404)
        bodies = [make_body(rng, 5)]
        vis = np.ones((60, 1, 8), dtype=bool)
        vis[20:29, 0, 2:] = False          # two markers for nine frames: max_missed = 5 of them coast, four have nothing
        s = path_scene(rng, bodies, 60, 16, 6, _PATHS[:1], visible=vis)
        K, st = 16, (0.03, 5, 0.5)
    elif name == "identical":
        rng = np.random.default_rng(505)
        body = make_body(rng, 5, size=0.12, min_sep=0.04)
        bodies = [body, body]
        s = two_identical_scene(rng, body, 90, 32, 6)
        K, st = 32, (0.03, 10, 0.5)
    elif name == "full64":
        rng = np.random.default_rng(606)
        bodies = [make_body(rng, 8), make_body(rng, 5)]
        s = path_scene(rng, bodies, 20, 64, 51, _PATHS[:2])
        K, st = 64, (0.03, 10, 0.5)
    elif name == "eight":
        rng = np.random.default_rng(707)
        bodies = [make_body(rng, 3 + (b % 2), size=0.2 + 0.03 * b) for b in range(8)]
        paths = [((-0.8 + 0.22 * b, 0.5 * (b % 3) - 0.5, 0.3 + 0.1 * b), (0.05, 0.05, 0.02), 2.0, 0.3 * b, (0.1 * b, 0.2, 1.0), 2.0)
                 for b in range(8)]
        s = path_scene(rng, bodies, 12, 32, 4, paths)
        K, st = 32, (0.03, 10, 0.5)
    else:
        raise KeyError(name)
    return {"bodies": bodies, "K_max": K, "settings": st, "t": s[0], "xyz": s[1], "n_pts": s[2], "truth": s[3]}


SCENES = ("planted1", "planted3", "symmetric", "occlusion", "identical", "full64", "eight")
_cache = {}


def scene(name):
    """The scene and the reference's results for it, computed once per process and shared: treat both as read-only."""
    if name not in _cache:
        s = _scene(name)
        trk = Tracker(s["bodies"], TOL, MAX_RMS, *s["settings"])
        s["ref"] = trk.run(s["t"], s["xyz"], s["n_pts"])
        s["ref_state"] = trk.state()
        s["margin"] = dict(trk.margin)
        s["margins_ok"] = trk.margins_ok()
        _cache[name] = s
    return _cache[name]
