"""The "marker tracker" section of include/mocap_core.h in plain NumPy / Python: a sorted pair list and a sequential loop,
nothing of the kernel's structure.  Every operation is one IEEE double operation (NumPy's elementwise ufuncs and Python's float
arithmetic do not fuse), in the order the header writes it, so ids, hits, counts, status AND the state's doubles are compared
with the device bit for bit.  Also the scene generators the tests share, and the mutual-best-rounds statement of step 3 that
tests/test_marker_track_reference_cpu.py holds against the sorted one."""
import numpy as np

MAX_TRACKS, MAX_POINTS = 64, 64
ST_FULL, ST_BAD_TIME = 1, 2
DEFAULTS = dict(gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64)


def validate(gate, max_missed, vel_alpha, T_max):
    """None when mocap_set_marker_tracker accepts the settings (T_max >= 1), else the reason."""
    if not 1 <= T_max <= MAX_TRACKS:
        return "T_max outside 1 .. 64"
    if not (np.isfinite(gate) and gate > 0):
        return "gate must be finite and > 0"
    if max_missed < 0:
        return "max_missed < 0"
    if not 0.0 <= vel_alpha <= 1.0:
        return "vel_alpha outside [0, 1]"
    return None


def pair_d2(pred, pts):
    """d2 [slot][point]: d = x_j - pred_i, dx dx + dy dy + dz dz summed in x, y, z order."""
    with np.errstate(all="ignore"):
        d = pts[None, :, :] - pred[:, None, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def associate_sorted(d2, live, fin, g2):
    """Step 3 as written: the admissible pairs in ascending (d2, slot, point) order, committed when both are free."""
    pairs = sorted((float(d2[i, j]), int(i), int(j)) for i in np.flatnonzero(live) for j in np.flatnonzero(fin) if d2[i, j] < g2)
    slot_of, point_of = {}, {}
    for _, i, j in pairs:
        if i not in point_of and j not in slot_of:
            point_of[i] = j
            slot_of[j] = i
    return point_of, 0


def associate_rounds(d2, live, fin, g2):
    """Step 3 as the kernel evaluates it: rounds of "commit every pair that is both its track's best free point by (d2, j) and its
    point's best free track by (d2, i)".  Returns the same dict and the number of rounds that committed something."""
    free_t, free_p = set(map(int, np.flatnonzero(live))), set(map(int, np.flatnonzero(fin)))
    point_of, rounds = {}, 0
    while free_t and free_p:
        best_p = {i: min(((float(d2[i, j]), j) for j in free_p if d2[i, j] < g2), default=None) for i in free_t}
        best_t = {j: min(((float(d2[i, j]), i) for i in free_t if d2[i, j] < g2), default=None) for j in free_p}
        commit = [(i, bp[1]) for i, bp in best_p.items() if bp is not None and best_t[bp[1]][1] == i]
        if not commit:
            break
        rounds += 1
        for i, j in commit:
            point_of[i] = j
            free_t.discard(i)
            free_p.discard(j)
    return point_of, rounds


class Tracker:
    def __init__(self, gate=0.05, max_missed=5, vel_alpha=0.5, T_max=64, associate=associate_sorted):
        assert validate(gate, max_missed, vel_alpha, T_max) is None
        self.g2 = float(gate) * float(gate)
        self.max_missed, self.alpha, self.T, self.associate = int(max_missed), float(vel_alpha), int(T_max), associate
        self.rounds = []          # per frame, when `associate` counts them
        self.reset()

    def reset(self):
        T = self.T
        self.live = np.zeros(T, dtype=bool)
        self.id = np.zeros(T, dtype=np.int32)
        self.p, self.v = np.zeros((T, 3)), np.zeros((T, 3))
        self.t_seen = np.zeros(T)
        self.missed, self.hits = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
        self.next_id = 0

    def step(self, t, pts, n):
        """One frame: pts [K_max][3], n points -> (id [K_max], hits [K_max], n_tracks, status)."""
        pts = np.asarray(pts, dtype=np.float64)
        K = pts.shape[0]
        out_id, out_hits = np.full(K, -1, dtype=np.int32), np.zeros(K, dtype=np.int32)
        t = float(t)
        if not np.isfinite(t):
            return out_id, out_hits, 0, ST_BAD_TIME
        n = int(n) if 0 <= int(n) <= K else 0
        fin = np.zeros(K, dtype=bool)
        fin[:n] = np.isfinite(pts[:n]).all(axis=1)
        # 1. prediction
        with np.errstate(all="ignore"):
            dt = t - self.t_seen
            pred = np.where((dt > 0)[:, None], self.p + self.v * dt[:, None], self.p)
        # 2.-3. admissible pairs, association
        point_of, rounds = self.associate(pair_d2(pred, pts), self.live, fin, self.g2)
        self.rounds.append(rounds)
        # 4.-5. matched and unmatched live slots
        for i in np.flatnonzero(self.live):
            if i in point_of:
                x = pts[point_of[i]]
                if dt[i] > 0:
                    u = (x - self.p[i]) / dt[i]
                    self.v[i] = self.v[i] + self.alpha * (u - self.v[i])
                self.p[i] = x
                self.t_seen[i] = t
                self.missed[i] = 0
                self.hits[i] += 1
                out_id[point_of[i]], out_hits[point_of[i]] = self.id[i], self.hits[i]
            else:
                self.missed[i] += 1
                if self.missed[i] > self.max_missed:
                    self.live[i] = False
        # 6. births
        status, taken = 0, set(point_of.values())
        for j in np.flatnonzero(fin):
            if j in taken:
                continue
            free = np.flatnonzero(~self.live)
            if free.size == 0:
                status |= ST_FULL
                continue
            i = free[0]
            self.live[i], self.id[i] = True, self.next_id
            self.next_id += 1
            self.p[i], self.v[i], self.t_seen[i], self.missed[i], self.hits[i] = pts[j], 0.0, t, 0, 1
            out_id[j], out_hits[j] = self.id[i], 1
        return out_id, out_hits, int(self.live.sum()), status

    def run(self, t, xyz, n_pts):
        """Consecutive frames -> the dict MocapCore.track_markers returns."""
        F, K = len(t), np.asarray(xyz).shape[1]
        o = {"id": np.full((F, K), -1, dtype=np.int32), "hits": np.zeros((F, K), dtype=np.int32),
             "n_tracks": np.zeros(F, dtype=np.int32), "mk_status": np.zeros(F, dtype=np.int32)}
        for f in range(F):
            o["id"][f], o["hits"][f], o["n_tracks"][f], o["mk_status"][f] = self.step(t[f], xyz[f], n_pts[f])
        return o

    def tracks(self):
        """The live slots in slot order -> the dict MocapCore.marker_tracks returns."""
        s = np.flatnonzero(self.live)
        return {"id": self.id[s].copy(), "pos": self.p[s].copy(), "vel": self.v[s].copy(), "t_seen": self.t_seen[s].copy(),
                "missed": self.missed[s].copy(), "hits": self.hits[s].copy()}

    def slots(self):
        return np.flatnonzero(self.live)


# ---------------------------------------------------------------------------------------------------------------- scenes
def planted_scene(markers, K_max, clutter, seed, n_frames=96, rate=60.0, t0=100.0, noise=0.0005):
    """`markers` markers on smooth paths (< 0.6 m/s, >= 0.12 m apart at all times: nodes of a 0.3 m grid, each circling its node
    within 0.05 m per axis), `noise` m of Gaussian noise, occlusions of 1-4 frames, `clutter` one-frame points per frame at least
    0.12 m from every marker, the point order shuffled per frame.  Returns t [F], xyz [F][K_max][3] (unused slots hold a value
    that must never be read as a point: 1e6), n_pts [F], truth [F][K_max] (marker index, -1 = clutter or unused)."""
    assert markers + clutter <= K_max
    rng = np.random.default_rng(seed)
    side = int(np.ceil(markers ** (1 / 3)))
    nodes = np.array([[a, b, c] for a in range(side) for b in range(side) for c in range(side)], dtype=np.float64)
    nodes = nodes[rng.permutation(len(nodes))[:markers]] * 0.3
    w = rng.uniform(2.0, 6.0, size=(markers, 3))          # rad/s: speed <= 0.05 * 6 * sqrt(3) = 0.52 m/s
    ph = rng.uniform(0, 2 * np.pi, size=(markers, 3))
    t = t0 + np.arange(n_frames) / rate
    pos = nodes[None] + 0.05 * np.sin(w[None] * (t - t0)[:, None, None] + ph[None])     # [F][markers][3]
    speed = np.linalg.norm(0.05 * w[None] * np.cos(w[None] * (t - t0)[:, None, None] + ph[None]), axis=2)
    assert speed.max() < 0.6
    for f in range(n_frames):
        d = np.linalg.norm(pos[f][:, None] - pos[f][None], axis=2) + np.eye(markers)
        assert d.min() >= 0.12
    hidden = np.zeros((n_frames, markers), dtype=bool)
    for m in range(markers):
        f = int(rng.integers(4, 12))
        while f < n_frames - 6:
            L = int(rng.integers(1, 5))
            hidden[f:f + L, m] = True
            f += L + int(rng.integers(8, 30))
    lo, hi = nodes.min(axis=0) - 0.3, nodes.max(axis=0) + 0.3
    xyz = np.full((n_frames, K_max, 3), 1e6)
    truth = np.full((n_frames, K_max), -1, dtype=np.int32)
    n_pts = np.zeros(n_frames, dtype=np.int32)
    for f in range(n_frames):
        pts, lab = [], []
        for m in range(markers):
            if not hidden[f, m]:
                pts.append(pos[f, m] + rng.normal(0, noise, 3))
                lab.append(m)
        k = 0
        while k < clutter:
            c = rng.uniform(lo, hi)
            if np.linalg.norm(pos[f] - c, axis=1).min() >= 0.12:
                pts.append(c)
                lab.append(-1)
                k += 1
        order = rng.permutation(len(pts))
        n_pts[f] = len(pts)
        xyz[f, :len(pts)] = np.array(pts)[order]
        truth[f, :len(pts)] = np.array(lab)[order]
    return t, xyz, n_pts, truth


def id_switches(ids, truth):
    """Number of planted markers whose id is not one value over every frame they are seen in."""
    bad = 0
    for m in range(int(truth.max()) + 1):
        seen = ids[truth == m]
        bad += int(seen.size > 0 and (seen.min() < 0 or seen.min() != seen.max()))
    return bad


def crossing_scene(n_frames=22, rate=60.0, t0=100.0):
    """Two markers at (x, 0, 1) and (-x, 0.01, 1), x = -0.42 + 0.04 f: they pass each other 0.01 m apart."""
    t = t0 + np.arange(n_frames) / rate
    xyz = np.zeros((n_frames, 2, 3))
    for f in range(n_frames):
        x = -0.42 + 0.04 * f
        xyz[f] = [[x, 0.0, 1.0], [-x, 0.01, 1.0]]
    return t, xyz, np.full(n_frames, 2, dtype=np.int32)


def crowded_scene(n_points, K_max, seed, n_frames=24, rate=60.0, t0=100.0, box=0.12):
    """Points that jump about inside a box no larger than a few gates, a varying number per frame: nearly every track has several
    admissible points and nearly every point several admissible tracks, so the association needs many rounds; one point in
    eight repeats another exactly (equal d2: the index decides)."""
    rng = np.random.default_rng(seed)
    t = t0 + np.arange(n_frames) / rate
    xyz = np.full((n_frames, K_max, 3), 1e6)
    n_pts = rng.integers(max(1, n_points // 2), n_points + 1, size=n_frames).astype(np.int32)
    for f in range(n_frames):
        p = rng.uniform(0, box, size=(n_pts[f], 3))
        for j in range(1, n_pts[f]):
            if rng.random() < 0.125:
                p[j] = p[rng.integers(0, j)]
        xyz[f, :n_pts[f]] = p
    return t, xyz, n_pts
