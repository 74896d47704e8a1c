"""Constructed frames for the object locator (reference helpers.py:424-480), plain NumPy.

The locator is a chain of yes/no decisions; seeded drone triangles in sparse clutter never come near one.  The builders
here put frames ON the decisions: adjacent doubles on either side of each threshold, the same triangles translated so that
the last bit of the distance decides, points shared by two objects, leads skipped because they were matched as base points,
members on both sides of the 64-point chunk edges of the wave search, dense clutter with leads in every 64-bit word of
`matched[]`, non-finite points and out-of-range counts.

Every builder returns a case set: {"name", "xyz" [F][K_max][3], "err" [F][K_max], "n_pts" [F], "labels" [F]} (NaN beyond
each frame's points).  What a frame SHOULD give never comes from the device: statement() runs
oracle.mocap_oracle.locate_objects one frame at a time, and tests/golden/locate_edges.npz holds what the reference's
own function returned for the same inputs (oracle/make_golden.py, golden_locate_edges).
"""
import itertools

import numpy as np

H_TRI = np.sqrt(0.095 ** 2 - 0.075 ** 2)       # height of the 0.095 / 0.095 / 0.15 triangle

# threshold -> (last double inside, first double outside); lead at the origin and the other point on a coordinate axis, so
# that sqrt(x * x) == |x| exactly and the doubles themselves meet `|d - 0.095| < 0.025` / `|d - 0.15| > 0.025`
EDGES = {
    "lead_lower": (0.07, np.nextafter(0.07, 0)),
    "lead_upper": (0.12, np.nextafter(0.12, 1)),
    "pair_upper": (0.0875, np.nextafter(0.0875, 1)),     # pair at +-d: distance 2 d = 0.175
    "pair_lower": (0.0625, np.nextafter(0.0625, 0)),     # pair at +-d: distance 2 d = 0.125
}
CHUNK_K = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 256)
DENSE_SEEDS = {63: 5, 64: 5, 65: 5, 129: 4, 256: 5}      # 24 frames in all
DENSE_RECORDED = {63: 2, 64: 3, 65: 2, 129: 2, 256: 3}   # the 12 of them the golden holds
WAVE_GRID = 4096                                         # workgroups of the wave search, frames beyond walk in this stride


def edge_triangle(edge, d):
    """[lead, p1, p2] in the plane (u, v) of the edge's axis and the next one."""
    if edge == "lead_lower":
        return [(0.0, 0.0), (-0.075, 0.0), (d, 0.0)]
    if edge == "lead_upper":       # not collinear (0.07 + 0.12 > 0.175): pair distance sqrt(0.09^2 + 0.12^2) = 0.15
        return [(0.0, 0.0), (0.0, 0.09), (d, 0.0)]
    if edge == "pair_upper":
        return [(0.0, 0.0), (-d, 0.0), (d, 0.0)]
    if edge == "pair_lower":       # 0.0625 is below the lead gate: the lead sits off the pair's axis
        return [(0.0, 0.07), (-d, 0.0), (d, 0.0)]
    raise KeyError(edge)


def embed(uv, axis):
    p = np.zeros((len(uv), 3))
    for k, (u, v) in enumerate(uv):
        p[k, axis] = u
        p[k, (axis + 1) % 3] = v
    return p


def pack(name, frames, k_max):
    """frames: [(points [n][3], err [n], label)] or [(points, err, label, n_pts)] with an explicit count."""
    F = len(frames)
    xyz = np.full((F, k_max, 3), np.nan)
    err = np.full((F, k_max), np.nan)
    n_pts = np.zeros(F, dtype=np.int32)
    labels = []
    for f, fr in enumerate(frames):
        p, e, label = np.asarray(fr[0], dtype=np.float64).reshape(-1, 3), np.asarray(fr[1], dtype=np.float64), fr[2]
        assert p.shape[0] == e.shape[0] <= k_max, label
        xyz[f, :p.shape[0]] = p
        err[f, :p.shape[0]] = e
        n_pts[f] = fr[3] if len(fr) > 3 else p.shape[0]
        labels.append(label)
    return {"name": name, "xyz": xyz, "err": err, "n_pts": n_pts, "labels": labels}


def effective_n(n_pts, k_max):
    """A count outside 0 .. K_max means no valid slot (include/mocap_core.h, mocap_locate_objects)."""
    n = np.asarray(n_pts).astype(np.int64)
    return np.where((n < 0) | (n > k_max), 0, n)


# ----------------------------------------------------------------------------- the families
def exact_edges():
    rng = np.random.default_rng(101)
    frames = []
    for edge, (inside, outside) in EDGES.items():
        for side, d in (("inside", inside), ("outside", outside)):
            for axis in range(3):
                tri = embed(edge_triangle(edge, d), axis)
                for order in itertools.permutations(range(3)):
                    frames.append((tri[list(order)], rng.random(3), f"{edge}/{side}/axis{axis}/order{''.join(map(str, order))}"))
    return pack("exact", frames, 3)


def shifted_edges(n_offsets=200):
    rng = np.random.default_rng(202)
    frames = []
    for edge, (inside, _) in EDGES.items():
        tri = embed(edge_triangle(edge, inside), 0)
        for k, off in enumerate(rng.uniform(-2, 2, (n_offsets, 3))):
            frames.append((tri + off, rng.random(3), f"{edge}/shift{k}"))
    return pack("shifted", frames, 3)


def turned_edges(n_poses=100):
    """The same four triangles in seeded random poses (an orthonormal pair for the plane, an offset in [-2, 2]^3): every
    coordinate difference is inexact, so the decisive distance lands a few ulps either side of its threshold.  (A pure
    translation leaves the difference along the axis a function of the offset's binade alone, and the other two exactly zero.)"""
    rng = np.random.default_rng(707)
    frames = []
    for edge, (inside, _) in EDGES.items():
        uv = np.array(edge_triangle(edge, inside))
        for k in range(n_poses):
            u = rng.normal(0, 1, 3)
            u /= np.linalg.norm(u)
            v = np.cross(u, rng.normal(0, 1, 3))
            v /= np.linalg.norm(v)
            tri = rng.uniform(-2, 2, 3) + uv[:, :1] * u + uv[:, 1:] * v
            frames.append((tri[rng.permutation(3)], rng.random(3), f"{edge}/pose{k}"))
    return pack("turned", frames, 3)


DIAMOND = np.array([[-0.075, 0, 0], [0.075, 0, 0], [0, H_TRI, 0], [0, -H_TRI, 0]])   # base pair, a lead on each side


def skip_points():
    """[L1, A, B, C, D]: L1 leads (A, B); A itself leads (C, D).  With L1 first A is matched as a base point and skipped."""
    A, B, L1 = DIAMOND[0], DIAMOND[1], DIAMOND[2]
    C = A + np.array([-H_TRI, 0, 0.075])
    D = A + np.array([-H_TRI, 0, -0.075])
    return np.array([L1, A, B, C, D])


def fan_points():
    """Lead at the origin, five points 0.095 away in the xy-plane at 0, 10, 20, 60 and 60 + 104.27 degrees (chord 0.15 with the
    60-degree one only): the rows of the first three fail in full before (60, 164.27) is met."""
    ang = np.radians([0, 10, 20, 60, 60 + np.degrees(2 * np.arcsin(0.15 / 0.19))])
    return np.vstack([np.zeros((1, 3)), 0.095 * np.stack([np.cos(ang), np.sin(ang), np.zeros(5)], axis=1)])


def sharing():
    rng = np.random.default_rng(303)
    frames = []
    for order in itertools.permutations(range(4)):
        frames.append((DIAMOND[list(order)], rng.random(4), f"diamond/order{''.join(map(str, order))}"))
    sk = skip_points()
    for tag, order in (("lead_first", (0, 1, 2, 3, 4)), ("base_first", (1, 0, 2, 3, 4)), ("pair_first", (3, 4, 2, 1, 0)),
                       ("lead_last", (1, 2, 3, 4, 0))):
        frames.append((sk[list(order)], rng.random(5), f"skip/{tag}"))
    fan = fan_points()
    frames.append((fan, rng.random(6), "fan/order012345"))
    for _ in range(5):
        order = rng.permutation(6)
        frames.append((fan[order], rng.random(6), f"fan/order{''.join(map(str, order))}"))
    return pack("sharing", frames, 6)


def clutter_grid(n, origin=10.0, step=0.5):
    """n points on a grid `step` apart, far from everything planted near the origin: nothing here matches anything."""
    i = np.arange(n)
    return origin + step * np.stack([i % 7, (i // 7) % 7, i // 49], axis=1).astype(np.float64)


def posed_triangle(rng, centre):
    """[lead, p1, p2] of a 0.095 / 0.095 / 0.15 triangle in a random pose."""
    u = rng.normal(0, 1, 3)
    u /= np.linalg.norm(u)
    w = np.cross(u, rng.normal(0, 1, 3))
    w /= np.linalg.norm(w)
    c = np.asarray(centre, dtype=np.float64)
    return np.array([c + H_TRI * w, c + 0.075 * u, c - 0.075 * u])


def chunk_triples(K):
    """(lead, p1, p2) index triples with members on both sides of 64 / 128 / 192 and at the ends of the frame."""
    cand = [(63, 64, 255), (200, 0, 64), (64, 63, 128), (127, 128, 192), (192, 191, 0), (128, 255, 127), (0, 1, 2),
            (K - 1, 0, K // 2), (0, K - 1, K - 2), (K - 2, K - 1, 0)]
    out = []
    for t in cand:
        if min(t) >= 0 and max(t) < K and len(set(t)) == 3 and t not in out:
            out.append(t)
    return out


def chunk_edges():
    rng = np.random.default_rng(404)
    frames = []

    def planted(K, plants, label):
        """plants: [(indices, points)]; every other slot is far clutter."""
        p = clutter_grid(K)
        for idx, pts in plants:
            p[list(idx)] = pts
        frames.append((p, rng.random(K), label))

    for K in CHUNK_K:
        if K == 1:
            planted(1, [], "chunk/K1/clutter")
            continue
        if K == 2:
            planted(2, [((0, 1), posed_triangle(rng, (0, 0, 0))[:2])], "chunk/K2/two_of_three")
            continue
        triples = chunk_triples(K)
        for t in triples:
            planted(K, [(t, posed_triangle(rng, (0, 0, 0)))], f"chunk/K{K}/tri{t[0]}_{t[1]}_{t[2]}")
        if K < 63:
            continue
        # several at once, each 3 m from the next: greedy choice of triples with no index in common
        used, plants = set(), []
        for t in triples:
            if not used & set(t):
                used |= set(t)
                plants.append((t, posed_triangle(rng, (3.0 * len(plants), 0, 0))))
        planted(K, plants, f"chunk/K{K}/together{len(plants)}")
        if K >= 193:
            planted(K, [((63, 64, 128, 192), DIAMOND)], f"chunk/K{K}/diamond_base63_64_leads128_192")
            planted(K, [((128, 192, 63, 64), DIAMOND)], f"chunk/K{K}/diamond_base128_192_leads63_64")
        if K == 256:
            fan = fan_points()
            planted(K, [((130, 5, 70, 140, 200, 255), fan)], "chunk/K256/fan_lead130_rows5_70_140_pair200_255")
            planted(K, [((130, 64, 127, 128, 3, 250), fan)], "chunk/K256/fan_lead130_rows64_127_128_pair3_250")
    return pack("chunk", frames, 256)


def dense():
    frames = []
    for K, seeds in DENSE_SEEDS.items():
        for s in range(seeds):
            rng = np.random.default_rng(1000 * K + s)
            frames.append((rng.uniform(0, 0.4, (K, 3)), rng.random(K), f"dense/K{K}/seed{s}"))
    return pack("dense", frames, 256)


def dense_recorded(cs):
    """Indices of the dense frames the golden holds."""
    keep = []
    for f, label in enumerate(cs["labels"]):
        _, k, s = label.split("/")
        if int(s[4:]) < DENSE_RECORDED[int(k[1:])]:
            keep.append(f)
    return np.array(keep)


def nonfinite():
    rng = np.random.default_rng(505)
    tri = posed_triangle(rng, (0.3, -0.2, 0.1))
    far = clutter_grid(5)
    nan, inf = np.nan, np.inf
    frames = []
    for name, val in (("nan", nan), ("pinf", inf), ("ninf", -inf)):
        for comp in range(3):
            bad = far[0].copy()
            bad[comp] = val
            frames.append((np.vstack([bad, tri, far[1]]), rng.random(5), f"clutter_{name}_{'xyz'[comp]}/before"))
            frames.append((np.vstack([tri, bad, far[1]]), rng.random(5), f"clutter_{name}_{'xyz'[comp]}/after"))
    frames.append((np.vstack([[nan, nan, nan], tri, [inf, -inf, nan]]), rng.random(5), "clutter_all_bad"))
    for member, k in (("lead", 0), ("p1", 1), ("p2", 2)):
        for comp in range(3):
            t = tri.copy()
            t[k, comp] = nan
            frames.append((np.vstack([t, far[:2]]), rng.random(5), f"{member}_nan_{'xyz'[comp]}"))
    t = tri.copy()
    t[0, 1] = inf
    frames.append((np.vstack([t, far[:2]]), rng.random(5), "lead_pinf_y"))
    for member, k in (("lead", 0), ("p1", 1), ("p2", 2), ("clutter", 3)):
        e = rng.random(5)
        e[k] = nan
        frames.append((np.vstack([tri, far[:2]]), e, f"err_nan_{member}"))
    e = rng.random(5)
    e[0] = inf
    frames.append((np.vstack([tri, far[:2]]), e, "err_pinf_lead"))
    full = np.vstack([tri, far])                                        # K_max = 8 finite points, the triangle in slots 0 .. 2
    for n in (-1, 0, 1, 2, 3, 8, 9, 2 ** 31 - 1, -2 ** 31):
        frames.append((full, rng.random(8), f"n_pts/{n}", n))
    return pack("nonfinite", frames, 8)


FAMILIES = {"exact": exact_edges, "shifted": shifted_edges, "turned": turned_edges, "sharing": sharing, "chunk": chunk_edges, "dense": dense,
            "nonfinite": nonfinite}
CONSTRUCTED = ("exact", "shifted", "turned", "sharing", "chunk", "nonfinite")     # recorded in full; of "dense", 12 frames
_sets, _statements = {}, {}


def case_set(name):
    if name not in _sets:
        _sets[name] = FAMILIES[name]()
    return _sets[name]


def recorded():
    """[(family, case set, indices of its frames in tests/golden/locate_edges.npz)]."""
    out = [(name, case_set(name), np.arange(len(case_set(name)["labels"]))) for name in CONSTRUCTED]
    return out + [("dense", case_set("dense"), dense_recorded(case_set("dense")))]


# ----------------------------------------------------------------------------- what the frames should give
def statement(cs):
    """oracle.mocap_oracle.locate_objects per frame -> arrays: n_obj [F], and per object (O = the largest count, at least 1)
    lead [F][O], pair [F][O][2], droneIndex [F][O], pos [F][O][3], heading [F][O], error [F][O]; -1 / NaN beyond n_obj.
    Computed once per case set and shared; do not write into it."""
    if cs["name"] in _statements:
        return _statements[cs["name"]]
    from oracle import mocap_oracle as mo
    F, k_max = cs["err"].shape
    n = effective_n(cs["n_pts"], k_max)
    with np.errstate(invalid="ignore"):      # inf - inf among the non-finite points
        objs = [mo.locate_objects(cs["xyz"][f, :n[f]], cs["err"][f, :n[f]]) for f in range(F)]
    O = max(1, max(len(o) for o in objs))
    out = {"n_obj": np.array([len(o) for o in objs], dtype=np.int32),
           "lead": np.full((F, O), -1, dtype=np.int32), "pair": np.full((F, O, 2), -1, dtype=np.int32),
           "droneIndex": np.full((F, O), -1, dtype=np.int32), "pos": np.full((F, O, 3), np.nan),
           "heading": np.full((F, O), np.nan), "error": np.full((F, O), np.nan)}
    for f, fo in enumerate(objs):
        for j, o in enumerate(fo):
            out["lead"][f, j], out["pair"][f, j], out["droneIndex"][f, j] = o["lead"], o["pair"], o["droneIndex"]
            out["pos"][f, j], out["heading"][f, j], out["error"][f, j] = o["pos"], o["heading"], o["error"]
    for a in out.values():
        a.setflags(write=False)
    _statements[cs["name"]] = out
    return out


def lead_words(st, f):
    """Which 64-bit words of the searches' bit sets held a lead in frame f."""
    n = int(st["n_obj"][f])
    return sorted(set((st["lead"][f, :n] >> 6).tolist()))


# ----------------------------------------------------------------------------- pattern banks for the grid limits
def _take(cs, label):
    f = next(i for i, have in enumerate(cs["labels"]) if have.startswith(label))
    n = int(effective_n(cs["n_pts"], cs["err"].shape[1])[f])
    return cs["xyz"][f, :n], cs["err"][f, :n]


def grid_bank():
    """16 pattern frames, K_max 256.  Tiled with tile_index() the wave search meets, in ONE workgroup and one LDS copy, the
    dense 256-point frame (pattern 0), 4 096 frames later a 3-point triangle (pattern 1) and 4 096 later again a frame whose
    count is out of range (pattern 2)."""
    ex, sh, ch, de = case_set("exact"), case_set("sharing"), case_set("chunk"), case_set("dense")
    tri = _take(ex, "lead_upper/inside/axis0/order012")
    full = np.vstack([tri[0], clutter_grid(253)])
    frames = [
        _take(de, "dense/K256/seed0") + ("dense256",),
        tri + ("triangle3_after_dense",),
        (full, np.linspace(0.1, 0.9, 256), "count_257", 257),
        _take(sh, "diamond/order2031") + ("diamond",),
        _take(ex, "lead_lower/inside/axis1/order120") + ("lead_lower_inside",),
        _take(ex, "lead_lower/outside/axis1/order120") + ("lead_lower_outside",),
        _take(ex, "pair_upper/inside/axis1/order021") + ("pair_upper_inside_along_y",),
        _take(ex, "pair_upper/outside/axis1/order021") + ("pair_upper_outside",),
        _take(ch, "chunk/K256/tri63_64_255") + ("chunk63_64_255",),
        _take(ex, "pair_lower/inside/axis2/order201") + ("pair_lower_inside",),
        (full, np.linspace(0.9, 0.1, 256), "count_minus1", -1),
        _take(de, "dense/K65/seed0") + ("dense65",),
        _take(sh, "fan/order012345") + ("fan",),
        _take(ex, "pair_upper/inside/axis0/order210") + ("pair_upper_inside_along_x",),
        (np.zeros((0, 3)), np.zeros(0), "empty"),
        _take(ch, "chunk/K193/together") + ("chunk193_together",),
    ]
    return pack("grid_bank", frames, 256)


def small_bank():
    """Triangles and empties only, K_max 4: for the frame counts beyond the lane search's grid."""
    ex, sh = case_set("exact"), case_set("sharing")
    tri = _take(ex, "lead_upper/inside/axis0/order012")
    four = np.vstack([tri[0], [[5.0, 5.0, 5.0]]])
    frames = [
        tri + ("triangle",),
        (np.zeros((0, 3)), np.zeros(0), "empty"),
        _take(sh, "diamond/order0123") + ("diamond",),
        (four, np.array([0.1, 0.2, 0.3, 0.4]), "count_5", 5),
        _take(ex, "pair_lower/outside/axis2/order012") + ("pair_lower_outside",),
        _take(ex, "pair_upper/inside/axis1/order102") + ("pair_upper_inside_along_y",),
        (four, np.array([0.4, 0.3, 0.2, 0.1]), "count_minus1", -1),
        (four[:2], np.array([0.5, 0.6]), "two_points"),
        _take(sh, "diamond/order3120") + ("diamond_leads_first",),
        (four, np.array([0.7, 0.1, 0.2, 0.9]), "triangle_and_one"),
        _take(ex, "lead_lower/inside/axis0/order201") + ("lead_lower_inside",),
    ]
    return pack("small_bank", frames, 4)


FAMILIES.update(grid_bank=grid_bank, small_bank=small_bank)


def tile_index(F, n_patterns):
    """Pattern of frame f: one step on per 4 096 frames, so that the frames one workgroup of the wave search walks
    (f, f + 4 096, ...) run through the bank in order."""
    f = np.arange(F, dtype=np.int64)
    return (f + f // WAVE_GRID) % n_patterns


def tiled(bank, F):
    """bank tiled over F frames, each frame with an `err` of its own; the expected result from the bank's statement (once per
    pattern), its `error` recomputed per frame from the statement's lead and pair in the reference's order of additions."""
    st = statement(bank)
    idx = tile_index(F, bank["err"].shape[0])
    xyz, n_pts = bank["xyz"][idx], bank["n_pts"][idx]
    err = bank["err"][idx] + ((np.arange(F) % 4099) * 2.0 ** -12)[:, None]
    want = {k: st[k][idx] for k in ("n_obj", "lead", "pair", "droneIndex", "pos", "heading")}
    have = want["lead"] >= 0
    rows = np.arange(F)[:, None]
    e = lambda i: err[rows, np.where(have, i, 0)]          # noqa: E731
    want["error"] = np.where(have, ((e(want["lead"]) + e(want["pair"][..., 0])) + e(want["pair"][..., 1])) / 3, np.nan)
    return xyz, err, n_pts, want
