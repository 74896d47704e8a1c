"""Predicted precision on the GPU (include/mocap_core.h, "predicted precision"; kernels csrc/precision.hip): every integer exactly
and every double and float32 BIT FOR BIT against the statement (tests/precision_reference.py) -- points in the named and the
by-visibility form, the decision edges on a rig with integer intrinsics, the frame form chained behind the frame path, the
capture-volume map with its summary, and the bookkeeping: canaries around every output, optional outputs, every refusal, host = _dev
= second call = second stream, the helpers NumPy = resident = statement."""
import numpy as np
import pytest

import precision_reference as pr
from mocap_core import capi, helpers, synth

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
PAD = 64
KEYS = ("cov", "sig", "axis", "n_views", "info")


class Guarded:
    """A device array with PAD canary elements on either side (and the same value inside, so an untouched output shows too)."""
    FILL = {"float64": -12345.5, "float32": -12345.5, "int32": 0x5A5A5A5A, "uint8": 0xA5, "int64": 0x5A5A5A5A5A5A5A5A}

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.fill = self.FILL[str(dtype).split(".")[-1]]
        self.buf = torch.full((self.n + 2 * PAD,), self.fill, dtype=dtype, device="cuda:0")
        self.ptr = self.buf.data_ptr() + PAD * self.buf.element_size()

    def numpy(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy().reshape(self.shape)

    def intact(self, whole=False):
        b = self.buf.cpu().numpy()
        pads = np.concatenate([b[:PAD], b[PAD + self.n:]]) if not whole else b
        return bool((pads == b.dtype.type(self.fill)).all())


def _outs(shape, cov=True, axis=True):
    import torch
    g = {"sig": Guarded(shape + (3,), torch.float64), "n_views": Guarded(shape, torch.int32), "info": Guarded(shape, torch.int32)}
    if cov:
        g["cov"] = Guarded(shape + (6,), torch.float64)
    if axis:
        g["axis"] = Guarded(shape + (3,), torch.float64)
    return g


def _ptrs(g):
    return [g[k].ptr if k in g else 0 for k in KEYS]


def _same(got, want, keys=KEYS):
    for k in keys:
        if k in got and got[k] is not None:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k]).astype(got[k].dtype, copy=False).reshape(got[k].shape)
            assert a.tobytes() == b.tobytes(), (k, np.argwhere(a.view(np.uint8) != b.view(np.uint8))[:4], a.reshape(-1)[:6], b.reshape(-1)[:6])


def _rig(C, seed=3):
    rig = synth.calibrated_ring_rig(C, seed=seed)
    return rig, pr.camera_table(rig["K"], rig["R"], rig["t"])


def _set(core, rig):
    core.set_cameras(rig["K"], rig["R"], rig["t"])


def _points_dev(core, xyz, seen, image_size, near, far, sigma, frame, cov=True, axis=True):
    import torch
    N = len(xyz)
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    d_seen = None if seen is None else torch.from_numpy(np.ascontiguousarray(seen).view(np.int64)).cuda()
    g = _outs((N,), cov, axis)
    core.point_precision_dev(N, d_xyz.data_ptr(), 0 if seen is None else d_seen.data_ptr(), image_size, near, far, sigma, frame, *_ptrs(g))
    core.synchronize()
    assert all(v.intact() for v in g.values())
    return {k: v.numpy() for k, v in g.items()}


def _cloud(rig, N, rng):
    x = rig["centre"][None] + rng.uniform(-1.2, 1.2, (N, 3))
    if N > 8:
        x[3] = [0.0, 0.0, -2.0]          # behind camera 0
        x[5] = [40.0, -30.0, 1.0]        # outside most pictures
    return x


def _masks(C, N, rng):
    full = (1 << C) - 1
    m = rng.integers(0, full + 1, N, dtype=np.uint64) if C < 64 else rng.integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    m[::3] = full
    return m


@pytest.mark.parametrize("C", [2, 3, 8, 64])
def test_points_named_and_by_visibility_bit_for_bit(core, C):
    rig, P = _rig(C)
    _set(core, rig)
    rng = np.random.default_rng(50 + C)
    w, h = rig["image_size"]
    frame = np.concatenate([0.8 * np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], axis=1)
    ok = 0
    for N in (1, 63, 64, 65, 257):
        x = _cloud(rig, N, rng)
        seen = _masks(C, N, rng)
        for f, xs in ((None, x), (frame, (x - frame[:, 3]) @ np.linalg.inv(frame[:, :3]).T)):
            want = pr.point_precision(P, xs, seen=seen, sigma_px=0.7, frame=f)
            _same(core.point_precision(xs, seen, 0.7, frame=f), want)
            _same(_points_dev(core, xs, seen, None, 0.0, INF, 0.7, f), want)
            ok += int((want["info"] == pr.OK).sum())
            want = pr.point_precision(P, xs, image_size=(w, h), near=0.5, far=6.0, sigma_px=1.3, frame=f)
            _same(core.point_precision(xs, None, 1.3, (w, h), 0.5, 6.0, frame=f), want)
            _same(_points_dev(core, xs, None, (w, h), 0.5, 6.0, 1.3, f), want)
            ok += int((want["info"] == pr.OK).sum())
    assert ok > 400        # numbers were compared, not NaN alone


# ----------------------------------------------------------------------------- decision edges
def _edge_rig():
    """Integer intrinsics (f = 128, centre (64, 48), picture 128 x 96), three cameras: 0 at the origin looking along +z, 1 two units
    along +x looking the same way, 2 at (0, 0, 10) looking back along -z.  Projections of the crafted points are exact."""
    K = np.repeat(np.array([[128.0, 0, 64.0], [0, 128.0, 48.0], [0, 0, 1.0]])[None], 3, axis=0)
    R = np.stack([np.eye(3), np.eye(3), np.diag([-1.0, 1.0, -1.0])])
    t = np.array([[0.0, 0, 0], [-2.0, 0, 0], [0.0, 0, 10.0]])
    return {"K": K, "R": R, "t": t, "image_size": (128, 96)}


def test_decision_edges(core):
    rig = _edge_rig()
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    _set(core, rig)
    size = rig["image_size"]
    below = 2.0 - 2.0 ** -51          # 128 x + 256 = 512 - 2^-44 exactly; / 4 = 128 - 2^-46: one ulp below the width
    x = np.array([[-2.0, 0.0, 4.0],    # 0: pu == 0 in camera 0
                  [2.0, 0.0, 4.0],     # 1: pu == width in camera 0: not a view of it
                  [below, 0.0, 4.0],   # 2: pu one ulp below the width
                  [0.5, 0.25, 4.0],    # 3: plainly inside cameras 0, 1 and 2
                  [0.0, 0.0, 4.0]])    # 4: on the baseline of cameras 0 and 2
    vis = lambda near, far: (pr.point_precision(P, x, image_size=size, near=near, far=far), core.point_precision(x, None, 1.0, size, near, far),
                             _points_dev(core, x, None, size, near, far, 1.0, None))
    want, host, dev = vis(0.0, INF)
    _same(host, want), _same(dev, want)
    assert [int(s) & 1 for s in want["seen"]] == [1, 0, 1, 1, 1]                       # camera 0: the left edge is inside, the right edge is not
    assert int(want["n_views"][3]) == 3 and int(want["info"][3]) == pr.OK
    for near, far, cam0 in ((4.0, INF, 1), (0.0, 4.0, 1), (np.nextafter(4.0, INF), INF, 0), (0.0, np.nextafter(4.0, 0.0), 0)):   # w == near, w == far: views
        want, host, dev = vis(near, far)
        _same(host, want), _same(dev, want)
        assert int(want["seen"][3]) & 1 == cam0
    # named views
    big = 1e200
    pts = np.array([[0.5, 0.25, 12.0],   # 0: behind camera 2, which is named
                    [0.5, 0.25, 4.0],    # 1: one view
                    [0.5, 0.25, 4.0],    # 2: no view
                    [0.0, 0.0, 4.0],     # 3: two views, the point on their baseline
                    [NAN, 0.25, 4.0], [0.5, INF, 4.0], [0.5, 0.25, -INF], [big, 0.25, 4.0], [0.5, -big, 4.0], [0.5, 0.25, big],
                    [0.5, 0.25, 4.0],    # 10: bits at and above C are ignored
                    [0.5, 0.25, 4.0]])   # 11: the same point with the plain mask
    seen = np.array([5, 1, 0, 5, 7, 7, 7, 7, 7, 7, 0xFFFFFFFFFFFFFFFF, 7], dtype=np.uint64)
    want = pr.point_precision(P, pts, seen=seen)
    _same(core.point_precision(pts, seen), want)
    _same(_points_dev(core, pts, seen, None, 0.0, INF, 1.0, None), want)
    info = want["info"].tolist()
    assert info[0] == pr.BAD_VIEW and info[1] == pr.FEW_VIEWS and info[2] == pr.FEW_VIEWS and info[3] == pr.DEGENERATE
    assert all(i & pr.BAD_POINT for i in info[4:7]) and all(i != pr.OK for i in info[7:10])
    assert info[10] == info[11] == pr.OK and want["n_views"][10] == 3
    assert want["sig"][10].tobytes() == want["sig"][11].tobytes() and np.isnan(want["sig"][:10]).all()
    # the same odd points by visibility
    want = pr.point_precision(P, pts, image_size=size)
    _same(core.point_precision(pts, None, 1.0, size), want)
    _same(_points_dev(core, pts, None, size, 0.0, INF, 1.0, None), want)


# ----------------------------------------------------------------------------- frame form
def _frame_batch():
    rig = synth.ring_rig(8)
    blobs, counts, _ = synth.make_blob_stream(rig, 3, 16, seed=9)
    return rig, blobs, counts


def test_frame_form_chained_behind_the_frame_path(core):
    import torch
    rig, blobs, counts = _frame_batch()
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    _set(core, rig)
    F, C, M, _ = blobs.shape
    K = 32
    dev = "cuda:0"
    d_blobs, d_counts = torch.from_numpy(blobs).to(dev), torch.from_numpy(counts).to(dev)
    d_xyz = torch.full((F, K, 3), NAN, dtype=torch.float64, device=dev)
    d_err = torch.full((F, K), NAN, dtype=torch.float64, device=dev)
    d_corr = torch.full((F, K, C), -1, dtype=torch.int16, device=dev)
    d_n, d_st = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    g = _outs((F, K))
    torch.cuda.synchronize()
    core.match_triangulate_dev(F, M, d_blobs.data_ptr(), d_counts.data_ptr(), 5.0, K, 1 << 20, d_xyz.data_ptr(), d_err.data_ptr(),
                               d_corr.data_ptr(), d_n.data_ptr(), d_st.data_ptr())
    core.frame_precision_dev(F, K, d_xyz.data_ptr(), d_corr.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), 0.5, None, *_ptrs(g))   # (no synchronise between)
    core.synchronize()
    assert all(v.intact() for v in g.values())
    xyz, corr, n, st = d_xyz.cpu().numpy(), d_corr.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()
    assert (n >= 8).all() and not (st & pr.ST_SKIP).any()
    want = pr.frame_precision(P, xyz, corr, n, st, 0.5)
    _same({k: v.numpy() for k, v in g.items()}, want)
    assert (want["info"][0, :n[0]] == pr.OK).sum() >= 8 and (want["info"][0, n[0]:] == 0).all() and np.isnan(want["sig"][0, n[0]:]).all()
    _same(core.frame_precision(xyz, corr, n, st, 0.5), want)
    _same(core.frame_precision(xyz, corr, n, None, 0.5), want)
    # an overflow bit in a copied status, and a point count out of range: those frames are skipped
    st2, n2 = st.copy(), n.copy()
    st2[1] |= capi.ST_CAND_OVERFLOW
    n2[2] = K + 1
    want2 = pr.frame_precision(P, xyz, corr, n2, st2, 0.5)
    assert (want2["info"][1:] == 0).all() and (want2["n_views"][1:] == 0).all() and np.isnan(want2["cov"][1:]).all()
    _same(core.frame_precision(xyz, corr, n2, st2, 0.5), want2)
    n2[2] = -1
    _same(core.frame_precision(xyz, corr, n2, st2, 0.5), want2)


def test_frame_form_with_a_world_transform_through_the_helper(core):
    import torch
    rig, blobs, counts = _frame_batch()
    P = pr.camera_table(rig["K"], rig["R"], rig["t"])
    _set(core, rig)
    rng = np.random.default_rng(4)
    T = np.eye(4)
    T[:3, :3] = 1.9 * np.linalg.qr(rng.standard_normal((3, 3)))[0]
    T[:3, 3] = [0.3, -0.2, 1.1]
    T *= 2.0                                   # the last row is (0, 0, 0, 2)
    plain = core.match_triangulate(blobs, counts, K_max=32)
    helpers.set_core(core)
    try:
        helpers.set_to_world_coords_matrix(T)
        res = core.match_triangulate(blobs, counts, K_max=32)
        assert np.array_equal(res["n_out"], plain["n_out"]) and not np.allclose(res["xyz"][0, 0], plain["xyz"][0, 0])
        frame = helpers.precision_frame()
        assert np.allclose(frame, pr.world_frame(T), rtol=1e-12, atol=1e-12)
        want = pr.frame_precision(P, res["xyz"], res["corr"], res["n_out"], res["status"], 0.5, frame)
        got = helpers.frame_precision(res, sigma_px=0.5)
        _same(got, want)
        resident = {k: torch.from_numpy(res[k]).cuda() for k in ("xyz", "corr", "n_out", "status")}
        _same({k: v.cpu().numpy() for k, v in helpers.frame_precision(resident, sigma_px=0.5).items()}, want)
        # world units: the transform scales lengths by 3.8 / 2, and so every sig of the same points in camera-0 coordinates
        cam = pr.frame_precision(P, plain["xyz"], plain["corr"], plain["n_out"], plain["status"], 0.5)
        m = want["info"] == pr.OK
        assert m.sum() >= 24 and np.allclose(want["sig"][m], cam["sig"][m] * 1.9, rtol=1e-9)
        for bad in (np.diag([1.0, 1.0, 1.0, 0.0]), np.diag([1.0, 1.0, 0.0, 1.0]), np.eye(4) + np.eye(4)[[3, 0, 1, 2]] * 0.5):
            with pytest.raises(ValueError):
                helpers.precision_frame(bad)
    finally:
        helpers.set_to_world_coords_matrix(None)
        helpers.set_core(None)


# ----------------------------------------------------------------------------- the map
def _map_dev(core, shape, grid, size, near, far, sigma, frame, min_views, max_sigma, want_seen):
    import torch
    n = shape[::-1]
    g = {"n_views": Guarded(n, torch.uint8), "sig_max": Guarded(n, torch.float32), "summary": Guarded((pr.SUMMARY,), torch.int64)}
    if want_seen:
        g["seen"] = Guarded(n, torch.int64)
    core.coverage_map_dev(shape, *grid, size, near, far, sigma, frame, min_views, max_sigma, g["n_views"].ptr, g["sig_max"].ptr,
                          g["seen"].ptr if want_seen else 0, g["summary"].ptr)
    core.synchronize()
    assert all(v.intact() for v in g.values())
    out = {k: v.numpy() for k, v in g.items()}
    if want_seen:
        out["seen"] = out["seen"].view(np.uint64)
    return out


MAP_KEYS = ("n_views", "sig_max", "seen", "summary")


@pytest.mark.parametrize("shape", [(1, 1, 1), (64, 1, 1), (65, 3, 2), (7, 5, 129)])
def test_map_bit_for_bit_with_its_summary(core, shape):
    rig, P = _rig(8)
    _set(core, rig)
    size = rig["image_size"]
    nx, ny, nz = shape
    span = np.array([3.0, 2.4, 2.0])
    step = span / np.maximum(np.array(shape) - 1, 1)
    R0 = rig["R0"]                     # the grid's axes are the room's, seen from camera 0: a slanted grid in its coordinates
    e = [R0[:, d] * step[d] for d in range(3)]
    origin = rig["centre"] - sum(e[d] * (shape[d] - 1) / 2.0 for d in range(3)) if shape != (1, 1, 1) else rig["centre"]
    grid = (origin, e[0], e[1], e[2])
    base = pr.coverage_map(P, shape, *grid, size, 0.3, 5.0, 0.5)
    ok = base["info"] == pr.OK
    split = float(np.median(base["sig"][..., 2][ok])) if ok.sum() > 1 else INF
    for min_views, max_sigma in ((2, INF), (3, split), (65, INF)):
        want = pr.coverage_map(P, shape, *grid, size, 0.3, 5.0, 0.5, None, min_views, max_sigma)
        s = want["summary"]
        assert s[:65].sum() == nx * ny * nz
        if min_views == 65:
            assert s[65] == 0 and s[66:].tolist() == [nx, -1, ny, -1, nz, -1]
        elif max_sigma == split and ok.sum() > 3:
            assert 0 < s[65] < ok.sum()
        for want_seen in (True, False):
            _same(core.coverage_map(shape, *grid, size, 0.3, 5.0, 0.5, None, min_views, max_sigma, want_seen), want, MAP_KEYS)
            _same(_map_dev(core, shape, grid, size, 0.3, 5.0, 0.5, None, min_views, max_sigma, want_seen), want, MAP_KEYS)


# ----------------------------------------------------------------------------- bookkeeping
def test_optional_outputs_and_every_refusal(core):
    import torch
    rig, P = _rig(3)
    rng = np.random.default_rng(1)
    x = _cloud(rig, 65, rng)
    seen = _masks(3, 65, rng)
    size = rig["image_size"]
    fresh = capi.MocapCore(0)
    try:
        with pytest.raises(capi.MocapError) as ei:
            fresh.point_precision(x, seen)
        assert ei.value.code == -3          # MOCAP_E_NOCAMS
        with pytest.raises(capi.MocapError) as ei:
            fresh.coverage_map((2, 2, 2), np.zeros(3), *np.eye(3), size)
        assert ei.value.code == -3
    finally:
        fresh.close()
    _set(core, rig)
    want = pr.point_precision(P, x, seen=seen)
    got = _points_dev(core, x, seen, None, 0.0, INF, 1.0, None, cov=False, axis=False)     # NULL cov and NULL axis
    assert "cov" not in got and "axis" not in got
    _same(got, want)
    _same(_points_dev(core, x, seen, None, 0.0, INF, 1.0, None, cov=True, axis=False), want)

    d_xyz = torch.from_numpy(x).cuda()
    d_seen = torch.from_numpy(seen.view(np.int64)).cuda()
    d_corr = torch.zeros((65, 3), dtype=torch.int16, device="cuda:0")
    d_n = torch.ones(65, dtype=torch.int32, device="cuda:0")
    bad_frame = np.eye(3, 4)
    bad_frame[1, 2] = NAN

    def refused(call):
        g = _outs((65,))
        with pytest.raises(capi.MocapError) as ei:
            call(g)
        assert ei.value.code == capi.MOCAP_E_ARG
        core.synchronize()
        assert all(v.intact(whole=True) for v in g.values())

    def points(N=65, xyz=None, mask=True, size=None, near=0.0, far=INF, sigma=1.0, frame=None, null=None):
        def call(g):
            p = _ptrs(g)
            if null is not None:
                p[KEYS.index(null)] = 0
            core.point_precision_dev(N, d_xyz.data_ptr() if xyz is None else xyz, d_seen.data_ptr() if mask else 0, size, near, far, sigma,
                                     frame, *p)
        return call

    for call in (points(N=0), points(N=-1), points(N=capi.PM_MAX_POINTS + 1), points(sigma=0.0), points(sigma=-1.0), points(sigma=NAN),
                 points(sigma=INF), points(frame=bad_frame), points(xyz=0), points(null="sig"), points(null="n_views"), points(null="info"),
                 points(mask=False, size=(0, 480)), points(mask=False, size=(640, 0)), points(mask=False, size=(640, 480), near=-1.0),
                 points(mask=False, size=(640, 480), near=NAN), points(mask=False, size=(640, 480), near=2.0, far=2.0),
                 points(mask=False, size=(640, 480), near=0.0, far=NAN), points(mask=False, size=(640, 480), near=INF, far=INF)):
        refused(call)
    points(size=(0, 0), near=NAN, far=NAN)(_outs((65,)))          # named: the picture and the range are not read
    core.synchronize()

    def frames(F=5, K=13, xyz=True, corr=True, n=True, sigma=1.0, frame=None, null=None):
        def call(g):
            p = _ptrs(g)
            if null is not None:
                p[KEYS.index(null)] = 0
            core.frame_precision_dev(F, K, d_xyz.data_ptr() if xyz else 0, d_corr.data_ptr() if corr else 0, d_n.data_ptr() if n else 0, 0,
                                     sigma, frame, *p)
        return call

    for call in (frames(F=-1), frames(K=0), frames(F=capi.PM_MAX_POINTS, K=2), frames(sigma=0.0), frames(frame=bad_frame), frames(xyz=False),
                 frames(corr=False), frames(n=False), frames(null="sig"), frames(null="n_views"), frames(null="info")):
        refused(call)
    g = _outs((65,))
    frames(F=0)(g)                                                 # no frames: nothing to do, nothing written
    core.synchronize()
    assert all(v.intact(whole=True) for v in g.values())

    def refused_map(shape=(4, 3, 2), size=size, near=0.0, far=INF, sigma=1.0, frame=None, min_views=2, max_sigma=INF, null=None, grid_null=None):
        n = (2, 3, 4)
        g = {"n_views": Guarded(n, torch.uint8), "sig_max": Guarded(n, torch.float32), "seen": Guarded(n, torch.int64),
             "summary": Guarded((pr.SUMMARY,), torch.int64)}
        p = {k: (0 if k == null else v.ptr) for k, v in g.items()}
        with pytest.raises(capi.MocapError) as ei:
            core.coverage_map_dev(shape, np.zeros(3), *np.eye(3), size, near, far, sigma, frame, min_views, max_sigma, p["n_views"],
                                  p["sig_max"], p["seen"], p["summary"])
        assert ei.value.code == capi.MOCAP_E_ARG
        core.synchronize()
        assert all(v.intact(whole=True) for v in g.values())

    for kw in (dict(shape=(0, 3, 2)), dict(shape=(4, 0, 2)), dict(shape=(4, 3, 0)), dict(shape=(1025, 1, 1)), dict(shape=(1, 1025, 1)),
               dict(shape=(1, 1, 1025)), dict(shape=(1024, 1024, 129)), dict(size=(0, 10)), dict(size=(10, 0)), dict(near=-0.5), dict(near=NAN),
               dict(near=1.0, far=1.0), dict(far=NAN), dict(sigma=0.0), dict(sigma=NAN), dict(frame=bad_frame), dict(min_views=-1),
               dict(max_sigma=NAN), dict(null="n_views"), dict(null="sig_max"), dict(null="summary")):
        refused_map(**kw)
    lim = [capi.ctypes.c_int(), capi.ctypes.c_int64(), capi.ctypes.c_int()]
    core.lib.mocap_precision_limits(*[capi.ctypes.byref(v) for v in lim])
    assert [v.value for v in lim] == [capi.PM_MAX_POINTS, capi.PM_MAX_VOXELS, capi.PM_SUMMARY]
    core.lib.mocap_precision_limits(None, None, None)


def test_host_dev_second_call_and_second_stream_agree(core):
    import torch
    rig, P = _rig(8)
    _set(core, rig)
    rng = np.random.default_rng(2)
    x = _cloud(rig, 257, rng)
    size = rig["image_size"]
    shape = (33, 9, 5)
    grid = (rig["centre"] - np.array([1.6, 0.8, 0.4]), np.array([0.1, 0, 0]), np.array([0, 0.2, 0]), np.array([0, 0, 0.2]))

    def both():
        return _points_dev(core, x, None, size, 0.2, 8.0, 0.5, None), _map_dev(core, shape, grid, size, 0.2, 8.0, 0.5, None, 3, 0.0023, True)

    host_p = core.point_precision(x, None, 0.5, size, 0.2, 8.0)
    host_m = core.coverage_map(shape, *grid, size, 0.2, 8.0, 0.5, None, 3, 0.0023, True)
    p1, m1 = both()
    p2, m2 = both()
    stream = torch.cuda.Stream(device=0)
    try:
        core.set_stream(stream.cuda_stream)
        p3, m3 = both()
    finally:
        core.set_stream(0)
    for p, m in ((p1, m1), (p2, m2), (p3, m3)):
        _same(p, host_p)
        _same(m, host_m, MAP_KEYS)
    _same(host_p, pr.point_precision(P, x, image_size=size, near=0.2, far=8.0, sigma_px=0.5))
    assert 0 < host_m["summary"][65] < 33 * 9 * 5


def test_helpers_numpy_resident_and_statement_agree(core):
    import torch
    rig, P = _rig(8)
    _set(core, rig)
    size = rig["image_size"]
    rng = np.random.default_rng(6)
    x = _cloud(rig, 65, rng)
    seen = _masks(8, 65, rng)
    helpers.set_core(core)
    try:
        want = pr.point_precision(P, x, seen=seen, sigma_px=0.4)
        _same(helpers.point_precision(x, seen, sigma_px=0.4), want)
        got = helpers.point_precision(torch.from_numpy(x).cuda(), seen, sigma_px=0.4)
        _same({k: v.cpu().numpy() for k, v in got.items()}, want)
        want = pr.point_precision(P, x, image_size=size, near=0.1, far=7.0, sigma_px=0.4)
        _same(helpers.point_precision(x, None, 0.4, size, 0.1, 7.0), want)
        got = helpers.point_precision(torch.from_numpy(x).cuda(), None, 0.4, size, 0.1, 7.0)
        _same({k: v.cpu().numpy() for k, v in got.items()}, want)

        lo, hi, step = rig["centre"] - [1.0, 0.5, 0.5], rig["centre"] + [1.0, 0.5, 0.5], 0.25
        vol = helpers.capture_volume(lo, hi, step, size, sigma_px=0.4, near=0.1, far=7.0, min_views=3, max_sigma=0.0019, want_seen=True)
        assert vol["shape"] == (9, 5, 5)
        want = pr.coverage_map(P, (9, 5, 5), lo, [step, 0, 0], [0, step, 0], [0, 0, step], size, 0.1, 7.0, 0.4, None, 3, 0.0019)
        _same(vol, want, MAP_KEYS)
        res = helpers.capture_volume(lo, hi, step, size, sigma_px=0.4, near=0.1, far=7.0, min_views=3, max_sigma=0.0019, resident=True, want_seen=True)
        _same({k: res[k].cpu().numpy() if k != "seen" else res[k].cpu().numpy().view(np.uint64) for k in MAP_KEYS}, want, MAP_KEYS)
        good = int(want["summary"][65])
        assert vol["good_voxels"] == res["good_voxels"] == good and 0 < good < 225
        assert vol["good_volume"] == good * step ** 3 and vol["histogram"].tolist() == want["summary"][:65].tolist()
        box = want["summary"][66:].reshape(3, 2)
        assert np.array_equal(vol["bbox"][0], lo + box[:, 0] * step) and np.array_equal(vol["bbox"][1], lo + box[:, 1] * step)
        none = helpers.capture_volume(lo, hi, step, size, min_views=65)
        assert none["good_voxels"] == 0 and none["bbox"] is None and none["good_volume"] == 0.0
    finally:
        helpers.set_core(None)
