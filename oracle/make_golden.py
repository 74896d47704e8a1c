"""TEST INFRASTRUCTURE ONLY (oracle/).  Generates tests/golden/*.npz by running the
REFERENCE'S OWN functions (/root/reference/computer_code/api/helpers.py) through the
stub harness (oracle/ref_harness.py).  Runs only in the build container, where
/root/reference exists; the vectors are committed so the GPU box never needs it.

    python -m oracle.make_golden            # from the repo root

The reference ships no tests or vectors, so these are the
pinning set: reference outputs on seeded synthetic inputs.  The three OpenCV calls
inside are the NumPy restatements of oracle/cv_restate.py (PARITY UNPINNED there).
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "low-cost-mocap_amd"))

from mocap_core import synth  # noqa: E402
from oracle import ref_harness  # noqa: E402

OUT = os.path.join(_ROOT, "tests", "golden")

# Default camera poses of the reference UI (computer_code/src/App.tsx:44): a really calibrated
# 4-camera rig.  Numeric fixture only.
APP_TSX_POSES = [
    {"R": [[1, 0, 0], [0, 1, 0], [0, 0, 1]], "t": [0, 0, 0]},
    {"R": [[-0.0008290000610233772, -0.7947131755287576, 0.6069845808584402],
           [0.7624444396180684, 0.3922492478955913, 0.5146056781855716],
           [-0.6470531579819294, 0.46321862674804054, 0.6055994671226776]],
     "t": [-2.6049886186449047, -2.173986915510569, 0.7303458563542193]},
    {"R": [[-0.9985541623963866, -0.028079891357569067, -0.045837806036037466],
           [-0.043210651917521686, -0.08793122558361385, 0.9951888962042462],
           [-0.03197537054848707, 0.995730696156702, 0.0865907408997996]],
     "t": [0.8953888630067902, -3.4302652822708373, 3.70967106300893]},
    {"R": [[-0.4499864100408215, 0.6855400696798954, -0.5723172578577878],
           [-0.7145273934510732, 0.10804105689305427, 0.6912146801345055],
           [0.5356891214002657, 0.7199735709654319, 0.4412201517663212]],
     "t": [2.50141072072536, -2.313616767292231, 1.8529907514099284]},
]
# computer_code/api/camera-params copy.json:3-21 (three really calibrated intrinsics)
CALIBRATED_K = [
    [[268.66976067, 0, 123.58679484], [0, 268.57495496, 167.56126939], [0, 0, 1]],
    [[269.95158059, 0, 139.37072352], [0, 270.09608831, 160.36482761], [0, 0, 1]],
    [[269.95158059, 0, 139.37072352], [0, 270.09608831, 160.36482761], [0, 0, 1]],
]


def rig_from_poses(poses, Ks, image_size=(320, 320)):
    """Wrap explicit poses as a synth rig; markers are placed around the point closest to all optical axes."""
    R = np.array([np.array(p["R"], dtype=np.float64) for p in poses])
    t = np.array([np.array(p["t"], dtype=np.float64).reshape(3) for p in poses])
    A = np.zeros((3, 3))
    b = np.zeros(3)
    for i in range(len(R)):
        c = -R[i].T @ t[i]
        d = R[i].T @ np.array([0, 0, 1.0])
        Pm = np.eye(3) - np.outer(d, d)
        A += Pm
        b += Pm @ c
    centre = np.linalg.solve(A, b)
    return {"K": np.array(Ks, dtype=np.float64), "R": R, "t": t, "image_size": image_size,
            "centre": centre, "R0": np.eye(3)}


def run_reference_frames(H, rig, blobs, counts, as_int=True):
    """find_point_correspondance_and_object_points (helpers.py:339) per frame, also capturing the
    winning group's coordinates per kept root (what the reference carries instead of indices)."""
    F, C, M, _ = blobs.shape
    poses = synth.rig_to_pose_dicts(rig)
    kmax = C * M
    ref_xyz = np.full((F, kmax, 3), np.nan)
    ref_err = np.full((F, kmax), np.nan)
    ref_xy = np.full((F, kmax, C, 2), np.nan)
    ref_n = np.zeros(F, dtype=np.int32)
    captured = []
    orig = H.calculate_reprojection_errors

    def spy(image_points, object_points, camera_poses):
        e = orig(image_points, object_points, camera_poses)
        captured.append(image_points[int(np.argmin(e))])
        return e

    H.calculate_reprojection_errors = spy
    try:
        for f in range(F):
            captured.clear()
            ip = synth.frame_to_reference_lists(blobs[f], counts[f], as_int=as_int)
            err, pts, _ = H.find_point_correspondance_and_object_points(ip, poses, [None] * C)
            k = len(err)
            assert k == len(captured)
            ref_n[f] = k
            if k:
                ref_xyz[f, :k] = np.asarray(pts, dtype=np.float64)
                ref_err[f, :k] = err
                for r, grp in enumerate(captured):
                    for c, xy in enumerate(grp):
                        if xy[0] is not None:
                            ref_xy[f, r, c] = xy
    finally:
        H.calculate_reprojection_errors = orig
    return ref_xyz, ref_err, ref_xy, ref_n


def golden_frames(name, rig, n_frames, n_markers, seed, Ks_list=None, **kw):
    C = len(rig["R"])
    if Ks_list is None:
        Ks_list = rig["K"].tolist()
    H = ref_harness.load_reference(C, intrinsics=Ks_list)
    blobs, counts, _ = synth.make_blob_stream(rig, n_frames, n_markers, seed=seed, **kw)
    ref_xyz, ref_err, ref_xy, ref_n = run_reference_frames(H, rig, blobs, counts)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), K=rig["K"], R=rig["R"], t=rig["t"],
                        blobs=blobs, counts=counts, ref_xyz=ref_xyz, ref_err=ref_err,
                        ref_corr_xy=ref_xy, ref_n=ref_n)
    print(name, "frames", n_frames, "points", int(ref_n.sum()))


def golden_dlt(name, rig, n_points, seed, Ks_list=None, dropout=0.3):
    C = len(rig["R"])
    if Ks_list is None:
        Ks_list = rig["K"].tolist()
    H = ref_harness.load_reference(C, intrinsics=Ks_list)
    obs, _ = synth.make_ba_observations(rig, n_points, seed=seed, dropout=dropout)
    obs[0, :, :] = np.nan            # no view at all
    obs[1, 1:, :] = np.nan           # a single view
    poses = synth.rig_to_pose_dicts(rig)
    ref_obs = synth.obs_to_reference_array(obs)
    xyz = H.triangulate_points(ref_obs, poses)
    ref_xyz = np.full((n_points, 3), np.nan)
    ref_err = np.full(n_points, np.nan)
    for n in range(n_points):
        if xyz[n][0] is not None:
            ref_xyz[n] = np.asarray(xyz[n], dtype=np.float64)
            ref_err[n] = H.calculate_reprojection_error(ref_obs[n], xyz[n], poses)
    # calculate_reprojection_errors skips None rows (helpers.py:207-208): keep the packed form too
    packed = H.calculate_reprojection_errors(ref_obs, xyz, poses)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), K=rig["K"], R=rig["R"], t=rig["t"], obs=obs,
                        ref_xyz=ref_xyz, ref_err=ref_err, ref_err_packed=packed)
    print(name, "points", n_points, "valid", int(np.isfinite(ref_err).sum()))


def golden_ba(name, C, n_points, seed, run_solver):
    """residual_function values (helpers.py:264-276) at several parameter vectors, and (small case)
    the poses bundle_adjustment returns (helpers.py:287-290)."""
    from scipy.spatial.transform import Rotation
    H = ref_harness.load_reference(C)
    rig = synth.ring_rig(C)
    rng = np.random.default_rng(seed)
    obs, _ = synth.make_ba_observations(rig, n_points, seed=seed, dropout=0.1)
    init = synth.perturb_rig(rig, rng)
    ref_obs = synth.obs_to_reference_array(obs)
    poses0 = [{"R": init["R"][i].copy(), "t": init["t"][i].copy()} for i in range(C)]

    # helpers.py:278-285 (parameter vector layout)
    x0 = [320.0]
    for i in range(1, C):
        x0 += [320.0] + Rotation.from_matrix(init["R"][i]).as_rotvec().tolist() + init["t"][i].tolist()
    x0 = np.array(x0)
    xs = [x0] + [x0 + rng.normal(0, 1e-3, x0.size) for _ in range(3)]

    # evaluate the reference's residual_function closure by capturing it from least_squares
    captured = {}
    real_ls = H.optimize.least_squares

    def fake_ls(fun, x_init, **kw):
        captured["fun"] = fun
        captured["x_init"] = np.array(x_init)
        captured["kw"] = kw

        class Res:
            x = np.array(x_init)
        return Res()

    H.optimize.least_squares = fake_ls
    try:
        H.bundle_adjustment(ref_obs, poses0, ref_harness.NullSocket())
    finally:
        H.optimize.least_squares = real_ls
    assert np.allclose(captured["x_init"], x0, atol=1e-12), (captured["x_init"], x0)
    res32 = np.array([captured["fun"](x) for x in xs])          # float32, None rows dropped
    # float64 (pre-cast) residuals through the reference's public functions
    res64 = []
    for x in xs:
        poses = [{"R": np.eye(3), "t": np.zeros(3)}]
        for i in range(C - 1):
            poses.append({"R": Rotation.from_rotvec(x[i * 7 + 2:i * 7 + 5]).as_matrix(),
                          "t": x[i * 7 + 5:i * 7 + 8]})
        op = H.triangulate_points(ref_obs, poses)
        res64.append(H.calculate_reprojection_errors(ref_obs, op, poses))
    res64 = np.array(res64)
    out = dict(K=rig["K"], R_true=rig["R"], t_true=rig["t"], R_init=init["R"], t_init=init["t"],
               obs=obs, xs=np.array(xs), res32=res32, res64=res64,
               ls_kwargs=np.array(sorted((k, str(v)) for k, v in captured["kw"].items())))
    if run_solver:
        import contextlib
        import io
        # the reference's own call (helpers.py:287), observed: the optimizer's result object and every
        # parameter vector its residual_function is asked about, in order
        seen = {"xs": []}

        def spy_ls(fun, x_init, **kw):
            def spy_fun(x):
                seen["xs"].append(np.array(x, dtype=np.float64))
                return fun(x)
            seen["res"] = real_ls(spy_fun, x_init, **kw)
            return seen["res"]

        H.optimize.least_squares = spy_ls
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                sol = H.bundle_adjustment(ref_obs, [{"R": init["R"][i].copy(), "t": init["t"][i].copy()}
                                                    for i in range(C)], ref_harness.NullSocket())
        finally:
            H.optimize.least_squares = real_ls
        out["R_ba"] = np.array([np.asarray(p["R"], dtype=np.float64) for p in sol])
        out["t_ba"] = np.array([np.asarray(p["t"], dtype=np.float64).reshape(3) for p in sol])
        res = seen["res"]
        out["x_ba"] = np.array(res.x, dtype=np.float64)
        out["ba_stats"] = np.array([res.nfev, res.njev, res.status], dtype=np.int64)
        out["ba_cost"] = np.array([res.cost, res.optimality], dtype=np.float64)
        out["ba_eval_xs"] = np.array(seen["xs"])            # (nfev + njev * n, n): trial points and FD probes
        # How reproducible is that result?  The same reference call with its start vector moved in the LAST BIT
        # (x0 * (1 + 1e-15 N(0,1)), three draws): the float32 cast of the residuals (helpers.py:273) turns any
        # 1e-16 change of a trial point into 1e-4-relative changes of a few Jacobian entries, so the
        # reference's own poses move by this much under perturbations no caller could notice.  This is the
        # yardstick for a solver that cannot share SciPy's LAPACK bits (mode "resident").
        self_dR, self_dt, self_stats = [], [], []
        for k in range(3):
            prng = np.random.default_rng(1000 + k)

            def nudged_ls(fun, x_init, **kw):
                x_init = np.asarray(x_init, dtype=np.float64)
                seen["res"] = real_ls(fun, x_init * (1.0 + 1e-15 * prng.standard_normal(x_init.size)), **kw)
                return seen["res"]

            H.optimize.least_squares = nudged_ls
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    sol_k = H.bundle_adjustment(ref_obs, [{"R": init["R"][i].copy(), "t": init["t"][i].copy()}
                                                          for i in range(C)], ref_harness.NullSocket())
            finally:
                H.optimize.least_squares = real_ls
            Rk = np.array([np.asarray(p["R"], dtype=np.float64) for p in sol_k])
            tk = np.array([np.asarray(p["t"], dtype=np.float64).reshape(3) for p in sol_k])
            self_dR.append(np.abs(Rk - out["R_ba"]).max())
            self_dt.append(np.abs(tk - out["t_ba"]).max() / np.abs(out["t_ba"]).max())
            self_stats.append([seen["res"].nfev, seen["res"].njev, seen["res"].status])
        out["self_dR"] = np.array(self_dR)
        out["self_dt"] = np.array(self_dt)
        out["self_stats"] = np.array(self_stats, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(name, "points", n_points, "m", res32.shape[1])


def reference_world_epilogue(object_points, to_world):
    """Runs the reference's OWN lines computer_code/api/helpers.py:97-103 (inline in
    Cameras._camera_read, not callable on their own): the loop is read from the file and exec'd."""
    path = os.path.join(ref_harness.REFERENCE_API, "helpers.py")
    with open(path) as fh:
        lines = fh.read().split("\n")[96:103]
    assert lines[0].strip() == "for i, object_point in enumerate(object_points):", lines[0]
    assert "object_points[i] = new_object_point" in lines[-1], lines[-1]
    import textwrap
    import types
    env = {"np": np, "object_points": np.array(object_points, dtype=np.float64).copy(),
           "self": types.SimpleNamespace(to_world_coords_matrix=to_world)}
    exec(textwrap.dedent("\n".join(lines)), env)
    return env["object_points"]


def golden_post(name, n_frames, k_max, seed):
    """World-coordinate epilogue (helpers.py:96-103) and locate_objects (helpers.py:424-480)."""
    H = ref_harness.load_reference(4)
    W = synth.APP_TSX_TO_WORLD
    Winv = np.linalg.inv(np.array(W))
    xyz_w, err, n_pts = synth.make_object_frames(n_frames, k_max, seed=seed)
    # camera-0 coordinates whose epilogue image is (about) xyz_w: undo swap, W and the sign flip
    cam = np.full_like(xyz_w, np.nan)
    ref_world = np.full_like(xyz_w, np.nan)
    o_max = 8
    ref_pos = np.full((n_frames, o_max, 3), np.nan)
    ref_heading = np.full((n_frames, o_max), np.nan)
    ref_error = np.full((n_frames, o_max), np.nan)
    ref_drone = np.full((n_frames, o_max), -1, dtype=np.int32)
    ref_nobj = np.zeros(n_frames, dtype=np.int32)
    for f in range(n_frames):
        n = int(n_pts[f])
        q = xyz_w[f, :n][:, [0, 2, 1]]
        h = np.c_[q, np.ones(n)] @ Winv.T
        cam[f, :n] = (h[:, :3] / h[:, 3:4]) * np.array([-1, -1, 1.0])
        if n:
            ref_world[f, :n] = reference_world_epilogue(cam[f, :n], W)
        objs = H.locate_objects(ref_world[f, :n].copy(), err[f, :n].copy())
        ref_nobj[f] = len(objs)
        for j, o in enumerate(objs[:o_max]):
            ref_pos[f, j] = o["pos"]
            ref_heading[f, j] = o["heading"]
            ref_error[f, j] = o["error"]
            ref_drone[f, j] = o["droneIndex"]
    np.savez_compressed(os.path.join(OUT, name + ".npz"), to_world=np.array(W, dtype=np.float64), cam_xyz=cam,
                        err=err, n_pts=n_pts, ref_world=ref_world, ref_pos=ref_pos, ref_heading=ref_heading,
                        ref_error=ref_error, ref_drone=ref_drone, ref_nobj=ref_nobj)
    print(name, "frames", n_frames, "objects", int(ref_nobj.sum()))


def golden_locate_edges(name="locate_edges"):
    """locate_objects (helpers.py:424-480) on the constructed frames of tests/locate_cases.py: frames on the function's decision
    edges, shared and skipped points, members across the 64-point chunk edges, non-finite points, out-of-range counts (no valid
    slot: the function sees an empty frame) and 12 dense-clutter frames.  Per family: the inputs and the reference's n_obj,
    pos, heading, error and droneIndex (as many object slots as the family's fullest frame needs)."""
    sys.path.insert(0, os.path.join(_ROOT, "tests"))
    import locate_cases as lc
    H = ref_harness.load_reference(4)
    arrays, report = {}, []
    for fam, cs, idx in lc.recorded():
        xyz, err, n_pts = cs["xyz"][idx], cs["err"][idx], cs["n_pts"][idx]
        n_eff = lc.effective_n(n_pts, err.shape[1])
        with np.errstate(invalid="ignore"):      # inf - inf among the non-finite points
            objs = [H.locate_objects(xyz[f, :n_eff[f]].copy(), err[f, :n_eff[f]].copy()) for f in range(len(idx))]
        o_max = max(1, max(len(o) for o in objs))
        ref_pos = np.full((len(idx), o_max, 3), np.nan)
        ref_heading = np.full((len(idx), o_max), np.nan)
        ref_error = np.full((len(idx), o_max), np.nan)
        ref_drone = np.full((len(idx), o_max), -1, dtype=np.int32)
        for f, fo in enumerate(objs):
            for j, o in enumerate(fo):
                ref_pos[f, j], ref_heading[f, j], ref_error[f, j], ref_drone[f, j] = o["pos"], o["heading"], o["error"], o["droneIndex"]
        arrays.update({fam + "_frames": idx.astype(np.int32), fam + "_xyz": xyz, fam + "_err": err, fam + "_n_pts": n_pts,
                       fam + "_ref_nobj": np.array([len(o) for o in objs], dtype=np.int32), fam + "_ref_pos": ref_pos,
                       fam + "_ref_heading": ref_heading, fam + "_ref_error": ref_error, fam + "_ref_drone": ref_drone})
        report.append(f"{fam} {len(idx)}/{sum(len(o) for o in objs)}")
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **arrays)
    print(name, "frames/objects:", ", ".join(report))


def golden_track(name, n_frames, seed):
    """The live loop's body after _find_dot, end to end through the reference's own code (helpers.py:94-108):
    find_point_correspondance_and_object_points -> the world-coordinate loop (exec'd from the file) -> locate_objects,
    on the really calibrated rig + to-world matrix of the reference UI (App.tsx:44-45).  Markers: 0-2 drone LED
    triangles + clutter per frame, projected to int() pixel centroids like _find_dot's."""
    rig = rig_from_poses(APP_TSX_POSES, [synth.DEFAULT_K] * 4)
    C = 4
    W = synth.APP_TSX_TO_WORLD
    H = ref_harness.load_reference(C, intrinsics=rig["K"].tolist())
    poses = synth.rig_to_pose_dicts(rig)
    rng = np.random.default_rng(seed)
    M = 12
    blobs = np.zeros((n_frames, C, M, 2), dtype=np.float32)
    counts = np.zeros((n_frames, C), dtype=np.int32)
    h = np.sqrt(0.095 ** 2 - 0.075 ** 2)
    for f in range(n_frames):
        pts = []
        for _ in range(int(rng.integers(0, 3))):
            c = rig["centre"] + rng.uniform(-0.35, 0.35, 3)
            u = rng.normal(0, 1, 3)
            u /= np.linalg.norm(u)
            w = np.cross(u, rng.normal(0, 1, 3))
            w /= np.linalg.norm(w)
            pts += [c + h * w, c + 0.075 * u, c - 0.075 * u]
        pts += [rig["centre"] + rng.uniform(-0.45, 0.45, 3) for _ in range(int(rng.integers(0, 4)))]
        for i in range(C):
            px = []
            for X in pts:
                xc = rig["R"][i] @ X + rig["t"][i]
                if xc[2] <= 0.1 or rng.random() < 0.03:
                    continue
                uv = rig["K"][i] @ (xc / xc[2])
                if 0 <= uv[0] < 320 and 0 <= uv[1] < 320:
                    px.append([int(uv[0]), int(uv[1])])
            px = [px[j] for j in rng.permutation(len(px))][:M]
            counts[f, i] = len(px)
            if px:
                blobs[f, i, :len(px)] = np.array(px, dtype=np.float32)
    kmax, o_max = C * M, 8
    ref_n = np.zeros(n_frames, dtype=np.int32)
    ref_err = np.full((n_frames, kmax), np.nan)
    ref_world = np.full((n_frames, kmax, 3), np.nan)
    ref_nobj = np.zeros(n_frames, dtype=np.int32)
    ref_pos = np.full((n_frames, o_max, 3), np.nan)
    ref_heading = np.full((n_frames, o_max), np.nan)
    ref_error = np.full((n_frames, o_max), np.nan)
    ref_drone = np.full((n_frames, o_max), -1, dtype=np.int32)
    for f in range(n_frames):
        ip = synth.frame_to_reference_lists(blobs[f], counts[f], as_int=True)
        errors, object_points, _ = H.find_point_correspondance_and_object_points(ip, poses, [None] * C)
        k = len(errors)
        ref_n[f] = k
        if not k:
            continue
        object_points = reference_world_epilogue(object_points, W)       # helpers.py:96-103
        objs = H.locate_objects(object_points, errors)                   # helpers.py:108
        ref_err[f, :k] = errors
        ref_world[f, :k] = object_points
        ref_nobj[f] = len(objs)
        for j, o in enumerate(objs[:o_max]):
            ref_pos[f, j] = o["pos"]
            ref_heading[f, j] = o["heading"]
            ref_error[f, j] = o["error"]
            ref_drone[f, j] = o["droneIndex"]
    np.savez_compressed(os.path.join(OUT, name + ".npz"), K=rig["K"], R=rig["R"], t=rig["t"], to_world=np.array(W, dtype=np.float64),
                        blobs=blobs, counts=counts, ref_n=ref_n, ref_err=ref_err, ref_world=ref_world, ref_nobj=ref_nobj,
                        ref_pos=ref_pos, ref_heading=ref_heading, ref_error=ref_error, ref_drone=ref_drone)
    print(name, "frames", n_frames, "points", int(ref_n.sum()), "objects", int(ref_nobj.sum()))


def golden_blobs(name, C, n_frames, n_markers, seed, Ks=None, dists=None, rotation=None, noisy=False):
    """Blob extraction: the reference's own Cameras._camera_read preprocessing and
    Cameras._find_dot (helpers.py:68-82, 143-163) on synthetic raw frames.  rot90 / make_square / the
    centroid rule are the reference's code; its OpenCV calls are oracle/cv_image_restate.py."""
    rig = synth.ring_rig(C)
    Ks = [synth.DEFAULT_K] * C if Ks is None else Ks
    rig["K"] = np.array(Ks, dtype=np.float64)
    dists = [synth.REFERENCE_DISTORTION] * C if dists is None else dists
    rotation = [0] * C if rotation is None else rotation
    images, _ = synth.render_camera_frames(rig, n_frames, n_markers, seed=seed, noise_levels=2,
                                           spot_sigma=(1.0, 6.0) if noisy else (1.2, 2.2))
    if noisy:
        rng = np.random.default_rng(seed)
        images[0, 0] = np.maximum(images[0, 0], rng.integers(0, 90, images[0, 0].shape, dtype=np.uint8))
    H = ref_harness.load_reference(C, intrinsics=[np.asarray(k).tolist() for k in Ks])
    ref_frames, ref_pts = [], []
    for f in range(n_frames):
        fr, pts = ref_harness.reference_find_dots(H, list(images[f]), distortion=dists, rotation=rotation)
        ref_frames.append(np.array(fr))
        ref_pts.append(pts)
    mmax = max(1, max(len(p) for fp in ref_pts for p in fp))
    ref_points = np.zeros((n_frames, C, mmax, 2), dtype=np.int32)
    ref_counts = np.zeros((n_frames, C), dtype=np.int32)
    for f in range(n_frames):
        for c in range(C):
            p = ref_pts[f][c]
            if p != [[None, None]]:
                ref_counts[f, c] = len(p)
                ref_points[f, c, :len(p)] = p
    np.savez_compressed(os.path.join(OUT, name + ".npz"), images=images, K=rig["K"], dist=np.array(dists, dtype=np.float64),
                        rotation=np.array(rotation, dtype=np.int32), ref_frames=np.array(ref_frames),
                        ref_points=ref_points, ref_counts=ref_counts)
    print(name, "frame sets", n_frames, "points", int(ref_counts.sum()))


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--blobs-only" in sys.argv:
        return main_blobs()
    if "--pose-only" in sys.argv:
        return main_pose()
    if "--ba-only" in sys.argv:
        return main_ba()
    if "--track-only" in sys.argv:
        return golden_track("track_apptsx_chain", 60, seed=19)
    if "--locate-only" in sys.argv:
        return golden_locate_edges()
    if "--with-cv2" in sys.argv:       # pin the OpenCV restatements against a REAL cv2, where one exists
        from oracle import make_cv2_golden
        return make_cv2_golden.main()
    main_blobs()
    main_pose()
    # BASELINE.json configs[0..2] shapes
    golden_frames("frames_c2_m1", synth.ring_rig(2), 8, 1, seed=0)
    golden_frames("frames_c4_m4", synth.ring_rig(4), 40, 4, seed=0)
    golden_frames("frames_c8_m16", synth.ring_rig(8), 6, 16, seed=0)
    # VGA intrinsics (configs[1] "640x480")
    golden_frames("frames_c4_m4_vga", synth.ring_rig(4, K=synth.VGA_K, image_size=(640, 480)), 20, 4, seed=1)
    # really calibrated rig of the reference UI + default intrinsics
    golden_frames("frames_apptsx_rig", rig_from_poses(APP_TSX_POSES, [synth.DEFAULT_K] * 4), 20, 5,
                  seed=2, half_extent=0.5)
    # non-identical intrinsics: exercises the compacted-index quirk (helpers.py:305-307)
    rig3 = synth.ring_rig(3)
    rig3["K"] = np.array(CALIBRATED_K, dtype=np.float64)
    golden_frames("frames_c3_calibK", rig3, 20, 4, seed=3, Ks_list=CALIBRATED_K, half_extent=0.5, dropout=0.2)
    # heavy dropout / empty cameras
    golden_frames("frames_c4_dropout", synth.ring_rig(4), 30, 3, seed=4, dropout=0.5)
    # explicit-correspondence DLT + reprojection error
    golden_dlt("dlt_c4", synth.ring_rig(4), 64, seed=5)
    golden_dlt("dlt_c8", synth.ring_rig(8), 96, seed=6)
    golden_dlt("dlt_c3_calibK", rig3, 48, seed=7, Ks_list=CALIBRATED_K)
    main_ba()
    # the rows right after the path: world-coordinate epilogue + object locator
    golden_post("post_world_locate", 300, 24, seed=10)
    # ... the locator again where its decisions flip and its searches change chunk
    golden_locate_edges()
    # ... and the live loop's body end to end (match -> world -> locate) on the reference UI's own rig
    golden_track("track_apptsx_chain", 60, seed=19)


def golden_pose(name, C, n_points, seed, Ks=None, dropout=0.05, noise_px=0.3):
    """Initial pose estimation: the reference's own calculate_camera_pose handler
    (index.py:229-270, extracted by AST) up to the poses it hands to bundle_adjustment."""
    rig = synth.ring_rig(C)
    if Ks is not None:
        rig["K"] = np.array(Ks, dtype=np.float64)
    obs, _ = synth.make_ba_observations(rig, n_points, seed=seed, dropout=dropout, noise_px=noise_px)
    obs = np.trunc(obs)                                  # _find_dot yields int() centroids (helpers.py:153-154)
    H = ref_harness.load_reference(C, intrinsics=[np.asarray(k).tolist() for k in rig["K"]])
    poses = ref_harness.reference_initial_poses(H, synth.obs_to_reference_array(obs, as_int=True).tolist())
    np.savez_compressed(os.path.join(OUT, name + ".npz"), K=rig["K"], obs=obs,
                        ref_R=np.array([p["R"] for p in poses]),
                        ref_t=np.array([np.asarray(p["t"], dtype=np.float64).reshape(3) for p in poses]),
                        true_R=rig["R"], true_t=rig["t"])
    print(name, "points", n_points, "cameras", C)


def main_ba():
    golden_ba("ba_c4_n40", 4, 40, seed=8, run_solver=False)
    golden_ba("ba_c3_n24", 3, 24, seed=9, run_solver=True)
    golden_ba("ba_c4_n60_solved", 4, 60, seed=16, run_solver=True)
    golden_ba("ba_c6_n80_solved", 6, 80, seed=18, run_solver=True)        # between the two: where does the reference stop reproducing itself?
    golden_ba("ba_c8_n100_solved", 8, 100, seed=17, run_solver=True)      # ~2-3 min of reference CPU


def main_pose():
    golden_pose("pose_c4_n120", 4, 120, seed=3)
    golden_pose("pose_c8_n400", 8, 400, seed=14, dropout=0.2)
    golden_pose("pose_c3_calibK", 3, 200, seed=15, Ks=CALIBRATED_K)


def main_blobs():
    # the step before the path: raw camera frames -> image points
    golden_blobs("blobs_c2_ref_params", 2, 1, 8, seed=11)
    golden_blobs("blobs_c3_calib_rot", 3, 1, 6, seed=12, Ks=CALIBRATED_K,
                 dists=[[-0.2, 0.1, 0.002, -0.001, 0.05], list(synth.REFERENCE_DISTORTION), [0, 0, 0, 0, 0]],
                 rotation=[0, 2, 2])
    golden_blobs("blobs_c1_noisy", 1, 1, 10, seed=13, noisy=True)


if __name__ == "__main__":
    main()
