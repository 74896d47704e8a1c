"""Writes tests/golden/calib_tail_session.npz: what the reference's OWN three calibration-tail handlers emit for two synthetic
captures -- `determine-scale` (computer_code/api/index.py:290-309), `acquire-floor` (:158-194) and `set-origin` (:197-210).

The handlers are cut out of index.py by their AST (index.py itself imports flask, serial and ruckig, which a machine without
the rig does not have; oracle/ref_harness.reference_initial_poses does the same for `calculate-camera-pose`) and run
unmodified against a recording `socketio` and a stand-in `Cameras` singleton.  The fixture holds inputs and emitted payloads
only.

Session (per record): 300 frames of 0-4 points, K_max 8; points on a plane tilted about 12 degrees with 2 mm of noise around
an offset; every two-point frame is a pair about 0.4 m apart; four poses with non-zero t; `set-origin` on the matrix
`acquire-floor` emitted.  Record 0 sits at (2.0, -1.5, 0.7) m, record 1 at (20, -15, 3) m, where cond([x y 1]) is about 1.1e3.
Pose 1's t starts with exactly 1.0: the emitted t[1][0] IS the handler's scale_factor, bit for bit.

usage: python scripts/make_calib_tail_golden.py      (needs the reference checkout and SciPy)"""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_harness import REFERENCE_API, reference_available  # noqa: E402

SEED = 20260
F, K_MAX = 300, 8
OFFSETS = ((2.0, -1.5, 0.7), (20.0, -15.0, 3.0))
PLANE_A, PLANE_B = 0.17, -0.1277          # |(a, b)| = tan(12.0 deg)
HALF_EXTENT = 1.0                         # points spread +-1 m around the offset in x and y
NOISE = 0.002
PAIR_DISTANCE = 0.4


class RecordingSocket:
    def __init__(self):
        self.events = []

    def emit(self, name, payload):
        self.events.append((name, payload))


class _Cameras:
    """Stand-in for the reference's Cameras singleton: the handlers only assign to_world_coords_matrix."""
    _inst = None

    @classmethod
    def instance(cls):
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst


def reference_handlers(socketio):
    from scipy import linalg
    src = open(os.path.join(REFERENCE_API, "index.py")).read()
    want = ("determine_scale", "acquire_floor", "set_origin")
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(f.name for f in fns) == sorted(want)
    for fn in fns:
        fn.decorator_list = []
    ns = {"np": np, "linalg": linalg, "Cameras": _Cameras, "socketio": socketio}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "index.py:calibration tail", "exec"), ns)
    return ns


def make_capture(rng, offset):
    """-> xyz [F][K_MAX][3] (NaN beyond n_pts), n_pts [F]"""
    off = np.asarray(offset)
    counts = rng.choice(5, size=F, p=[0.1, 0.2, 0.3, 0.2, 0.2])
    xyz = np.full((F, K_MAX, 3), np.nan)

    def on_plane(uv):
        z = PLANE_A * uv[..., 0] + PLANE_B * uv[..., 1]
        return off + np.concatenate([uv, z[..., None]], axis=-1) + rng.normal(0, NOISE, uv.shape[:-1] + (3,))

    for f in range(F):
        n = int(counts[f])
        if n == 2:
            ang = rng.uniform(0, 2 * np.pi)
            d = np.array([np.cos(ang), np.sin(ang)])
            d = d * PAIR_DISTANCE / np.sqrt(1.0 + (PLANE_A * d[0] + PLANE_B * d[1]) ** 2)    # 0.4 m along the plane
            mid = rng.uniform(-HALF_EXTENT + 0.2, HALF_EXTENT - 0.2, 2)
            xyz[f, :2] = on_plane(np.stack([mid - d / 2, mid + d / 2]))
        elif n:
            xyz[f, :n] = on_plane(rng.uniform(-HALF_EXTENT, HALF_EXTENT, (n, 2)))
    return xyz, counts.astype(np.int32)


def main():
    if not reference_available():
        raise SystemExit("the reference checkout is not present")
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(SEED)
    out = {k: [] for k in ("xyz", "n_pts", "pose_R", "pose_t", "scaled_t", "floor_to_world", "origin_point", "origin_to_world")}
    for offset in OFFSETS:
        xyz, n_pts = make_capture(rng, offset)
        assert (n_pts == 2).sum() >= 60
        object_points = [xyz[f, :n_pts[f]].tolist() for f in range(F)]
        pose_R = np.array([np.eye(3)] + [Rotation.from_rotvec(rng.normal(0, 0.5, 3)).as_matrix() for _ in range(3)])
        pose_t = np.array([[0.25, -0.5, 0.125]] + [rng.uniform(-3, 3, 3) for _ in range(3)])
        pose_t[1, 0] = 1.0
        sock = RecordingSocket()
        ns = reference_handlers(sock)
        ns["determine_scale"]({"objectPoints": object_points,
                               "cameraPoses": [{"R": pose_R[i].tolist(), "t": pose_t[i].tolist()} for i in range(4)]})
        ns["acquire_floor"]({"objectPoints": object_points})
        name, payload = sock.events[1]
        assert name == "to-world-coords-matrix"
        floor_W = np.array(payload["to_world_coords_matrix"])
        point = xyz[int(np.nonzero(n_pts)[0][7]), 0]
        ns["set_origin"]({"objectPoint": point.tolist(), "toWorldCoordsMatrix": floor_W.tolist()})
        assert [e[0] for e in sock.events] == ["camera-pose", "to-world-coords-matrix", "to-world-coords-matrix"]
        assert list(sock.events[0][1].keys()) == ["error", "camera_poses"] and sock.events[0][1]["error"] is None
        assert all(list(p.keys()) == ["R", "t"] for p in sock.events[0][1]["camera_poses"])
        assert np.array_equal(np.array([p["R"] for p in sock.events[0][1]["camera_poses"]]), pose_R)
        assert np.array_equal(_Cameras.instance().to_world_coords_matrix, np.array(sock.events[2][1]["to_world_coords_matrix"]))
        out["xyz"].append(xyz)
        out["n_pts"].append(n_pts)
        out["pose_R"].append(pose_R)
        out["pose_t"].append(pose_t)
        out["scaled_t"].append(np.array([p["t"] for p in sock.events[0][1]["camera_poses"]]))
        out["floor_to_world"].append(floor_W)
        out["origin_point"].append(point)
        out["origin_to_world"].append(np.array(sock.events[2][1]["to_world_coords_matrix"]))
        pts = xyz[np.arange(K_MAX)[None, :] < n_pts[:, None]]
        A = np.c_[pts[:, :2], np.ones(len(pts))]
        print(f"offset {offset}: {len(pts)} points, {(n_pts == 2).sum()} pairs, cond([x y 1]) = {np.linalg.cond(A):.4g}, "
              f"scale_factor = {out['scaled_t'][-1][1, 0]!r}")
    path = os.path.join(ROOT, "tests", "golden", "calib_tail_session.npz")
    np.savez_compressed(path, actual_distance=np.array([0.15]), **{k: np.array(v) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
