"""Writes tests/golden/objfilter_two_drones.npz: the reference's OWN KalmanFilter.py / LowPassFilter.py (unmodified, real SciPy)
driven frame by frame over a synthetic two-drone session, on the CPU.

   python scripts/make_objfilter_golden.py

OpenCV is not a dependency of this project, so `cv2` is a stub here whose KalmanFilter restates cv::KalmanFilter's predict()
and correct() (video/src/kalman.cpp) in NumPy at one dtype; time.time is patched to return the session's time stamps.  The
session is run twice -- float32 stub (what cv.KalmanFilter(9, 6) is) and float64 stub -- and the largest difference between
the two, per output, is stored as `d`: the scale of float32 rounding in this recurrence, from which the GPU test's tolerance
is taken.

Session: 700 frames (crosses the low-pass buffer's truncation at 300 samples twice), 2 drones, O_max = 4, irregular dt around
1/60 s, frames without one drone, frames without any object (the clock still advances), a decoy with the same droneIndex
0.3 m from the true object on most frames, one reset() half way.  Asserted: on every frame the nearest and second-nearest
candidate distances differ by more than 1e-3 m and both runs choose identically, so float32 rounding cannot flip an
association; every drone has more than 450 valid frames.

The file holds arrays only.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_harness import REFERENCE_API, reference_available  # noqa: E402

F, D, O_MAX, RESET_FRAME, SEED = 700, 2, 4, 350, 11
OUT = os.path.join(ROOT, "tests", "golden", "objfilter_two_drones.npz")


class _Clock:
    now = 0.0


def _stub_cv2(dtype):
    class KalmanFilter:
        def __init__(self, dynam, measure):
            self._m = {"transitionMatrix": np.eye(dynam, dtype=dtype), "measurementMatrix": np.zeros((measure, dynam), dtype=dtype),
                       "processNoiseCov": np.eye(dynam, dtype=dtype), "measurementNoiseCov": np.eye(measure, dtype=dtype),
                       "statePre": np.zeros((dynam, 1), dtype=dtype), "statePost": np.zeros((dynam, 1), dtype=dtype),
                       "errorCovPre": np.zeros((dynam, dynam), dtype=dtype), "errorCovPost": np.zeros((dynam, dynam), dtype=dtype)}

        def predict(self):
            m = self._m
            A = m["transitionMatrix"]
            m["statePre"] = A @ m["statePost"]
            m["errorCovPre"] = (A @ m["errorCovPost"]) @ A.T + m["processNoiseCov"]
            m["statePost"] = m["statePre"].copy()
            m["errorCovPost"] = m["errorCovPre"].copy()
            return m["statePre"]

        def correct(self, z):
            m = self._m
            H = m["measurementMatrix"]
            z = np.asarray(z, dtype=dtype).reshape(-1, 1)
            t2 = H @ m["errorCovPre"]
            t3 = t2 @ H.T + m["measurementNoiseCov"]
            gain = np.linalg.solve(t3, t2).astype(dtype).T
            t5 = z - H @ m["statePre"]
            m["statePost"] = m["statePre"] + gain @ t5
            m["errorCovPost"] = m["errorCovPre"] - gain @ t2
            return m["statePost"]

    def member(name):
        return property(lambda self: self._m[name], lambda self, v: self._m.__setitem__(name, np.array(v, dtype=dtype)))
    for name in ("transitionMatrix", "measurementMatrix", "processNoiseCov", "measurementNoiseCov", "statePre", "statePost",
                 "errorCovPre", "errorCovPost"):
        setattr(KalmanFilter, name, member(name))
    mod = types.ModuleType("cv2")
    mod.KalmanFilter = KalmanFilter
    return mod


def _load_reference(dtype):
    """A fresh import of the reference's two modules against a cv2 stub of `dtype`."""
    for name in ("KalmanFilter", "LowPassFilter", "cv2"):
        sys.modules.pop(name, None)
    sys.modules["cv2"] = _stub_cv2(dtype)
    if REFERENCE_API not in sys.path:
        sys.path.insert(0, REFERENCE_API)
    import KalmanFilter as ref_module
    ref_module.time = types.SimpleNamespace(time=lambda: _Clock.now)
    return ref_module.KalmanFilter


def make_session():
    rng = np.random.default_rng(SEED)
    t = 1.7e9 + np.cumsum(rng.uniform(0.012, 0.022, F))
    reset_t = 0.5 * (t[RESET_FRAME - 1] + t[RESET_FRAME])
    s = t - t[0]
    true = np.zeros((F, D, 3))
    true[:, 0] = np.stack([np.cos(0.8 * s), np.sin(0.8 * s), 1.0 + 0.2 * np.sin(0.5 * s)], axis=1)
    true[:, 1] = np.stack([-0.5 + 0.6 * np.sin(0.6 * s), 0.3 + 0.4 * np.sin(0.9 * s + 1.0), 0.8 + 0.1 * np.cos(0.7 * s)], axis=1)
    true += rng.normal(0.0, 1e-3, true.shape)
    head = np.stack([0.9 * np.sin(0.4 * s), 0.7 * np.cos(0.3 * s)], axis=1) + rng.normal(0.0, 1e-2, (F, D))
    decoy_dir = np.array([[0.0, 0.3, 0.0], [0.3, 0.0, 0.0]])
    present = np.ones((F, D), dtype=bool)
    present[rng.random(F) < 0.06, 0] = False
    present[rng.random(F) < 0.08, 1] = False
    present[200:240, 1] = False                  # a drone away for 40 frames
    present[rng.random(F) < 0.03] = False        # frames without any object
    present[0] = present[RESET_FRAME] = True
    decoy = present & (rng.random((F, D)) < np.array([0.8, 0.4]))
    pos = np.zeros((F, O_MAX, 3))
    heading = np.zeros((F, O_MAX))
    drone = np.full((F, O_MAX), -1, dtype=np.int32)
    n_obj = np.zeros(F, dtype=np.int32)
    for f in range(F):
        objs = []
        for d in range(D):
            if present[f, d]:
                objs.append((true[f, d], head[f, d], d))
            if decoy[f, d]:
                objs.append((true[f, d] + decoy_dir[d] + rng.normal(0.0, 1e-3, 3), head[f, d] + 0.5, d))
        for j, k in enumerate(rng.permutation(len(objs))):   # list order is arbitrary: a decoy may come first
            pos[f, j], heading[f, j], drone[f, j] = objs[k]
        n_obj[f] = len(objs)
    return t, reset_t, pos, heading, drone, n_obj


def run(dtype, t, reset_t, pos, heading, drone, n_obj):
    kf = _load_reference(dtype)(D)
    chosen = np.full((F, D), -1, dtype=np.int32)
    fpos, fvel, fhead = (np.full(s, np.nan) for s in ((F, D, 3), (F, D, 3), (F, D)))
    gap = np.full((F, D), np.inf)
    for f in range(F):
        if f == RESET_FRAME:
            _Clock.now = reset_t
            kf.reset()
        _Clock.now = t[f]
        objects = [{"pos": pos[f, j].copy(), "heading": np.float64(heading[f, j]), "droneIndex": int(drone[f, j])}
                   for j in range(n_obj[f])]
        for r in kf.predict_location(objects):
            d = r["droneIndex"]
            assert r["pos"].dtype == dtype and r["vel"].dtype == dtype
            fpos[f, d], fvel[f, d], fhead[f, d] = r["pos"], r["vel"], r["heading"]
            # the association, on the values the reference computed it from (KalmanFilter.py:76-77; "pos" IS the prediction)
            cand = [j for j in range(n_obj[f]) if drone[f, j] == d]
            dist = np.sqrt(np.sum((pos[f, cand] - r["pos"]) ** 2, axis=1))
            chosen[f, d] = cand[int(np.argmin(dist))]
            if len(cand) > 1:
                ds = np.sort(dist)
                gap[f, d] = ds[1] - ds[0]
    return chosen, fpos, fvel, fhead, gap


def main():
    assert reference_available(), "the reference checkout is needed to (re)generate this fixture"
    session = make_session()
    c32, p32, v32, h32, g32 = run(np.float32, *session)
    c64, p64, v64, h64, g64 = run(np.float64, *session)
    assert np.array_equal(c32, c64), "float32 and float64 runs associate differently"
    assert min(g32.min(), g64.min()) > 1e-3, (g32.min(), g64.min())
    assert ((c32 >= 0).sum(axis=0) > 450).all(), (c32 >= 0).sum(axis=0)
    d = np.array([0.0] + [np.nanmax(np.abs(a - b)) for a, b in ((p32, p64), (v32, v64), (h32, h64))])
    t, reset_t, pos, heading, drone, n_obj = session
    np.savez_compressed(OUT, t=t, pos=pos, heading=heading, drone=drone, n_obj=n_obj, reset_frame=np.array([RESET_FRAME]),
                        reset_t=np.array([reset_t]), chosen=c32, fpos=p32.astype(np.float32), fvel=v32.astype(np.float32),
                        fheading=h32, chosen64=c64, fpos64=p64, fvel64=v64, fheading64=h64, d=d)
    print(f"{OUT}: valid frames per drone {(c32 >= 0).sum(axis=0).tolist()}, frames with a decoy {(np.isfinite(g32)).sum(axis=0).tolist()}, "
          f"smallest gap {min(g32.min(), g64.min()):.4f} m, d (chosen, fpos, fvel, fheading) = {d.tolist()}")


if __name__ == "__main__":
    main()
