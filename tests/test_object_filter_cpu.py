"""No GPU: the object filter's ABI surface, its fixture (tests/golden/objfilter_two_drones.npz, written by
scripts/make_objfilter_golden.py from the reference's own KalmanFilter.py / LowPassFilter.py) and the identity the low-pass kernel
rests on: lfilter from a zero state over a buffer, last sample kept = dot product of the buffer with the impulse response."""
import os
import re
import subprocess

import numpy as np
from scipy.signal import butter, lfilter

from conftest import PKG, ROOT, load_golden

SYMBOLS = ("mocap_set_object_filter", "mocap_reset_object_filter", "mocap_filter_objects", "mocap_filter_objects_dev",
           "mocap_track_frame_filtered", "mocap_track_frame_filtered_dev")


def test_header_declares_and_library_exports_the_object_filter():
    header = open(os.path.join(ROOT, "include", "mocap_core.h")).read()
    from mocap_core import capi
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(mocap_ctx\* ctx," % name, header), name
        assert name in capi.SIGNATURES, name
    lib = os.path.join(PKG, "lib", "libmocap_core.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r" T %s$" % name, exported, re.M), name


def test_fixture_satisfies_the_generators_conditions():
    g = load_golden("objfilter_two_drones")
    F, O_max = g["pos"].shape[:2]
    assert F == 700 and O_max == 4 and g["chosen"].shape == (F, 2)
    assert np.array_equal(g["chosen"], g["chosen64"])                    # float32 rounding flips no association
    assert ((g["chosen"] >= 0).sum(axis=0) > 450).all()
    assert (np.diff(g["t"]) > 0).all() and (g["n_obj"] == 0).sum() > 5 and g["n_obj"].max() <= O_max
    assert g["t"][g["reset_frame"][0] - 1] < g["reset_t"][0] < g["t"][g["reset_frame"][0]]
    gaps = []
    for f in range(F):
        for d in range(2):
            cand = [j for j in range(g["n_obj"][f]) if g["drone"][f, j] == d]
            assert (g["chosen"][f, d] in cand) if cand else (g["chosen"][f, d] == -1)
            if len(cand) > 1:   # "pos" is the prediction the reference measured the candidates' distances to
                for key in ("fpos", "fpos64"):
                    dist = np.sort(np.sqrt(np.sum((g["pos"][f, cand] - g[key][f, d]) ** 2, axis=1)))
                    gaps.append(dist[1] - dist[0])
    assert len(gaps) > 2 * 500 and min(gaps) > 1e-3
    for k, key in enumerate(("chosen", "fpos", "fvel", "fheading")):
        diff = np.abs(g[key].astype(np.float64) - g[key + "64"])
        assert np.nanmax(diff) == g["d"][k], key
    assert 0 < g["d"][1] < 1e-2 and 0 < g["d"][2] < 1e-2 and g["d"][3] == 0.0   # the heading never meets the Kalman state


def test_lowpass_is_a_dot_product_with_the_impulse_response():
    """Replays the reference's buffer schedule (append; filter; at >= 300 rows keep the newer 150) over the headings the fixture's
    session chose, as sum_k h[k] x[n-k] over the window: equal to the reference's float64 output to 1e-12."""
    g = load_golden("objfilter_two_drones")
    b, a = butter(5, 20 / (60.0 / 2), btype="low")
    B = 300
    h = lfilter(b, a, np.r_[1.0, np.zeros(B - 1)])
    worst, lengths = 0.0, set()
    for d in range(2):
        hist, n = [], 0
        for f in np.nonzero(g["chosen"][:, d] >= 0)[0]:
            hist.append(g["heading"][f, g["chosen"][f, d]])
            n += 1
            lengths.add(n)
            window = np.array(hist[-n:])[::-1]
            worst = max(worst, abs(float(np.dot(h[:n], window)) - g["fheading64"][f, d]))
            if n >= B:
                n = -((-B) // 2)
    assert 1 in lengths and B in lengths and min(x for x in lengths if x > 150) == 151
    assert worst <= 1e-12 * max(1.0, np.abs(g["heading"]).max()), worst
