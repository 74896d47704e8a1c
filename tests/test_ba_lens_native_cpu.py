"""Memory safety and arithmetic of the lens calibration's per-view code on the CPU (csrc/ba_lens.hpp: bal_lens, bal_view,
bal_undistort, __host__ __device__): tests/native/bal_view_host.cpp is built as a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a process of its own, on the views of a planted capture and on views that are unused, behind
the camera, NaN or down-weighted; what it prints is compared with the NumPy statement (tests/ba_lens_reference.py), which runs the same
operations in the same order.  Nothing loaded into python runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np

import ba_lens_reference as bl
from conftest import ROOT

np.seterr(all="ignore")


def _build(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "bal_view_host")
    src = os.path.join(ROOT, "tests", "native", "bal_view_host.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-Wno-unknown-pragmas", src, "-o", exe])
    return exe


def _run(exe, mode, rows):
    text = "\n".join(" ".join(repr(float(x)) for x in row) for row in rows) + "\n"
    res = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(rows)} lines ok" in res.stderr
    return np.array([[float(x) for x in line.split()] for line in res.stdout.splitlines()])


def test_views_and_undistortion_under_asan_and_ubsan(tmp_path):
    from mocap_core import synth
    exe = _build(tmp_path)
    rig, obs, X0, start = bl.planted_case(4, 40, noise_px=0.3)
    a = bl.intrinsics(rig["K"], rig["dist"] * 0.8)
    a[:, 8] = -0.2
    rows, want = [], []
    for c in range(4):
        cam = np.concatenate([start["R"][c].ravel(), start["t"][c], a[c], np.zeros(3)])
        for p in range(40):
            for hub in (0.0, 2.0):
                X, uv = X0[p] + 0.01, obs[p, c]
                if p == 3:
                    X = X * np.array([1, 1, -1.0])          # behind camera 0 at least
                if p == 5:
                    uv = np.array([np.nan, 1.0])            # an observation nobody would hand over: NaN everywhere, no trap
                if np.isnan(obs[p, c, 0]) and p != 5:
                    continue
                rows.append(np.concatenate([cam, X, uv, [hub]]))
                v = bl.view_terms(bl.FLOAT, start["R"][c].tolist(), start["t"][c].tolist(), a[c].tolist(), [np.array([x]) for x in X],
                                  np.array([uv[0]]), np.array([uv[1]]), hub)
                want.append((bool(v["pos"][0]), bool(v["down"][0]),
                             np.concatenate([[v["rho"][0], v["ru"][0], v["rv"][0]], [x[0] for x in v["Bu"]], [x[0] for x in v["Bv"]],
                                             [x[0] for x in v["Au"]], [x[0] for x in v["Av"]]])))
    got = _run(exe, "views", rows)
    assert got.shape == (len(rows), 2 + 3 + 6 + 28)
    used = down = 0
    for g, (pos, dn, w) in zip(got, want):
        assert bool(g[0]) == pos
        if not pos or np.isnan(w).any():
            continue                                        # a view that is not used contributes nothing: its numbers are not pinned
        used += 1
        down += dn
        assert bool(g[1]) == dn
        assert np.array_equal(g[2:], w), (g[2:] - w)        # the same operations in the same order: the same doubles (a zero's sign aside)
    assert used > 200 and 0 < down < used
    # the Newton inverse: the whole picture's diagonal and border through the reference's lens, NaN, and the identity
    K = np.array(synth.DEFAULT_K)
    t = np.arange(0.0, 320.0, 1.0)
    uv = np.concatenate([np.stack([t, t], 1), np.stack([t, 319 - t], 1), np.stack([t, 0 * t], 1), np.stack([0 * t, t], 1)])
    raw = np.stack(synth.distort_pixels(uv[:, 0], uv[:, 1], K, synth.REFERENCE_DISTORTION), axis=1)
    raw[11, 0] = np.nan
    lens_rows = [np.concatenate([K.ravel(), synth.REFERENCE_DISTORTION, r]) for r in raw]
    flat_rows = [np.concatenate([K.ravel(), np.zeros(5), r]) for r in raw]
    got = _run(exe, "undistort", lens_rows + flat_rows)
    n = len(raw)
    want = bl.undistort(raw[:, None, :], K[None], np.array([synth.REFERENCE_DISTORTION]))[:, 0]
    assert np.isnan(got[11]).all() and np.isnan(got[n + 11]).all()
    ok = np.arange(n) != 11
    assert got[:n][ok].tobytes() == want[ok].tobytes()
    assert np.abs(got[:n][ok] - uv[ok]).max() < 1e-10
    assert got[n:][ok].tobytes() == raw[ok].tobytes()
