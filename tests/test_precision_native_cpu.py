"""The host's part and the arithmetic of "predicted precision" on the CPU (csrc/precision_host.hpp: the fold of the caller's
coordinates and the argument rules; csrc/precision_math.hpp: the per-point arithmetic, the very text the kernels compile):
tests/native/precision_check.cpp is built as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run as
a process of its own; what it prints is compared entry by entry, bit for bit, with the statement (tests/precision_reference.py).
Nothing loaded into python runs under a sanitizer."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import precision_reference as pr
from conftest import ROOT
from mocap_core import synth

INF, NAN = float("inf"), float("nan")


def _hex(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _dbl(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    out = str(tmp_path_factory.mktemp("precision") / "precision_check")
    src = os.path.join(ROOT, "tests", "native", "precision_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "low-cost-mocap_amd", "csrc"), src,
                           "-o", out])
    return out


def _run(exe, mode, text):
    res = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return res


def _table_text(P):
    return "%d %s\n" % (P.shape[0], " ".join(_hex(v) for v in P.reshape(-1)))


def _rig_table(C, seed=3):
    rig = synth.calibrated_ring_rig(C, seed=seed)
    return rig, pr.camera_table(rig["K"], rig["R"], rig["t"])


def test_the_fold_matches_the_statement_and_null_is_a_copy(exe):
    rng = np.random.default_rng(11)
    for C in (1, 2, 8, 64):
        _, P = _rig_table(max(C, 2))
        P = P[:C]
        frames = [None, np.eye(3, 4), np.concatenate([0.37 * np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], axis=1)]
        for f in frames:
            text = _table_text(P) + ("0\n" if f is None else "1 " + " ".join(_hex(v) for v in f.reshape(-1)) + "\n")
            got = np.array([_dbl(w) for w in _run(exe, "fold", text).stdout.split()]).reshape(C, 3, 4)
            assert got.tobytes() == pr.fold(P, f).tobytes()
            if f is None:
                assert got.tobytes() == P.tobytes()


def test_every_argument_row(exe):
    ident = list(np.eye(3, 4).reshape(-1))

    def common(s, f=None):
        return "common %s %s" % (_hex(s), "0" if f is None else "1 " + " ".join(_hex(v) for v in f)), pr.validate_common(s, f)

    def bad_frame(i, v):
        return ident[:i] + [v] + ident[i + 1:]

    rows = [common(1.0), common(5e-324), common(1e300, ident), common(0.0), common(-1.0), common(NAN), common(INF), common(-INF),
            common(1.0, bad_frame(0, NAN)), common(1.0, bad_frame(11, INF)), common(1.0, bad_frame(5, -INF)), common(1.0, bad_frame(3, 1e300))]
    for w, h, near, far in ((1, 1, 0.0, INF), (640, 480, 0.1, 0.2), (0, 480, 0.0, 1.0), (640, 0, 0.0, 1.0), (-1, 480, 0.0, 1.0), (640, 480, -0.1, 1.0),
                            (640, 480, NAN, 1.0), (640, 480, INF, INF), (640, 480, 1.0, 1.0), (640, 480, 2.0, 1.0), (640, 480, 0.0, NAN),
                            (640, 480, 0.0, 5e-324), (640, 480, -0.0, 1.0)):
        rows.append(("vis %d %d %s %s" % (w, h, _hex(near), _hex(far)), pr.validate_vis(w, h, near, far)))
    for N in (1, pr.MAX_POINTS, 0, -1, pr.MAX_POINTS + 1, 1 << 40):
        rows.append(("points %d" % N, pr.validate_points(N)))
    for F, K in ((0, 1), (3, 16), (pr.MAX_POINTS, 1), (pr.MAX_POINTS // 16, 16), (-1, 16), (3, 0), (3, -1), (pr.MAX_POINTS + 1, 1),
                 (pr.MAX_POINTS // 16 + 1, 16), (1 << 40, 1 << 30)):
        rows.append(("frames %d %d" % (F, K), pr.validate_frames(F, K)))
    for nx, ny, nz, mv, ms in ((1, 1, 1, 0, INF), (1024, 1024, 128, 65, 1e-3), (512, 512, 512, 2, 0.0), (0, 1, 1, 2, 1.0), (1, 0, 1, 2, 1.0),
                               (1, 1, 0, 2, 1.0), (1025, 1, 1, 2, 1.0), (1, 1025, 1, 2, 1.0), (1, 1, 1025, 2, 1.0), (1024, 1024, 129, 2, 1.0),
                               (1024, 1024, 1024, 2, 1.0), (4, 4, 4, -1, 1.0), (4, 4, 4, 2, NAN), (4, 4, 4, 2, -1.0), (-5, 4, 4, 2, 1.0)):
        rows.append(("map %d %d %d %d %s" % (nx, ny, nz, mv, _hex(ms)), pr.validate_map(nx, ny, nz, mv, ms)))
    res = _run(exe, "args", "\n".join(r for r, _ in rows) + "\n")
    assert f"{len(rows)} lines ok" in res.stderr
    assert [int(v) for v in res.stdout.split()] == [int(want is None) for _, want in rows]
    assert sum(want is None for _, want in rows) >= 12 and sum(want is not None for _, want in rows) >= 30

    res = _run(exe, "args", "init 7 5 129\ninit 1024 1 1\n")
    got = np.array([int(v) for v in res.stdout.split()]).reshape(2, pr.SUMMARY)
    assert got[:, :66].tolist() == [[0] * 66] * 2
    assert got[0, 66:].tolist() == [7, -1, 5, -1, 129, -1] and got[1, 66:].tolist() == [1024, -1, 1, -1, 1, -1]


def _cases(C, rng, rig):
    """Points around the rig's centre and the odd ones: behind a camera, far away, not finite."""
    x = rig["centre"][None] + rng.uniform(-1.0, 1.0, (40, 3))
    odd = np.array([[0.0, 0.0, -1.0], [NAN, 0.0, 1.0], [0.0, INF, 1.0], [0.0, 0.0, -INF], [1e200, 0.0, 1.0], [0.0, -1e200, 1.0],
                    [0.0, 0.0, 0.0], [1e-300, 0.0, 1e-300], [0.0, 0.0, 1e9]])
    x = np.concatenate([x, odd + np.array([0.0, 0.0, 0.0])])
    full = (1 << C) - 1
    masks = [full, 3, 1, 0, full ^ 1, 5 % (full + 1) | 1, (0xFFFFFFFFFFFFFFFF << C | 3) & 0xFFFFFFFFFFFFFFFF]
    seen = np.array([masks[i % len(masks)] for i in range(len(x))], dtype=np.uint64)
    return x, seen


@pytest.mark.parametrize("C", [2, 3, 8, 64])
def test_per_point_arithmetic_bit_for_bit(exe, C):
    rng = np.random.default_rng(100 + C)
    rig, P = _rig_table(C)
    frame = np.concatenate([1.7 * np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.standard_normal((3, 1))], axis=1)
    x, seen = _cases(C, rng, rig)
    w, h = rig["image_size"]
    for by_vis, f, sigma in ((0, None, 1.0), (1, None, 0.5), (0, frame, 0.3), (1, frame, 2.0)):
        Pp = pr.fold(P, f)
        xs = x if f is None else (x - f[:, 3]) @ np.linalg.inv(f[:, :3]).T       # (any points do: these stay near the rig)
        text = _table_text(Pp) + "%s %d %s %s %s %s\n%d\n" % (_hex(sigma), by_vis, _hex(w), _hex(h), _hex(0.5), _hex(1e6), len(xs))
        text += "".join("%s %s %s %x\n" % (_hex(p[0]), _hex(p[1]), _hex(p[2]), int(m)) for p, m in zip(xs, seen))
        res = _run(exe, "point", text)
        assert f"{len(xs)} cases ok" in res.stderr
        want = pr.evaluate(Pp, xs, sigma, vis=(w, h, 0.5, 1e6)) if by_vis else pr.evaluate(Pp, xs, sigma, named=pr.named_from_bits(seen, C))
        lines = [line.split() for line in res.stdout.splitlines()]
        assert len(lines) == len(xs)
        for i, g in enumerate(lines):
            assert (int(g[0]), int(g[1]), int(g[2], 16)) == (int(want["info"][i]), int(want["n_views"][i]), int(want["seen"][i])), (i, g[:3])
            vals = np.array([_dbl(v) for v in g[3:]])
            ref = np.concatenate([want["sig"][i], want["axis"][i], want["cov"][i]])
            assert vals.tobytes() == ref.tobytes(), (by_vis, i, vals, ref)
        assert (want["info"] == pr.OK).sum() >= 10        # the comparison is of numbers, not of NaN alone
        assert want["sweeps"][want["info"] == pr.OK].max() < pr.SWEEPS   # the header's limit ends the iteration of no point that is OK
