"""Memory safety of the host's part of "joint poses" on the CPU (csrc/joint_pose_host.hpp: the argument rules of mocap_pose_joints, the
forest check of its joints and the table of directed joints with their masks, plain C++): tests/native/joint_pose_host_check.cpp is
built as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own, on arguments at
every rule's edge and on bodies and joints whose arrays are heap blocks of exactly the contract's size; what it prints is compared
with the contract's rules and with the statement's tables (tests/joint_pose_reference.py).  Nothing loaded into python runs under a
sanitizer."""
import os
import shutil
import subprocess

import numpy as np

import joint_pose_reference as jp
from conftest import ROOT

INF, NAN = float("inf"), float("nan")


def _build(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "joint_pose_host_check")
    src = os.path.join(ROOT, "tests", "native", "joint_pose_host_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", src, "-o", exe])
    return exe


def _run(exe, mode, rows):
    text = "\n".join(" ".join(repr(x) for x in row) for row in rows) + "\n"
    res = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(rows)} lines ok" in res.stderr
    return [line.split() for line in res.stdout.splitlines()]


def _joint(a=0, b=1, kind=jp.BALL, c_a=(0.1, 0.2, 0.3), c_b=(-0.1, 0.0, 0.2), axis_a=(0.0, 0.0, 1.0), axis_b=(0.0, 0.6, 0.8)):
    return {"a": a, "b": b, "kind": kind, "c_a": list(c_a), "c_b": list(c_b), "axis_a": list(axis_a), "axis_b": list(axis_b)}


def _line(bodies, joints, axis_len=0.1):
    row = [len(bodies), axis_len, len(joints)]
    for q in bodies:
        pad = np.zeros((8, 3))
        pad[:len(q)] = q
        row += [len(q), *pad.reshape(-1).tolist()]
    for j in joints:
        row += [int(j["a"]), int(j["b"]), int(j["kind"]), *[float(v) for k in ("c_a", "c_b", "axis_a", "axis_b") for v in j[k]]]
    return row


def test_argument_rules_forest_and_masks_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path)
    # (B, J, axis_len, max_rms, max_rounds) -> stands?
    args = [((5, 4, 0.1, INF, 4), 1), ((2, 1, 5e-324, 5e-324, 1), 1), ((64, 63, 1e300, 1.0, 16), 1), ((1, 1, 0.1, INF, 4), 0),
            ((65, 4, 0.1, INF, 4), 0), ((5, 0, 0.1, INF, 4), 0), ((5, 5, 0.1, INF, 4), 0), ((5, 4, 0.0, INF, 4), 0), ((5, 4, NAN, INF, 4), 0),
            ((5, 4, INF, INF, 4), 0), ((5, 4, -0.1, INF, 4), 0), ((5, 4, 0.1, 0.0, 4), 0), ((5, 4, 0.1, NAN, 4), 0), ((5, 4, 0.1, -INF, 4), 0),
            ((5, 4, 0.1, INF, 0), 0), ((5, 4, 0.1, INF, 17), 0), ((5, 4, 0.1, INF, -1), 0)]
    got = _run(exe, "args", [row for row, _ in args])
    assert [int(g[0]) for g in got] == [want for _, want in args]

    # hand-made bodies: a square with its centre line, an L, a body with three collinear markers, one with eight markers
    square = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1, 0.1, 0.0], [0.0, 0.1, 0.0]])
    ell = np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.1, 0.0]])
    line3 = np.array([[-0.1, 0.0, 0.0], [0.0, 0.0, 0.0], [0.15, 0.0, 0.0], [0.0, 0.1, 0.05], [0.03, -0.04, 0.1]])
    rng = np.random.default_rng(5)
    eight = rng.uniform(-0.1, 0.1, (8, 3))
    bodies = [square, ell, line3, eight, ell + 0.01]
    s = 0.5 ** 0.5
    good = [_joint(0, 1, jp.BALL, c_a=(0.05, 0.05, 0.0), c_b=(0.1, 0.0, 0.0)),                      # c_a in the square's plane; c_b on the L's long arm
            _joint(2, 1, jp.HINGE, c_a=(0.04, 0.0, 0.0), c_b=(0.0, 0.0, 0.1), axis_a=(1.0, 0.0, 0.0), axis_b=(0.0, s, s)),   # body 2's axis along its line
            _joint(3, 2, jp.HINGE, c_a=eight[0], c_b=(0.01, 0.1, 0.0), axis_a=(0.0, 0.0, 1.0 + 4e-7), axis_b=(0.0, -1.0, 0.0)),
            _joint(4, 0, jp.BALL, c_a=(0.3, 0.3, 0.3), c_b=(0.0, 0.0, 0.2), axis_a=(NAN, INF, 0.0), axis_b=(NAN, NAN, NAN))]  # a BALL's axes are not read
    star = [_joint(0, b, jp.HINGE if b % 2 else jp.BALL, c_a=rng.uniform(-0.1, 0.1, 3), c_b=rng.uniform(-0.1, 0.1, 3)) for b in range(1, 64)]
    many = [rng.uniform(-0.1, 0.1, (3 + b % 6, 3)) for b in range(64)]
    stands = [(bodies, good, 0.1), (bodies, good[:1], 0.25), (many, star, 0.1), (bodies[:2], good[:1], 1e-3)]

    def bad(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(good)]

    refused = [bad(3, a=1, b=2),                                          # a cycle 0 - 1 - 2 ... closed by (1, 2) again: a duplicate pair
               bad(3, a=0, b=1), bad(3, a=1, b=0),                        # a duplicate pair, either way round
               bad(3, a=3, b=0),                                          # a cycle 0 - 1 - 2 - 3 - 0
               bad(0, kind=2), bad(0, kind=0), bad(0, kind=5),            # FIXED and every other kind
               bad(1, axis_a=(1.0, 0.0, 0.002)), bad(1, axis_b=(0.0, 0.0, 0.0)), bad(1, axis_a=(NAN, 0.0, 1.0)), bad(2, axis_b=(0.0, INF, 0.0)),
               bad(0, a=5), bad(0, b=-1), bad(0, a=1), bad(0, c_a=(0.0, NAN, 0.0)), bad(3, c_b=(INF, 0.0, 0.0)),
               good + [_joint(3, 4)]]                                     # J = B (no forest has that many)
    rows = [_line(b, j, L) for b, j, L in stands] + [_line(bodies, j) for j in refused]
    got = _run(exe, "table", rows)
    assert [int(g[0]) for g in got] == [1] * len(stands) + [0] * len(refused)

    for g, (bs, joints, L) in zip(got, stands):
        B = len(bs)
        first = [int(v) for v in g[1:B + 2]]
        rest = g[B + 2:]
        want = [(y, d) for y in range(B) for d in jp.directed(joints, y, L)]
        assert first == [sum(1 for y, _ in want if y < b) for b in range(B + 1)] and len(rest) == 19 * len(want) == 19 * 2 * len(joints)
        for n, (y, (j, x, hinge, v0, v1, c_x, ax_x)) in enumerate(want):
            e = rest[19 * n:19 * n + 19]
            assert [int(v) for v in e[:3]] == [j, x, jp.HINGE if hinge else jp.BALL]
            vals = np.array([float(v) for v in e[3:15]])
            ref = np.array(v0 + (v1 if hinge else [0.0] * 3) + c_x + (ax_x if hinge else [0.0] * 3))
            assert vals.tobytes() == ref.tobytes(), (y, j)
            bits = jp.dir_mask(bs[y], [v0] + ([v1] if hinge else []))
            mask = sum(int(v) << (64 * k) for k, v in enumerate(e[15:19]))
            assert mask == sum(1 << s for s, ok in enumerate(bits) if ok), (y, j)

    # the masks of the hand-made bodies, spelled out
    g = got[0]
    rest = g[len(bodies) + 2:]
    masks = {}
    for n, (y, d) in enumerate((y, d) for y in range(5) for d in jp.directed(good, y, 0.1)):
        masks[(y, d[0])] = sum(int(v) << (64 * k) for k, v in enumerate(rest[19 * n + 15:19 * n + 19]))
    sq = masks[(0, 0)]                                       # the square through its centre (BALL)
    assert not sq >> 0b0000 & 1 and not sq >> 0b0001 & 1     # no marker, one marker: two points at most
    assert not sq >> 0b0101 & 1 and sq >> 0b0011 & 1         # a diagonal passes through the centre; a side does not
    el = masks[(1, 0)]                                       # the L, the centre on its long arm
    assert not el >> 0b011 & 1 and el >> 0b101 & 1 and el >> 0b110 & 1 and not el >> 0b001 & 1
    ln = masks[(2, 1)]                                       # three collinear markers and a hinge along their line
    assert not ln >> 0b00111 & 1 and not ln >> 0b00001 & 1 and ln >> 0b01000 & 1 and ln >> 0b01001 & 1
    ln2 = masks[(2, 2)]                                      # the same body through a hinge whose axis leaves the line
    assert ln2 >> 0b00001 & 1 and ln2 >> 0b00111 & 1 and not ln2 >> 0 & 1
