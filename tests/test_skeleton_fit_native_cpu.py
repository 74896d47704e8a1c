"""Memory safety of the host's part of "skeleton fit" on the CPU (csrc/skeleton_fit_host.hpp: the argument rules of
mocap_fit_skeleton, the joints' check it shares with "joint poses", the directed joints and the forest's elimination tables, plain
C++): tests/native/skeleton_fit_host_check.cpp is built as a stand-alone program with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a process of its own, on arguments at every rule's edge and on joints whose arrays are heap
blocks of exactly the contract's size; what it prints is compared entry by entry with the statement's tables
(tests/skeleton_fit_reference.py).  Nothing loaded into python runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np

import joint_pose_reference as jp
import skeleton_fit_reference as sk
from conftest import ROOT

INF, NAN = float("inf"), float("nan")


def _build(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "skeleton_fit_host_check")
    src = os.path.join(ROOT, "tests", "native", "skeleton_fit_host_check.cpp")
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


def _line(B, joints):
    row = [B, len(joints)]
    for j in joints:
        row += [int(j["a"]), int(j["b"]), int(j["kind"]), *[float(v) for k in ("c_a", "c_b", "axis_a", "axis_b") for v in j[k]]]
    return row


def _random_joint(rng, a, b, n):
    u, v = rng.standard_normal(3), rng.standard_normal(3)
    return _joint(a, b, jp.HINGE if n % 2 else jp.BALL, rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.1, 0.1, 3), u / np.linalg.norm(u), v / np.linalg.norm(v))


def test_argument_rules_and_the_forests_tables_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path)
    # (B, J, axis_len, w_joint, iters) -> stands?
    args = [((5, 4, 0.1, 1.0, 8), 1), ((2, 1, 5e-324, 5e-324, 1), 1), ((64, 63, 1e300, 1e300, 16), 1), ((1, 1, 0.1, 1.0, 8), 0),
            ((65, 4, 0.1, 1.0, 8), 0), ((5, 0, 0.1, 1.0, 8), 0), ((5, 5, 0.1, 1.0, 8), 0), ((5, 4, 0.0, 1.0, 8), 0), ((5, 4, NAN, 1.0, 8), 0),
            ((5, 4, INF, 1.0, 8), 0), ((5, 4, -0.1, 1.0, 8), 0), ((5, 4, 0.1, 0.0, 8), 0), ((5, 4, 0.1, NAN, 8), 0), ((5, 4, 0.1, INF, 8), 0),
            ((5, 4, 0.1, -1.0, 8), 0), ((5, 4, 0.1, 1.0, 0), 0), ((5, 4, 0.1, 1.0, 17), 0), ((5, 4, 0.1, 1.0, -1), 0)]
    got = _run(exe, "args", [row for row, _ in args])
    assert [int(g[0]) for g in got] == [want for _, want in args]
    assert all((sk.validate(B, [_joint()] * J, L, w, it) is None) == bool(want) for (B, J, L, w, it), want in args if J == 1)

    rng = np.random.default_rng(7)
    chain = [_random_joint(rng, b + 1, b, b) for b in range(63)]                      # a chain of 64, the child named first
    star = [_random_joint(rng, 0, b, b) for b in range(1, 64)]                        # a star of 64
    star_high = [_random_joint(rng, b, 63, b) for b in range(63)]                     # ... whose hub is the highest body: its root is body 0
    two = [_random_joint(rng, 4, 2, 0), _random_joint(rng, 5, 1, 1), _random_joint(rng, 2, 6, 2), _random_joint(rng, 3, 1, 3)]  # 2-4, 2-6; 1-5, 1-3; 0 alone
    single = [_joint(1, 0, jp.HINGE)]
    ball_nan = [_joint(0, 1, jp.BALL, axis_a=(NAN, INF, 0.0), axis_b=(NAN, NAN, NAN))]      # a BALL's axes are not read
    stands = [(64, chain), (64, star), (64, star_high), (7, two), (2, single), (2, ball_nan), (9, two)]

    good = two

    def bad(i, **kw):
        return [dict(j, **kw) if n == i else j for n, j in enumerate(good)]

    refused = [bad(3, a=4, b=6),                                          # a cycle 2 - 4 - 6 - 2
               bad(3, a=2, b=4), bad(3, a=4, b=2),                        # a duplicate pair, either way round
               bad(0, kind=2), bad(0, kind=0), bad(0, kind=5),            # FIXED and every other kind
               bad(1, axis_a=(1.0, 0.0, 0.002)), bad(1, axis_b=(0.0, 0.0, 0.0)), bad(1, axis_a=(NAN, 0.0, 1.0)), bad(3, axis_b=(0.0, INF, 0.0)),
               bad(0, a=7), bad(0, b=-1), bad(0, a=2), bad(0, c_a=(0.0, NAN, 0.0)), bad(3, c_b=(INF, 0.0, 0.0))]
    rows = [_line(B, j) for B, j in stands] + [_line(7, j) for j in refused]
    got = _run(exe, "table", rows)
    assert [int(g[0]) for g in got] == [1] * len(stands) + [0] * len(refused)
    assert all(sk.validate(B, j, 0.1, 1.0, 8) is None for B, j in stands) and all(sk.validate(7, j, 0.1, 1.0, 8) is not None for j in refused)

    for g, (B, joints) in zip(got, stands):
        J = len(joints)
        tb = sk.forest(B, joints)
        ints = [int(v) for v in g[1:B + 2 + 4 * B + J]]
        first, rest = ints[:B + 1], ints[B + 1:]
        assert first == [sum(len(tb["dirs"][y]) for y in range(b)) for b in range(B + 1)]
        for n, key in enumerate(("parent", "depth", "joint_up", "order")):
            assert rest[n * B:(n + 1) * B] == tb[key], key
        assert rest[4 * B:] == tb["child_of"]
        e = g[B + 2 + 4 * B + J:]
        want = [d for y in range(B) for d in tb["dirs"][y]]
        assert len(e) == 16 * len(want) == 16 * 2 * J
        for n, (j, x, hinge, up, c_y, ax_y, c_x, ax_x) in enumerate(want):
            assert [int(v) for v in e[16 * n:16 * n + 4]] == [j, x, jp.HINGE if hinge else jp.BALL, int(up)]
            vals = np.array([float(v) for v in e[16 * n + 4:16 * n + 16]])
            assert vals.tobytes() == np.array(c_y + ax_y + c_x + ax_x).tobytes(), (n, j)

    # the tables spelled out: the chain is the deepest elimination, the star's leaves go in ascending order, a root is its component's lowest body
    tb = sk.forest(64, chain)
    assert tb["parent"] == [-1] + list(range(63)) and tb["depth"] == list(range(64)) and tb["order"] == list(range(63, -1, -1))
    tb = sk.forest(64, star)
    assert tb["order"] == list(range(1, 64)) + [0] and tb["joint_up"] == [-1] + list(range(63))
    tb = sk.forest(64, star_high)
    assert tb["parent"] == [-1, 63] + [63] * 61 + [0] and tb["depth"][63] == 1 and tb["depth"][1] == 2 and tb["order"][-2:] == [63, 0]
    tb = sk.forest(7, two)
    assert tb["parent"] == [-1, -1, -1, 1, 2, 1, 2] and tb["order"] == [3, 4, 5, 6, 0, 1, 2] and tb["child_of"] == [4, 5, 6, 3]
