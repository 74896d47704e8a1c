"""Memory safety of the host's part of "joints" on the CPU (csrc/joints_host.hpp: the argument rules of mocap_find_joints and the
joint table of mocap_joint_series, plain C++): tests/native/joints_host_check.cpp is built as a stand-alone program with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a process of its own, on arguments at every rule's edge and on joint tables
whose arrays are heap blocks of exactly the contract's size; what it prints is compared with the contract's rules written out here.
Nothing loaded into python runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np

import joints_reference as jr
from conftest import ROOT

INF, NAN = float("inf"), float("nan")


def _build(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler (g++) found"
    exe = str(tmp_path / "joints_host_check")
    src = os.path.join(ROOT, "tests", "native", "joints_host_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", src, "-o", exe])
    return exe


def _run(exe, mode, rows):
    text = "\n".join(" ".join(repr(x) for x in row) for row in rows) + "\n"
    res = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{len(rows)} lines ok" in res.stderr
    return [[float(x) for x in line.split()] for line in res.stdout.splitlines()]


def _joint(a=0, b=1, kind=jr.BALL, c_a=(0.1, 0.2, 0.3), c_b=(-0.1, 0.0, 0.2), axis_b=(0.0, 0.0, 1.0), q_ref=(1.0, 0.0, 0.0, 0.0)):
    return [a, b, kind, *c_a, *c_b, *axis_b, *q_ref]


def test_argument_rules_and_joint_tables_under_asan_and_ubsan(tmp_path):
    exe = _build(tmp_path)
    # mocap_find_joints: (n_frames, B, min_common, tol_rank, max_sep) -> stands?
    find = [((100, 5, 30, 1e-4, INF), 1), ((1, 2, 6, 0.5, 1e-300), 1), ((1 << 22, 64, 6, 1e-300, 0.01), 1),
            ((0, 5, 30, 1e-4, INF), 0), (((1 << 22) + 1, 5, 30, 1e-4, INF), 0), ((100, 1, 30, 1e-4, INF), 0), ((100, 65, 30, 1e-4, INF), 0),
            ((100, 5, 5, 1e-4, INF), 0), ((100, 5, 30, 0.0, INF), 0), ((100, 5, 30, 1.0, INF), 0), ((100, 5, 30, NAN, INF), 0),
            ((100, 5, 30, INF, INF), 0), ((100, 5, 30, -1e-4, INF), 0), ((100, 5, 30, 1e-4, 0.0), 0), ((100, 5, 30, 1e-4, NAN), 0),
            ((100, 5, 30, 1e-4, -INF), 0), ((100, 5, 30, float(np.nextafter(1.0, 0.0)), 5e-324), 1)]
    got = _run(exe, "find", [row for row, _ in find])
    assert [int(g[0]) for g in got] == [want for _, want in find]
    # mocap_joint_series: (B, J, joints) -> the table, or refused
    s = 0.5 ** 0.5
    rng = np.random.default_rng(1)
    full = []
    for j in range(64):
        q = rng.standard_normal(4)
        full += _joint(a=j % 7, b=7 + j % 5, kind=j % 5, c_a=rng.uniform(-1, 1, 3).tolist(), c_b=rng.uniform(-1, 1, 3).tolist(),
                       axis_b=rng.uniform(-1, 1, 3).tolist(), q_ref=(q / np.linalg.norm(q)).tolist())
    table = [([5, 1, *_joint()], True), ([5, 2, *_joint(), *_joint(a=4, b=0, kind=jr.HINGE, q_ref=(s, 0.0, -s, 0.0))], True),
             ([12, 64, *full], True),
             ([5, 1, *_joint(kind=jr.BALL, axis_b=(NAN, INF, 0.0))], True),                # the axis is read under HINGE alone
             ([5, 1, *_joint(q_ref=(1.0 + 4e-7, 0.0, 0.0, 0.0))], True),                  # |q|^2 - 1 = 8e-7
             ([5, 0], False), ([5, 65, *(full + _joint())], False), ([5, 1, *_joint(a=5)], False), ([5, 1, *_joint(b=-1)], False),
             ([5, 1, *_joint(a=2, b=2)], False), ([5, 1, *_joint(kind=5)], False), ([5, 1, *_joint(kind=-1)], False),
             ([5, 1, *_joint(c_a=(0.0, NAN, 0.0))], False), ([5, 1, *_joint(c_b=(0.0, 0.0, INF))], False),
             ([5, 1, *_joint(kind=jr.HINGE, axis_b=(0.0, NAN, 1.0))], False), ([5, 1, *_joint(q_ref=(NAN, 0.0, 0.0, 0.0))], False),
             ([5, 1, *_joint(q_ref=(1.001, 0.0, 0.0, 0.0))], False), ([5, 1, *_joint(q_ref=(0.0, 0.0, 0.0, 0.0))], False),
             ([5, 2, *_joint(), *_joint(q_ref=(2.0, 0.0, 0.0, 0.0))], False)]
    got = _run(exe, "table", [row for row, _ in table])
    for g, (row, stands) in zip(got, table):
        assert bool(g[0]) == stands, row[:2]
        if stands:
            want = np.array(row[2:], dtype=np.float64).reshape(row[1], 16)
            have = np.array(g[1:]).reshape(row[1], 16)
            hinge = want[:, 2] == jr.HINGE
            want[~hinge, 9:12] = 0.0                            # an axis that is not read is tabulated as zero
            assert have.tobytes() == want.tobytes()
