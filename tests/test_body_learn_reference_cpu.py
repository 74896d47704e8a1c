"""Rigid-body learning without a GPU: the plain statement of the contract (tests/body_learn_reference.py) on a hand-computed
case, on planted captures, against its own 50-digit evaluation, and the two C-ABI symbols (declared, exported, bound)."""
import os
import re
import subprocess

import numpy as np

import body_learn_reference as bl
import rigid_body_reference as rb
from conftest import ROOT


def test_hand_computed_single_frame_is_the_centred_frame():
    xyz = np.full((1, 4, 3), np.nan)
    xyz[0, :3] = [[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [1.0, 4.0, 3.0]]
    ids = np.array([[7, 5, 9, 5]], dtype=np.int32)
    got = bl.learn(xyz, [3], ids, sel=[5, 7, 9], iters=2)
    # markers in sel order: (2,2,3), (1,2,3), (1,4,3); centroid (4/3, 8/3, 3)
    want = np.array([[2.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 4.0, 3.0]]) - np.array([4.0 / 3.0, 8.0 / 3.0, 3.0])
    assert np.abs(got["markers"] - want).max() <= 4e-16
    assert got["ref_frame"] == 0 and got["frames_used"] == 1 and got["frames_valid"] == 1 and got["status"] == 0
    assert got["marker_frames"].tolist() == [1, 1, 1] and got["rms"] <= 1e-15 and got["marker_rms"].max() <= 1e-15
    assert got["pair_mean"][0, 1] == 1.0 and got["pair_mean"][1, 2] == 2.0 and got["pair_mean"][0, 2] == np.sqrt(5.0)
    assert not got["pair_std"].any() and got["pair_frames"][0, 1] == 1


def test_recovers_the_planted_template_within_three_times_the_averaged_noise():
    rng = np.random.default_rng(11)
    q = rb.make_body(rng, 5)
    q = q - q.mean(axis=0)
    cap = bl.make_capture(rng, q, 300, 16, noise=0.0005, dropout=0.25, n_clutter=4)
    got = bl.learn(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"], iters=4)
    assert got["status"] == 0 and got["ref_frame"] == 0
    # what averaging with the TRUE poses would leave: per marker the mean over its frames of R_f^T (p - t_f) - q = R_f^T noise
    slots, _ = bl.gather(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"])
    ideal = 0.0
    for m in range(5):
        fr = np.nonzero(slots[:, m] >= 0)[0]
        y = np.einsum("nji,nj->ni", cap["R"][fr], cap["xyz"][fr, slots[fr, m]] - cap["t"][fr])
        ideal = max(ideal, float(np.linalg.norm(y.mean(axis=0) - q[m])))
    err = float(np.linalg.norm(bl.align(got["markers"], q) - q, axis=1).max())
    print(f"planted template: learned error {err:.3e} m, mean back-mapped noise with the true poses {ideal:.3e} m, ratio {err / ideal:.2f}")
    assert err <= 3.0 * ideal


def test_pair_spread_separates_a_foreign_marker():
    rng = np.random.default_rng(12)
    q = rb.make_body(rng, 4)
    cap = bl.make_capture(rng, q, 200, 16, noise=0.0005, n_clutter=3, foreign=True)
    sel = cap["sel"] + [cap["foreign_id"]]
    got = bl.learn(cap["xyz"], cap["n_pts"], cap["id"], sel, iters=1)
    s = got["pair_std"]
    true_pairs = [s[i, j] for i in range(4) for j in range(i + 1, 4)]
    foreign_pairs = [s[i, 4] for i in range(4)]
    assert min(foreign_pairs) > 10 * max(true_pairs), (foreign_pairs, true_pairs)
    assert max(true_pairs) < 4 * 0.0005 and (got["pair_frames"][np.triu_indices(5, 1)] == 200).all()


def test_float64_and_fifty_digits_agree_on_every_discrete_output():
    rng = np.random.default_rng(13)
    q = rb.make_body(rng, 5)
    cap = bl.make_capture(rng, q, 60, 12, noise=0.0005, dropout=0.3, n_clutter=3)
    bl.displace(cap, range(3, 60, 7), 1, np.array([0.02, -0.01, 0.015]))
    cap["n_pts"][5] = 13                                                             # not a valid frame
    status = np.zeros(60, dtype=np.int32)
    status[9] = 4
    used = []
    for max_rms, iters in ((0.003, 3), (float("inf"), 1)):
        a = bl.learn(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"], status, iters=iters, max_rms=max_rms)
        e = bl.learn_mp(cap["xyz"], cap["n_pts"], cap["id"], cap["sel"], status, iters=iters, max_rms=max_rms)
        assert bl.gate_margin(e, max_rms) > 1e-9
        assert not bl.same_discrete(a, e), bl.same_discrete(a, e)
        assert a["frames_valid"] == 58
        used.append(a["frames_used"])
        errs = bl.field_errors(a, e)
        assert all(d <= 1e-12 for d, _ in errs.values()), errs
    assert 0 < used[0] < used[1] <= 58                                               # the gate rejected the displaced frames
    none = bl.learn(cap["xyz"], cap["n_pts"], cap["id"], [10, 11, 999])
    assert none["status"] == bl.ST_NO_REF and none["ref_frame"] == -1 and not none["markers"].any()


def test_the_two_symbols_are_declared_exported_and_bound():
    from mocap_core import capi
    names = ("mocap_learn_rigid_body", "mocap_learn_rigid_body_dev")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mocap_core.h")).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for n in names:
        assert re.search(r"\bint %s\s*\(" % n, header), n
        assert re.search(r" T %s$" % n, exported, flags=re.M), n
        assert n in capi.SIGNATURES and len(capi.SIGNATURES[n][1]) == 13
    assert "#define MOCAP_LB_RESULT 129" in header and capi.LB_RESULT == 129
    assert (capi.LB_ST_NO_REF, capi.LB_ST_MARKER_UNSEEN) == (1, 2)
