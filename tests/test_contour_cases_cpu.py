"""The crafted masks of tests/contour_cases.py on the CPU: the two references of the contour stage agree on them -- the C
oracle's sequential Suzuki-Abe scan (oracle/c/blob_oracle.c, bo_centroids_from_masks) and the Python restatement of
findContours + moments (oracle/cv_image_restate.py through oracle/blob_oracle.contours_from_mask) -- and every case reaches
the edge its name claims, by counts that neither reference computes (contour_cases.count_pairs / count_contours).
tests/test_gpu_contour_kernel.py then holds the device against the C oracle on the same table.

The Python restatement runs in the interpreter, so it sees the named cases and strided samples of the generated sets; the
C oracle sees everything."""
import numpy as np
import pytest

import contour_cases as cc
from oracle import blob_oracle, c_oracle

M_BIG = 1024


def assert_references_agree(masks, label):
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    counts, ncont, blobs, bbox = c_oracle.contours_from_masks(masks, M_BIG)
    for i, m in enumerate(masks):
        n_py, pts, boxes = blob_oracle.contours_from_mask(m * 255)
        where = "%s[%d]" % (label, i)
        assert ncont[i] == n_py, where
        assert counts[i] == len(pts) <= M_BIG, where
        assert np.array_equal(blobs[i, :len(pts)], np.asarray(pts, dtype=np.float32).reshape(-1, 2)), where
        assert np.array_equal(bbox[i, :len(pts)], np.asarray(boxes, dtype=np.int16).reshape(-1, 4)), where   # C boxes = vertex min / max


NAMED = cc.all_named()


@pytest.mark.parametrize("case", NAMED, ids=repr)
def test_named_case_is_what_its_name_claims(case):
    pairs, conts = cc.count_pairs(case.masks), cc.count_contours(case.masks)
    counts, ncont, _, _ = c_oracle.contours_from_masks(case.masks, M_BIG)
    if case.pairs is not None:
        assert np.array_equal(pairs, case.pairs)
    if case.min_pairs is not None:
        assert pairs.min() >= case.min_pairs
    assert np.array_equal(conts, case.contours)
    assert np.array_equal(ncont, case.contours)          # the reference finds as many borders as the topology has
    assert np.array_equal(counts, case.centroids)
    P, N = cc.large_tables(case.S)
    assert cc.lds_bytes(case.S, P, N) <= cc.LDS_CAP
    if case.overflows:
        assert pairs.min() > P or conts.min() > N
    else:                                                # no GPU test may pass by overflowing
        assert pairs.max() <= P and conts.max() <= N and counts.max() <= M_BIG


def test_large_tables():
    assert cc.large_tables(320) == cc.large_tables(352) == cc.LARGE_TABLES and cc.large_tables(832) == (4096, 256)


@pytest.mark.parametrize("case", NAMED, ids=repr)
def test_references_agree_on_named(case):
    assert_references_agree(case.masks, repr(case))


def test_references_agree_on_exhaustive_samples():
    whole = cc.patterns4(np.arange(0, 1 << 16, 37))
    assert_references_agree(whole, "4x4 as the image")
    assert_references_agree(cc.embed(cc.patterns4(np.arange(5, 1 << 16, 509)), cc.SEAM_S, cc.SEAM_Y, cc.SEAM_X), "4x4 across the seam")
    codes = cc.offset_sample_codes()
    for k, ((y, x), masks) in enumerate(cc.offset_batches()):
        assert_references_agree(masks[k % 7::293], "4x4 at y %d x %d" % (y, x))
    assert len(set(codes.tolist())) == cc.OFFSET_SAMPLE


def test_references_agree_on_random_samples():
    assert_references_agree(cc.random8()[::10], "8x8")
    for S in cc.RANDOM_SIZES:
        assert_references_agree(cc.random_sized(S)[::24], "random %d" % S)


def test_generated_sets_fit_their_tables():
    # every border crosses at least two horizontal pairs (at its leftmost and its rightmost pixel) and a pair lies on one
    # border only: contours <= pairs / 2, which bounds the small sets without labelling 115 000 masks
    P4, N4 = cc.SMALL_TABLES_4X4
    p = cc.patterns4()
    assert cc.count_pairs(p).max() == 16 <= P4 and 16 // 2 <= N4 and 4 * N4 <= P4
    assert (2 * cc.count_contours(p[::64]) <= cc.count_pairs(p[::64])).all()
    # embedding in a larger zero image changes neither count except at the image border, where pairs stay pairs
    lo, seam = next(cc.exhaustive_chunks(cc.SEAM_S))
    assert np.array_equal(cc.count_pairs(seam), cc.count_pairs(p[lo:lo + len(seam)]))
    assert seam[:, :, cc.SEAM_X:cc.SEAM_X + 4].any() and not seam[:, :, :cc.SEAM_X].any() and cc.SEAM_X < 64 < cc.SEAM_X + 3
    P, N = cc.LARGE_TABLES
    r8 = cc.random8()
    counts, ncont, _, _ = c_oracle.contours_from_masks(r8, 16)
    assert len(r8) == 50000 and cc.count_pairs(r8).max() <= 64 and counts.max() <= 16
    assert ncont.max() >= 10                          # nesting and shared pixels do occur
    for S in cc.RANDOM_SIZES:
        m = cc.random_sized(S)
        assert m.shape == (cc.RANDOM_SIZED_N, S, S) and m[:, -1, :].any() and m[:, :, -1].any()
        counts, _, _, _ = c_oracle.contours_from_masks(m, M_BIG)
        assert cc.count_pairs(m).max() <= P and cc.count_contours(m).max() <= N and counts.max() <= M_BIG


@pytest.mark.parametrize("tier", cc.CAP_TIERS, ids=lambda t: "%d_%d_then_%d_%d" % (t[0] + t[1]))
def test_cap_cases_hit_their_caps(tier):
    (P1, N1), (P2, N2) = tier
    masks, pairs, conts = cc.cap_batch(*tier)
    assert np.array_equal(cc.count_pairs(masks), pairs) and np.array_equal(cc.count_contours(masks), conts)
    for P, N in tier:
        assert ((pairs == P) & (conts <= N)).any() and ((pairs == P + 2) & (conts <= N)).any()      # at the pair cap, one pixel over
        assert ((conts == N) & (pairs <= P)).any() and ((conts == N + 1) & (pairs <= P)).any()      # at the contour cap, one over
    fits1, fits2 = (pairs <= P1) & (conts <= N1), (pairs <= P2) & (conts <= N2)
    assert fits1.sum() >= 4 and (fits2 & ~fits1).sum() >= 2 and (~fits2).sum() >= 2                 # a mixed batch
    assert cc.lds_bytes(cc.CAP_S, P2, N2) <= cc.LDS_CAP
    _, ncont, _, _ = c_oracle.contours_from_masks(masks, M_BIG)
    assert np.array_equal(ncont, conts)
