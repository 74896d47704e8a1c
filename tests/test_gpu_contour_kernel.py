"""blob_contour_kernel (csrc/blob_kernels.hip) on the crafted masks of tests/contour_cases.py, against the C oracle's
sequential Suzuki-Abe scan (oracle/c/blob_oracle.c), through the test-only probe tests/native/libmocap_contourprobe.so, which
compiles the product's blob_kernels.hip as it stands and calls its launch_blob_contours on caller-supplied 1-bit masks.  The
rest of the suite reaches the kernel only behind the 9x9 Gaussian of whole camera frames.

Everything is integers and is compared exactly, the whole output arrays at once: counts = min(centroids, M_max), blobs[:count]
bit for bit, n_contours, status (POINT_OVERFLOW iff centroids > M_max) and, with boxes, bbox[:count].  The outputs go in filled
with a sentinel; slots at and beyond `count` must come back holding it, and so must every array of an image a pass does not
work on.  tests/test_contour_cases_cpu.py shows that the oracle agrees with the Python restatement of findContours on the same
table and that no case passes here by overflowing its tables unless it is meant to.

Masks compared per run of this file, with the largest pair and contour counts among them (NumPy counts of contour_cases):
    exhaustive 4x4      65 536 as the image (S = 4) + 65 536 across the 64-bit word seam (S = 72)    16 pairs, 4 contours
    4x4 at offsets      2 048 patterns x 18 x-offsets x 2 y-offsets = 73 728 (S = 72)               16 pairs, 4 contours
    random 8x8          50 000                                                                      56 pairs, 12 contours
    random S x S        384 each at S = 30, 31, 32, 33, 62, 63, 64, 65 = 3 072                       2 234 pairs, 541 contours
    named topologies    99 masks in 45 cases (17 at 320 and at 832, 11 at 352), each with exact      8 192 pairs (32 rings, = the table),
                        tables without boxes, exact tables with boxes and the largest tables         1 024 contours (isolated pixels, = the table);
                                                                                                    one border of 6 006 pairs (comb), 5 102 (spiral)
    caps                two tiers of 11 masks: 64/16 -> 1 024/128 and 1 024/128 -> 8 192/1 024       each table at its cap and one pixel / contour over
"""
import ctypes
import os

import numpy as np
import pytest

import contour_cases as cc
from oracle import c_oracle

pytestmark = pytest.mark.gpu

FILL = -7                    # no count, coordinate or box is negative
STATUS_FILL = 0x100          # neither status bit
POINT_OVERFLOW, CAP_OVERFLOW = 1, 2
BAD_ARG = -100000
_vp = ctypes.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  (tests/conftest.py, `core`: a process that uses torch's HIP runtime as well must load torch first)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "native", "libmocap_contourprobe.so")
    assert os.path.exists(path), "build it with `make -C tests/native` (__graft_entry__.build does)"
    lib = ctypes.CDLL(path)
    lib.contourprobe_lds_bytes.restype = ctypes.c_size_t
    lib.contourprobe_lds_bytes.argtypes = [ctypes.c_int] * 3
    lib.contourprobe_run.restype = ctypes.c_int
    lib.contourprobe_run.argtypes = [ctypes.c_int, ctypes.c_int64, _vp] + [ctypes.c_int] * 5 + [_vp] * 5
    return lib


class Out:
    """The in/out arrays of one batch, filled with the sentinels."""

    def __init__(self, n, M_max):
        self.M_max = M_max
        self.blobs = np.full((n, M_max, 2), FILL, dtype=np.float32)
        self.counts = np.full(n, FILL, dtype=np.int32)
        self.status = np.full(n, STATUS_FILL, dtype=np.int32)
        self.n_contours = np.full(n, FILL, dtype=np.int32)
        self.bbox = np.full((n, M_max, 4), FILL, dtype=np.int16)


def launch(probe, masks, out, tables, only_overflowed=0, want_bbox=1, packed=None):
    packed = cc.pack(masks) if packed is None else packed
    n, S = packed.shape[:2]
    rc = probe.contourprobe_run(S, n, _p(packed), out.M_max, tables[0], tables[1], only_overflowed, want_bbox, _p(out.blobs),
                                _p(out.counts), _p(out.status), _p(out.n_contours), _p(out.bbox))
    assert rc == 0, "probe returned %d" % rc
    return out


def expected(masks, M_max, overflowed=None, want_bbox=1):
    """What a pass must leave behind: the oracle's arrays where the image fits the tables, the overflow report and
    otherwise the sentinels where it does not."""
    total, ncont, blobs, bbox = c_oracle.contours_from_masks(masks, M_max, fill=FILL)
    exp = Out(len(masks), M_max)
    exp.blobs, exp.bbox = blobs, bbox if want_bbox else exp.bbox
    exp.counts = np.minimum(total, M_max).astype(np.int32)
    exp.status = np.where(total > M_max, POINT_OVERFLOW, 0).astype(np.int32)
    exp.n_contours = ncont.copy()
    if overflowed is not None and overflowed.any():
        o = np.asarray(overflowed)
        exp.blobs[o], exp.bbox[o], exp.counts[o], exp.status[o], exp.n_contours[o] = FILL, FILL, 0, CAP_OVERFLOW, -1
    return exp


def assert_same(got, exp, label):
    for name in ("status", "n_contours", "counts"):
        g, e = getattr(got, name), getattr(exp, name)
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, "%s: %s differs on %d images, first %d: device %d, expected %d" % (label, name, bad.size, bad[0], g[bad[0]], e[bad[0]])
    for name, kind in (("blobs", np.uint32), ("bbox", np.int16)):
        g, e = getattr(got, name).view(kind), getattr(exp, name).view(kind)
        bad = np.flatnonzero((g != e).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs on %d images, first %d:\ndevice\n%s\nexpected\n%s" % (
            label, name, bad.size, bad[0], getattr(got, name)[bad[0], :12], getattr(exp, name)[bad[0], :12])


def run_and_compare(probe, masks, M_max, tables, label, want_bbox=1):
    got = launch(probe, masks, Out(len(masks), M_max), tables, want_bbox=want_bbox)
    assert_same(got, expected(masks, M_max, want_bbox=want_bbox), label)


# ------------------------------------------------------------------------------------------------------------- the probe
def test_probe_refuses_what_the_launcher_would(probe):
    for S, P, N in ((4, 32, 8), (72, 64, 16), (320, 8192, 1024), (352, 1024, 128), (832, 4096, 256)):
        assert probe.contourprobe_lds_bytes(S, P, N) == cc.lds_bytes(S, P, N) <= cc.LDS_CAP
    masks = cc.dots_mask(72, 3)[None]
    packed = cc.pack(masks)
    out = Out(1, 4)

    def rc(packed=packed, S=72, tables=(64, 16), want_bbox=1):
        return probe.contourprobe_run(S, 1, _p(packed), 4, tables[0], tables[1], 0, want_bbox, _p(out.blobs), _p(out.counts),
                                      _p(out.status), _p(out.n_contours), _p(out.bbox))
    beyond = packed.copy()
    beyond[0, 5, 1] |= np.uint64(1) << np.uint64(8)           # x = 72: the first bit beyond the image
    assert rc(packed=beyond) == BAD_ARG
    assert rc(tables=(64, 17)) == BAD_ARG                     # boxes borrow the link tables: 4 N_cap <= P_cap
    assert rc(tables=(8192, 2048)) == BAD_ARG                 # 179 KB of LDS
    assert cc.lds_bytes(72, 8192, 2048) > cc.LDS_CAP
    assert out.counts[0] == FILL and out.status[0] == STATUS_FILL and (out.blobs == FILL).all()
    assert rc(tables=(64, 17), want_bbox=0) == 0 and out.counts[0] == 0 and out.n_contours[0] == 3 and (out.bbox == FILL).all()


# ---------------------------------------------------------------------------------------------- exhaustive small patterns
@pytest.mark.parametrize("S", (4, cc.SEAM_S))
def test_every_4x4_pattern(probe, S):
    for lo, masks in cc.exhaustive_chunks(S):
        run_and_compare(probe, masks, 8, cc.SMALL_TABLES_4X4, "4x4 patterns %d.. at S = %d" % (lo, S))


def test_4x4_patterns_at_word_and_corner_offsets(probe):
    for (y, x), masks in cc.offset_batches():
        run_and_compare(probe, masks, 8, cc.SMALL_TABLES_4X4, "4x4 patterns at y = %d, x = %d" % (y, x))


# ----------------------------------------------------------------------------------------------------- random dense masks
def test_random_8x8(probe):
    run_and_compare(probe, cc.random8(), 16, (128, 32), "random 8x8")      # <= 64 pairs, <= 32 contours; 4 N <= P


@pytest.mark.parametrize("S", cc.RANDOM_SIZES)
def test_random_image_filling(probe, S):
    run_and_compare(probe, cc.random_sized(S), 1024, cc.LARGE_TABLES, "random %dx%d" % (S, S))


# ------------------------------------------------------------------------------------------------------- named topologies
@pytest.mark.parametrize("case", cc.all_named(), ids=repr)
def test_named_topology(probe, case):
    large = cc.large_tables(case.S)
    if case.overflows:
        got = launch(probe, case.masks, Out(len(case.masks), 128), large)
        assert_same(got, expected(case.masks, 128, overflowed=np.ones(len(case.masks), bool)), "%r, largest tables" % case)
        return
    pairs, conts = cc.count_pairs(case.masks), cc.count_contours(case.masks)
    exact = (int(pairs.max()), int(conts.max()))              # the smallest tables that hold the case: both at their cap
    M_max = max(1, int(case.centroids.max()))
    packed = cc.pack(case.masks)
    exp = expected(case.masks, M_max)
    assert_same(launch(probe, None, Out(len(packed), M_max), exact, want_bbox=0, packed=packed),
                expected(case.masks, M_max, want_bbox=0), "%r, tables %d / %d, no boxes" % ((case,) + exact))
    with_boxes = (max(exact[0], 4 * exact[1]), exact[1])
    for tables in (with_boxes, large):                         # the result does not depend on the caps
        assert_same(launch(probe, None, Out(len(packed), M_max), tables, packed=packed), exp, "%r, tables %d / %d" % ((case,) + tables))


# ---------------------------------------------------------------------------------------------------------- point overflow
@pytest.mark.parametrize("name", ("siblings_free_in_hole", "nested_depth_7", "diagonal_holes_2_3"))
def test_point_overflow(probe, name):
    case = next(c for c in cc.named_cases(320) if c.name == name)
    most = int(case.centroids.max())
    for M_max in (most, most - 1, 1):
        exp = expected(case.masks, M_max)
        assert (exp.status == POINT_OVERFLOW).any() == (M_max < most)
        assert_same(launch(probe, case.masks, Out(len(case.masks), M_max), cc.SMALL_TABLES), exp, "%s, M_max = %d" % (name, M_max))


# --------------------------------------------------------------------------------------------------------------------- caps
@pytest.mark.parametrize("tier", cc.CAP_TIERS, ids=lambda t: "%d_%d_then_%d_%d" % (t[0] + t[1]))
def test_cap_protocol(probe, tier):
    first, second = tier
    masks, pairs, conts = cc.cap_batch(first, second)
    over1 = (pairs > first[0]) | (conts > first[1])
    over2 = (pairs > second[0]) | (conts > second[1])
    M_max = 4
    out = launch(probe, masks, Out(len(masks), M_max), first)
    assert_same(out, expected(masks, M_max, overflowed=over1), "first pass")      # the fitting ones are already right
    # second pass, the product's "run again what overflowed": what had fitted goes in under a second sentinel (its status as
    # the first pass left it) and must come back untouched
    done = ~over1
    out.blobs[done], out.bbox[done], out.counts[done], out.n_contours[done] = -9, -9, -9, -9
    launch(probe, masks, out, second, only_overflowed=1)
    exp = expected(masks, M_max, overflowed=over2)
    exp.blobs[done], exp.bbox[done], exp.counts[done], exp.n_contours[done] = -9, -9, -9, -9
    assert_same(out, exp, "second pass")
    assert (over1 & ~over2).sum() >= 2 and over2.sum() >= 2 and done.sum() >= 4


# ------------------------------------------------------------------------------------------------- position in the batch
def test_result_does_not_depend_on_the_position_in_the_batch(probe):
    named = {c.name: c for c in cc.named_cases(320)}
    probe_mask = named["left_walk_outer_hole"].masks[0]
    others = [named["comb"].masks[0], named["nested_depth_7"].masks[0], np.zeros((320, 320), np.uint8), named["checkerboard_46"].masks[0],
              named["thin_ring"].masks[0], named["nested_rings_50"].masks[0], named["isolated_grid_1024"].masks[0]]
    masks = np.stack([probe_mask] + others[:4] + [probe_mask] + others[4:] + [probe_mask])
    where = [0, 5, len(masks) - 1]
    M_max = 3                                                   # the probed mask has 4 centroids: point overflow as well
    over = cc.count_pairs(masks) > cc.LARGE_TABLES[0]
    assert over.sum() == 1
    exp = expected(masks, M_max, overflowed=over)
    runs = [launch(probe, masks, Out(len(masks), M_max), cc.LARGE_TABLES) for _ in range(2)]
    for k, got in enumerate(runs):
        assert_same(got, exp, "run %d" % k)
        for name in ("blobs", "counts", "status", "n_contours", "bbox"):
            a = getattr(got, name)
            assert all(np.array_equal(a[w], getattr(runs[0], name)[0]) for w in where), name
    assert runs[0].status[0] == POINT_OVERFLOW and runs[0].counts[0] == 3 and runs[0].n_contours[0] == 4
