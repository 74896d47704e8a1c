"""The restatement of the preview overlays (tests/overlay_reference.py) checked on the CPU: the contour contract -- the
pixels a border trace visits -- against the rule the device kernel implements (a mask pixel with one of its four edge
neighbours off), the line rasteriser and the mark on their edge cases, and the Python constants against the header."""
import os
import re

import numpy as np
import pytest

import overlay_reference as ov
from mocap_core import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shape(rows):
    return np.array([[ch == "#" for ch in r] for r in rows], dtype=np.uint8)


HAND_SHAPES = {
    "single_pixel": _shape(["....", ".#..", "....", "...."]),
    "diagonal_pair": _shape(["....", ".#..", "..#.", "...."]),
    "ring": _shape([".......", ".#####.", ".#####.", ".##.##.", ".#####.", ".#####.", "......."]),
    "blob_inside_hole": _shape(["#########", "#########", "##.....##", "##.....##", "##..#..##", "##..##.##", "##.....##",
                                "#########", "#########"]),
    "on_the_edge": _shape(["......", "###...", "###...", "###...", "......", "......"]),
    "in_the_corner": _shape(["....", "....", "..##", "..##"]),
    "corner_touch": _shape(["......", ".##...", ".##...", "...##.", "...##.", "......"]),
    "full_image": _shape(["#####"] * 5),
    "thick_ring_with_wide_hole": _shape(["#######", "#######", "##...##", "##...##", "##...##", "#######", "#######"]),
}


@pytest.mark.parametrize("name", sorted(HAND_SHAPES))
def test_trace_equals_edge_rule_on_hand_shapes(name):
    m = HAND_SHAPES[name]
    assert np.array_equal(ov.traced_pixels(m), ov.edge_pixels(m))
    if name == "full_image":
        assert ov.edge_pixels(m).sum() == 16 and not ov.edge_pixels(m)[1:-1, 1:-1].any()
    if name == "single_pixel":
        assert ov.edge_pixels(m).sum() == 1


def test_trace_equals_edge_rule_on_random_masks():
    rng = np.random.default_rng(2024)
    for n in range(200):
        density = 0.3 + 0.4 * (n % 5) / 4
        m = (rng.random((24, 24)) < density).astype(np.uint8)
        assert np.array_equal(ov.traced_pixels(m), ov.edge_pixels(m)), (n, density)


def _line(S, a, b, c, colour=(1, 2, 3)):
    pic = np.zeros((S, S, 3), np.uint8)
    ov.rasterise_line(pic, np.float32(a), np.float32(b), np.float32(c), colour)
    return pic


def test_line_rasteriser_edge_cases():
    S = 16
    on = lambda pic: set(zip(*np.nonzero(pic.any(axis=2))))     # noqa: E731  {(y, x)}
    assert on(_line(S, 1, 0, -5)) == {(y, 5) for y in range(S)}            # b = 0: vertical, walked by rows
    assert on(_line(S, 0, 1, -7)) == {(7, x) for x in range(S)}            # a = 0: horizontal
    assert on(_line(S, 1, -1, 0)) == {(x, x) for x in range(S)}            # |a| = |b|: walked by columns
    assert on(_line(S, 1, 1, -15)) == {(15 - x, x) for x in range(S)}
    assert on(_line(S, 0, 1, 3)) == set() and on(_line(S, 1, 0, -16)) == set()   # misses the picture
    assert on(_line(S, 0, 0, 1)) == set()                                  # a = b = 0
    # ties go to the even pixel: y = x / 2 + 0.5 is exact at odd x
    assert on(_line(S, 1, -2, 1)) >= {(0, 0), (2, 2), (2, 3), (4, 6), (4, 7)}
    assert on(_line(S, 1, -2, 1)) == {(int(np.rint(x / 2 + 0.5)), x) for x in range(S)}
    # y = -0.4 rounds to row 0 (-0.0), y = -0.6 leaves the picture
    assert (0, 0) in on(_line(S, 0, 1, 0.4)) and on(_line(S, 0, 1, 0.6)) == set()
    # a steep line is walked by rows: one pixel per row, none skipped
    steep = on(_line(S, 3, 1, -20))
    assert sorted(y for y, _ in steep) == [y for y in range(S) if 0 <= np.rint((20 - y) / 3) < S]


def test_crossing_lines_overwrite_in_order():
    S = 9
    pic = np.zeros((S, S, 3), np.uint8)
    ov.rasterise_line(pic, 0, 1, -4, ov.PALETTE_BGR[0])     # row 4, by columns
    ov.rasterise_line(pic, 1, 0, -4, ov.PALETTE_BGR[1])     # column 4, by rows
    assert tuple(pic[4, 4]) == ov.PALETTE_BGR[1] and tuple(pic[4, 3]) == ov.PALETTE_BGR[0] and tuple(pic[3, 4]) == ov.PALETTE_BGR[1]
    pic = np.zeros((S, S, 3), np.uint8)
    ov.rasterise_line(pic, 1, 0, -4, ov.PALETTE_BGR[1])
    ov.rasterise_line(pic, 0, 1, -4, ov.PALETTE_BGR[0])
    assert tuple(pic[4, 4]) == ov.PALETTE_BGR[0]


def test_mark_is_clipped_at_all_four_edges():
    S = 8
    assert sorted(ov.mark_pixels(S, 3, 3)) == [(2, 3), (3, 2), (3, 3), (3, 4), (4, 3)]
    assert sorted(ov.mark_pixels(S, 0, 3)) == [(2, 0), (3, 0), (3, 1), (4, 0)]
    assert sorted(ov.mark_pixels(S, 7, 3)) == [(2, 7), (3, 6), (3, 7), (4, 7)]
    assert sorted(ov.mark_pixels(S, 3, 0)) == [(0, 2), (0, 3), (0, 4), (1, 3)]
    assert sorted(ov.mark_pixels(S, 3, 7)) == [(6, 3), (7, 2), (7, 3), (7, 4)]
    assert sorted(ov.mark_pixels(S, 0, 0)) == [(0, 0), (0, 1), (1, 0)]
    frame = np.zeros((S, S, 3), np.uint8)
    out = ov.draw_blobs(frame, 2, [(7, 7)])
    assert {(y, x) for y, x in zip(*np.nonzero(out.any(axis=2)))} == {(7, 7), (7, 6), (6, 7)}
    assert tuple(out[7, 7]) == ov.MARK_BGR


def test_marks_go_over_contours():
    frame = np.zeros((12, 12, 3), np.uint8)
    frame[4:7, 4:7] = 255                                   # 3 x 3 blob: its border is all but the centre
    out = ov.draw_blobs(frame, 3, [(5, 5)])
    assert tuple(out[5, 5]) == ov.MARK_BGR and tuple(out[4, 5]) == ov.MARK_BGR and tuple(out[5, 4]) == ov.MARK_BGR
    assert tuple(out[4, 4]) == ov.CONTOUR_BGR and tuple(out[6, 6]) == ov.CONTOUR_BGR
    only = ov.draw_blobs(frame, 1, [(5, 5)])
    assert tuple(only[5, 5]) == (255, 255, 255) and tuple(only[4, 5]) == ov.CONTOUR_BGR


def test_overlay_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "mocap_core.h")).read()
    for name in ("CONTOURS", "CENTRES", "EPILINES"):
        m = re.search(r"MOCAP_OVERLAY_%s\s*=\s*(\d+)" % name, header)
        assert m, name
        assert getattr(capi, "OVERLAY_" + name) == int(m.group(1))
    assert (capi.OVERLAY_CONTOURS, capi.OVERLAY_CENTRES, capi.OVERLAY_EPILINES) == (1, 2, 4)
    for sym in ("mocap_set_preview_overlay", "mocap_draw_epilines", "mocap_draw_epilines_dev"):
        assert sym in capi.SIGNATURES and re.search(r"\b%s\(" % sym, header)
