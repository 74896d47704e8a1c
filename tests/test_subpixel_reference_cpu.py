"""The NumPy statement of the grey-weighted centroid (tests/subpixel_reference.py) checked on the CPU: what it gains over the
reference's int() centroid on the project's synthetic IR frames, hand cases against sums written out by hand, and the
Python constants against the header."""
import functools
import os
import re

import numpy as np

import subpixel_reference as sp
from mocap_core import capi, synth
from oracle import blob_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _rendered():
    """The 4-camera input of DESIGN.md 3.5b through the oracle's preprocessing: per picture the weighted centroids, their
    windows, the reference's integer centroids and the ideal pixels of the visible markers."""
    rig = synth.ring_rig(4)
    images, truth = synth.render_camera_frames(rig, 3, 6, seed=1)
    out = []
    for f in range(3):
        frames, pts, wins = sp.find_dots_weighted(images[f], rig["K"], [synth.REFERENCE_DISTORTION] * 4)
        for c in range(4):
            uv = truth["uv"][f, c]
            out.append((pts[c], wins[c], bo.centroids_from_mask(bo.binary_mask(frames[c])), uv[~np.isnan(uv[:, 0])]))
    return out


def _matched_distances(points, uv):
    """Distance of each blob to the nearest ideal pixel, for the blobs that have one within 3 px."""
    d = [np.linalg.norm(uv - np.asarray(p, dtype=np.float64), axis=1).min() for p in points] if len(uv) else []
    return [x for x in d if x < 3.0]


def test_weighted_centroid_is_thirty_times_closer_to_the_ideal_pixel():
    dw, di = [], []
    for pts, _, ipts, uv in _rendered():
        assert len(pts) == len(ipts)                  # the same slots
        dw += _matched_distances(pts, uv)
        di += _matched_distances(ipts, uv)
    mw, mi = float(np.median(dw)), float(np.median(di))
    print(f"blobs matched {len(dw)} / {len(di)}: weighted median {mw:.4f} px, integer median {mi:.4f} px, factor {mi / mw:.1f}")
    assert len(dw) >= 60 and len(dw) == len(di)
    assert mw <= 0.05                                 # measured 0.0245: 2x margin for libm differences in the renderer
    assert mw * 10 <= mi                              # measured 0.785 for int(): about 32x


def test_no_two_windows_of_a_picture_overlap_on_the_rendered_input():
    """The condition under which the window equals the blob."""
    for _, wins, _, _ in _rendered():
        assert not sp.windows_overlap(wins)
    assert sp.windows_overlap([(0, 0, 4, 4), (4, 4, 6, 6)]) and not sp.windows_overlap([(0, 0, 4, 4), (5, 0, 6, 4)])


def _frame(grey):
    """A BGR frame whose grey plane is `grey`: equal channels pass COLOR_RGB2GRAY unchanged (the weights sum to 2^15)."""
    g = np.asarray(grey, dtype=np.uint8)
    f = np.repeat(g[:, :, None], 3, axis=2)
    assert np.array_equal(sp.grey_plane(f), g)
    return f


def test_two_by_two_blob():
    g = np.zeros((8, 8), np.uint8)
    g[3, 4], g[3, 5], g[4, 4], g[4, 5] = 61, 71, 81, 51 + 40   # weights 10 20 30 40
    pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
    assert wins == [(4, 3, 5, 4)]
    assert sp.window_sums(g, wins[0]) == (100, 10 * 4 + 20 * 5 + 30 * 4 + 40 * 5, 10 * 3 + 20 * 3 + 30 * 4 + 40 * 4)
    assert pts == [[np.float32(4.6), np.float32(3.7)]]
    assert bo.centroids_from_mask(bo.binary_mask(_frame(g))) == [[4, 3]]      # what int() keeps of it
    g[4, 5] = 51                                         # at the threshold: off, the blob is an L of three pixels
    pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
    assert wins == [(4, 3, 5, 4)] and sp.window_sums(g, wins[0]) == (60, 10 * 4 + 20 * 5 + 30 * 4, 10 * 3 + 20 * 3 + 30 * 4)
    assert pts == [[np.float32(np.float64(260) / np.float64(60)), np.float32(3.5)]]


def test_blob_in_a_corner():
    g = np.zeros((6, 6), np.uint8)
    g[4:6, 4:6] = [[255, 52], [52, 52]]                 # weights 204 1 1 1 in the bottom-right corner
    pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
    assert wins == [(4, 4, 5, 5)] and sp.window_sums(g, wins[0]) == (207, 204 * 4 + 4 + 5 + 5, 204 * 4 + 5 + 4 + 5)
    assert pts == [[np.float32(np.float64(830) / np.float64(207))] * 2]
    g = np.zeros((6, 6), np.uint8)
    g[0:2, 0:2] = 100                                    # top-left: x0 = y0 = 0
    pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
    assert wins == [(0, 0, 1, 1)] and pts == [[np.float32(0.5), np.float32(0.5)]]


def test_ring_outer_and_hole_contour():
    g = np.zeros((9, 9), np.uint8)
    g[1:8, 1:8] = 151                                    # weight 100
    g[1, 1:8] = 251                                      # top row: weight 200
    g[3:6, 3:6] = 0                                      # a 3 x 3 hole
    pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
    # outer border, then its hole; the hole border runs over the ring's inner pixels: window [2..6] x [2..6]
    assert wins == [(1, 1, 7, 7), (2, 2, 6, 6)]
    # outer: 7 pixels of 200 in row 1; rows 2 and 6..7 full (100 each), rows 3..5 four pixels each (x = 1, 2, 6, 7)
    sw = 7 * 200 + 3 * 7 * 100 + 3 * 4 * 100
    swx = 4 * sw                                         # symmetric about x = 4
    swy = 1 * 1400 + (2 + 6 + 7) * 700 + (3 + 4 + 5) * 400
    assert sp.window_sums(g, wins[0]) == (sw, swx, swy) == (4700, 18800, 16700)
    # hole: the 16 ring pixels of the 5 x 5 window, all of weight 100, symmetric about (4, 4)
    assert sp.window_sums(g, wins[1]) == (1600, 6400, 6400)
    assert pts == [[np.float32(4.0), np.float32(np.float64(16700) / np.float64(4700))], [np.float32(4.0), np.float32(4.0)]]


def test_saturated_full_picture_needs_64_bits():
    for S, past in ((320, 2 ** 31), (352, 2 ** 32)):     # 320: 3.3e9, past a signed 32-bit sum; 352: 4.4e9, past an unsigned one
        g = np.full((S, S), 255, np.uint8)
        pts, wins = sp.weighted_centroids(_frame(g), want_windows=True)
        assert wins == [(0, 0, S - 1, S - 1)]
        sw, swx, swy = sp.window_sums(g, wins[0])
        assert sw == 204 * S * S and swx == swy == 204 * S * (S * (S - 1) // 2)
        assert swx > past > sw
        half = np.float32((S - 1) / 2)
        assert pts == [[half, half]]
        assert np.float32(np.float64(swx % past) / np.float64(sw)) != half      # what a sum that wraps there would give


def test_centroid_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "mocap_core.h")).read()
    for name, value in (("REFERENCE", 0), ("WEIGHTED", 1)):
        m = re.search(r"MOCAP_CENTROID_%s\s*=\s*(\d+)" % name, header)
        assert m and int(m.group(1)) == value == getattr(capi, "CENTROID_" + name)
    assert "mocap_set_centroid_mode" in capi.SIGNATURES and re.search(r"\bmocap_set_centroid_mode\(", header)
