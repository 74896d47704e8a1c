"""NumPy statement of the grey-weighted centroid (include/mocap_core.h, mocap_set_centroid_mode; DESIGN.md 3.5b;
csrc/blob_centroid.hip), built on the oracle:

    contours   oracle.cv_image_restate.find_contours(RETR_TREE, CHAIN_APPROX_SIMPLE) over oracle.blob_oracle.binary_mask, a slot
               per contour with m00 != 0 in findContours' order -- exactly the slots of blob_oracle.centroids_from_mask
    window     the inclusive bounding box of the contour's (simplified) points
    pixels     the window's pixels with grey > 51, grey = COLOR_RGB2GRAY of the BGR frame (helpers.py:145-146)
    value      w = grey - 51;  x = float32(float64(sum(w x)) / float64(sum(w))), y likewise -- int64 sums, so exact
"""
import numpy as np

from oracle import blob_oracle as bo
from oracle import cv_image_restate as ci

THRESHOLD = 51            # int(255 * 0.2)


def grey_plane(frame_bgr):
    """The plane the reference thresholds (helpers.py:145)."""
    return ci.cvt_color(frame_bgr, ci.COLOR_RGB2GRAY)


def windows_from_mask(mask):
    """[(x0, y0, x1, y1), ...] inclusive, one per contour with m00 != 0, in findContours' order."""
    contours, _ = ci.find_contours(mask, ci.RETR_TREE, ci.CHAIN_APPROX_SIMPLE)
    out = []
    for c in contours:
        if ci.moments(c)["m00"] != 0:
            pts = c.reshape(-1, 2)
            out.append((int(pts[:, 0].min()), int(pts[:, 1].min()), int(pts[:, 0].max()), int(pts[:, 1].max())))
    return out


def window_sums(grey, window):
    """(sum w, sum w x, sum w y) as Python integers over the window's pixels with grey > 51."""
    x0, y0, x1, y1 = window
    g = np.asarray(grey)[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    dy, dx = np.nonzero(g > THRESHOLD)
    w = g[dy, dx] - THRESHOLD                     # int64: the sums of an 832 x 832 picture stay below 2^37
    sw, swx, swy = int(w.sum()), int((w * (x0 + dx)).sum()), int((w * (y0 + dy)).sum())
    return sw, swx, swy


def centroid_from_sums(sw, swx, swy):
    assert sw > 0 and max(swx, swy) < 2 ** 53
    return [np.float32(np.float64(swx) / np.float64(sw)), np.float32(np.float64(swy) / np.float64(sw))]


def weighted_centroids(frame_bgr, want_windows=False):
    """One processed BGR frame -> [[x, y], ...] float32 per slot (and the slots' windows)."""
    grey = grey_plane(frame_bgr)
    windows = windows_from_mask(bo.binary_mask(frame_bgr))
    pts = [centroid_from_sums(*window_sums(grey, w)) for w in windows]
    return (pts, windows) if want_windows else pts


def windows_overlap(windows):
    """True when two of the inclusive windows share a pixel."""
    for i, (ax0, ay0, ax1, ay1) in enumerate(windows):
        for bx0, by0, bx1, by1 in windows[i + 1:]:
            if ax0 <= bx1 and bx0 <= ax1 and ay0 <= by1 and by0 <= ay1:
                return True
    return False


def find_dots_weighted(raw_frames, Ks, dists, rotations=None):
    """blob_oracle.find_dots with weighted centroids: (processed frames, per-camera [[x, y], ...], per-camera windows)."""
    frames, points, windows = [], [], []
    for i, raw in enumerate(raw_frames):
        f = bo.preprocess(raw, Ks[i], dists[i], 0 if rotations is None else rotations[i])
        p, w = weighted_centroids(f, want_windows=True)
        frames.append(f)
        points.append(p)
        windows.append(w)
    return frames, points, windows


def blobs_from_processed(processed, M_max):
    """processed [F][C][S][S][3] (the blob stage's own output, pinned to the oracle by tests/test_gpu_blobs.py) ->
    blobs f32 [F][C][M_max][2] (zeros beyond the count), counts [F][C] (clipped to M_max), slots found [F][C]."""
    F, C = processed.shape[:2]
    blobs = np.zeros((F, C, M_max, 2), np.float32)
    counts = np.zeros((F, C), np.int32)
    found = np.zeros((F, C), np.int32)
    for f in range(F):
        b, n = bo.pack_points([weighted_centroids(processed[f, c]) for c in range(C)], M_max)
        blobs[f], found[f], counts[f] = b, n, np.minimum(n, M_max)
    return blobs, counts, found
