"""NumPy restatement of the preview overlays (csrc/overlay_kernels.hip), built on the oracle:

    contours   cv.drawContours(img, contours, -1, (0,255,0), 1) over cv.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE)
               (reference helpers.py:147-148): oracle.cv_image_restate.find_contours, then every contour is walked vertex to
               vertex, closing the polygon.  CHAIN_APPROX_SIMPLE only drops interior points of horizontal, vertical and
               45-degree runs, so every step between two vertices is one of the 8 unit moves repeated, and a thickness-1
               8-connected line repaints exactly the dropped pixels: the painted set is the set the trace visited.
    marks      cv.circle(img, (cx, cy), 1, (100,255,100), -1) (helpers.py:157): OpenCV's Circle() (imgproc/drawing.cpp) for
               radius 1, filled, restated from its published source -- the centre row from cx - 1 to cx + 1, the rows
               above and below at cx alone, clipped to the picture.  No cv2 here pins it (tests/test_overlay_cv2_pin.py
               does where there is one).
    lines      the core's own contract (include/mocap_core.h, mocap_draw_epilines) over
               oracle.cv_restate.fundamental_from_projections / compute_correspond_epilines.
"""
import numpy as np

from oracle import blob_oracle as bo
from oracle import cv_image_restate as ci
from oracle import cv_restate as cr
from oracle import mocap_oracle as mo

CONTOUR_BGR = (0, 255, 0)
MARK_BGR = (100, 255, 100)
PALETTE_BGR = ((255, 0, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 128, 0))


def traced_pixels(mask):
    """bool [H][W]: the pixels drawContours(-1, thickness 1) paints for the contours of `mask` (non-zero = on)."""
    mask = np.asarray(mask)
    out = np.zeros(mask.shape, dtype=bool)
    if not mask.any():
        return out
    contours, _ = ci.find_contours((mask != 0).astype(np.uint8), ci.RETR_TREE, ci.CHAIN_APPROX_SIMPLE)
    for c in contours:
        pts = c.reshape(-1, 2)
        for j in range(len(pts)):
            (x0, y0), (x1, y1) = pts[j], pts[(j + 1) % len(pts)]
            dx, dy = int(x1) - int(x0), int(y1) - int(y0)
            n = max(abs(dx), abs(dy))
            assert dx == 0 or dy == 0 or abs(dx) == abs(dy), "a step between two vertices is one of the 8 unit moves, repeated"
            sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
            for s in range(n + 1):
                out[y0 + s * sy, x0 + s * sx] = True
    return out


def edge_pixels(mask):
    """bool [H][W]: mask pixels with at least one of their four edge neighbours off (outside the picture = off)."""
    m = np.asarray(mask) != 0
    p = np.pad(m, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def mark_pixels(S, cx, cy):
    """[(y, x), ...] of cv.circle(radius 1, filled) around (cx, cy) inside an S x S picture."""
    px = [(cy, cx), (cy, cx - 1), (cy, cx + 1), (cy - 1, cx), (cy + 1, cx)]
    return [(y, x) for (y, x) in px if 0 <= x < S and 0 <= y < S]


def draw_blobs(frame_bgr, flags, centroids):
    """One processed frame [S][S][3] -> annotated copy.  flags: bit 1 contours, bit 2 marks; centroids: the (x, y) the
    call STORED for this picture (the first `counts` of M_max)."""
    out = np.array(frame_bgr, dtype=np.uint8)
    S = out.shape[0]
    if flags & 1:
        out[traced_pixels(bo.binary_mask(frame_bgr))] = CONTOUR_BGR
    if flags & 2:
        for cx, cy in centroids:
            for y, x in mark_pixels(S, int(cx), int(cy)):
                out[y, x] = MARK_BGR
    return out


def overlay_reference(processed, flags, blobs, counts, status=None):
    """processed [F][C][S][S][3] from the call with flags 0; blobs [F][C][M][2], counts [F][C] of either call."""
    out = np.array(processed, dtype=np.uint8)
    F, C = out.shape[:2]
    for f in range(F):
        for c in range(C):
            if status is not None and status[f, c] & 2:      # BLOB_ST_CAP_OVERFLOW: left undrawn
                continue
            out[f, c] = draw_blobs(processed[f, c], flags, blobs[f, c, :counts[f, c]])
    return out


def rasterise_line(pic, a, b, c, colour):
    """The line a x + b y + c = 0 into pic [S][S][3], in place: coefficients widened to double, one pixel per column
    (|b| >= |a|, b != 0) or per row (a != 0), rint = to nearest even, pixels outside dropped."""
    S = pic.shape[0]
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    t = np.arange(S, dtype=np.float64)
    with np.errstate(all="ignore"):
        if abs(b) >= abs(a) and b != 0:
            y = np.rint(-(a * t + c) / b)
            ok = (y >= 0) & (y < S)
            pic[y[ok].astype(np.int64), t[ok].astype(np.int64)] = colour
        elif a != 0:
            x = np.rint(-(b * t + c) / a)
            ok = (x >= 0) & (x < S)
            pic[t[ok].astype(np.int64), x[ok].astype(np.int64)] = colour


def draw_epilines(bgr, Ks, R, t, blobs, counts, corr, n_pts, status):
    """bgr [F][C][S][S][3] -> drawn copy, by the contract of mocap_draw_epilines."""
    out = np.array(bgr, dtype=np.uint8)
    F, C = out.shape[:2]
    M = blobs.shape[2]
    P = [mo.projection_matrix(Ks[i], R[i], t[i]) for i in range(C)]
    Ftab = {}
    for f in range(F):
        if status[f] != 0:
            continue
        for k in range(max(0, min(int(n_pts[f]), corr.shape[1]))):
            seen = np.flatnonzero(corr[f, k] >= 0)
            if seen.size == 0:
                continue
            r = int(seen[0])
            b = int(corr[f, k, r])
            if b >= min(int(counts[f, r]), M):
                continue
            for i in range(r + 1, C):
                if (r, i) not in Ftab:
                    Ftab[(r, i)] = cr.fundamental_from_projections(P[r], P[i])
                line = cr.compute_correspond_epilines(np.asarray(blobs[f, r, b], dtype=np.float32).reshape(1, 1, 2), 1, Ftab[(r, i)])
                rasterise_line(out[f, i], *line[0, 0], PALETTE_BGR[k % 6])
    return out
