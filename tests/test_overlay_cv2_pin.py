"""The restatement of cv.drawContours and cv.circle in tests/overlay_reference.py against a REAL cv2.  This image has no
OpenCV, so the module skips; it starts pinning wherever `import cv2` works."""
import numpy as np
import pytest

import overlay_reference as ov
from test_overlay_reference_cpu import HAND_SHAPES

cv2 = pytest.importorskip("cv2")


def _cv2_contours(mask):
    img = np.zeros(mask.shape + (3,), np.uint8)
    contours, _ = cv2.findContours((mask != 0).astype(np.uint8) * 255, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE)
    cv2.drawContours(img, contours, -1, (0, 255, 0), 1)
    return img


@pytest.mark.parametrize("name", sorted(HAND_SHAPES))
def test_draw_contours_on_hand_shapes(name):
    m = HAND_SHAPES[name]
    img = _cv2_contours(m)
    assert np.array_equal(img.any(axis=2), ov.traced_pixels(m))
    assert (img[ov.traced_pixels(m)] == ov.CONTOUR_BGR).all()


def test_draw_contours_on_random_masks():
    rng = np.random.default_rng(2024)
    for n in range(200):
        m = (rng.random((24, 24)) < 0.3 + 0.4 * (n % 5) / 4).astype(np.uint8)
        assert np.array_equal(_cv2_contours(m).any(axis=2), ov.edge_pixels(m)), n


@pytest.mark.parametrize("centre", [(3, 3), (0, 3), (7, 3), (3, 0), (3, 7), (0, 0), (7, 7)])
def test_circle_radius_1_filled(centre):
    S = 8
    img = np.zeros((S, S, 3), np.uint8)
    cv2.circle(img, centre, 1, (100, 255, 100), -1)
    want = np.zeros((S, S, 3), np.uint8)
    for y, x in ov.mark_pixels(S, *centre):
        want[y, x] = ov.MARK_BGR
    assert np.array_equal(img, want)
