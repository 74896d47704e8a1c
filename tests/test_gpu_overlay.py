"""The preview overlays on the GPU (csrc/overlay_kernels.hip) against tests/overlay_reference.py, the NumPy restatement that
tests/test_overlay_reference_cpu.py checks on the CPU.  Byte stores of constant colours at integer positions: every
comparison is byte for byte, no tolerance.  Frames are 48 x 64 raw (S = 64, the smallest square the blob stage and the JPEG
encoder both take: one 64 x 64 tile, two bands of the contour kernel); a 112 x 128 frame reaches a second mask word per row
and the golden frame its own size.  The session's core is shared: every test leaves the option at 0."""
import contextlib
import functools

import numpy as np
import pytest

import jpeg_reference as jr
import overlay_reference as ov
from conftest import load_golden
from mocap_core import capi, helpers, synth

pytestmark = pytest.mark.gpu

K64 = np.array([[64.0, 0, 32], [0, 64, 32], [0, 0, 1]])
NO_DIST = np.zeros(5)


@contextlib.contextmanager
def overlay(core, flags):
    core.set_preview_overlay(flags)
    try:
        yield core
    finally:
        core.set_preview_overlay(0)


def _disc(img, cx, cy, r, value=255, hole=0):
    rows, cols = img.shape[:2]
    yy, xx = np.mgrid[:rows, :cols]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    img[(d2 <= r * r) & (d2 >= hole * hole)] = value


@functools.lru_cache(maxsize=None)
def _shapes(rows=48, cols=64):
    """[2][3][rows][cols][3] raw RGB: discs, a ring, a dot on the frame edge, a one-pixel speck; frame set 1 holds an
    all-dark picture."""
    img = np.zeros((2, 3, rows, cols, 3), np.uint8)
    _disc(img[0, 0], 16, 14, 5)
    _disc(img[0, 0], 44, 22, 8, hole=4)           # ring: an outer and a hole border
    _disc(img[0, 0], 0, 36, 3)                    # on the left edge of the frame
    img[0, 0, 40, 30] = 255                       # speck (need not survive the filter chain)
    _disc(img[0, 1], cols - 1, 10, 4)             # on the right edge
    _disc(img[0, 1], 20, 30, 6)
    _disc(img[0, 1], 30, 33, 4)                   # touching its neighbour after the blur
    _disc(img[0, 2], 32, rows - 1, 5)             # on the last raw row (the feathered padding continues it)
    _disc(img[0, 2], 10, 8, 2)
    _disc(img[1, 0], 50, 40, 6)
    _disc(img[1, 2], 12, 12, 3, value=90)         # dim: partly below the threshold
    img[1, 2, 30, 40:44] = 255
    img.setflags(write=False)
    return img


def _params(core, images, K=K64):
    C = images.shape[1]
    core.set_image_params(images.shape[2], images.shape[3], [K] * C, [NO_DIST] * C)


def _bare_and_drawn(core, images, flags, M_max=16):
    core.set_preview_overlay(0)
    bare = core.find_blobs(images, M_max=M_max, want_processed=True)
    with overlay(core, flags):
        drawn = core.find_blobs(images, M_max=M_max, want_processed=True)
    for key in ("blobs", "counts", "status", "n_contours"):
        assert np.array_equal(bare[key], drawn[key]), key
    return bare, drawn


def _first_difference(a, b):
    d = np.argwhere(np.asarray(a) != np.asarray(b))
    return None if d.size == 0 else tuple(int(v) for v in d[0])


# ----------------------------------------------------------------------------- contours and marks
@pytest.mark.parametrize("flags", [3, 1, 2])
def test_contours_and_marks_equal_the_restatement(core, flags):
    images = _shapes()
    _params(core, images)
    bare, drawn = _bare_and_drawn(core, images, flags)
    want = ov.overlay_reference(bare["processed"], flags, bare["blobs"], bare["counts"], bare["status"])
    assert _first_difference(drawn["processed"], want) is None
    # the case is not vacuous: the ring's outer and hole border next to the discs of picture (0, 0), centroids in every
    # picture of frame set 0, drawings in every picture but the dark one
    assert bare["counts"][0].min() >= 2 and bare["n_contours"][0, 0] >= 5 and not bare["status"].any()
    changed = (drawn["processed"] != bare["processed"]).any(axis=(2, 3, 4))
    assert changed[0].all() and not changed[1, 1] and bare["counts"][1, 1] == 0
    assert np.array_equal(drawn["processed"][1, 1], bare["processed"][1, 1])


def test_dev_form_equals_host_form(core):
    import torch
    images = _shapes()
    _params(core, images)
    F, C = images.shape[:2]
    M, S = 16, 64
    dev = torch.device("cuda", 0)
    with overlay(core, 3):
        host = core.find_blobs(images, M_max=M, want_processed=True)
        d_img = torch.from_numpy(np.array(images)).to(dev)
        d_blobs = torch.zeros((F, C, M, 2), dtype=torch.float32, device=dev)
        d_counts = torch.zeros((F, C), dtype=torch.int32, device=dev)
        d_status = torch.zeros((F, C), dtype=torch.int32, device=dev)
        d_proc = torch.full((F * C * S * S * 3 + 64,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        core.find_blobs_dev(F, d_img.data_ptr(), M, d_blobs.data_ptr(), d_counts.data_ptr(), d_status.data_ptr(), d_proc.data_ptr())
        core.synchronize()
    out = d_proc.cpu().numpy()
    assert np.array_equal(out[:-64].reshape(F, C, S, S, 3), host["processed"]) and (out[-64:] == 0xAB).all()
    assert np.array_equal(d_counts.cpu().numpy(), host["counts"]) and np.array_equal(d_blobs.cpu().numpy(), host["blobs"])


@pytest.mark.parametrize("skip_dark", [0, 1])
def test_all_dark_frames_stay_as_they_are(core, skip_dark):
    images = np.zeros((1, 2, 48, 64, 3), np.uint8)
    _params(core, images)
    core.set_blob_options(skip_dark_tiles=bool(skip_dark))
    try:
        bare, drawn = _bare_and_drawn(core, images, 3)
    finally:
        core.set_blob_options(skip_dark_tiles=True)
    assert not bare["counts"].any() and np.array_equal(drawn["processed"], bare["processed"])


def test_blob_across_the_mask_word_boundary(core):
    images = np.zeros((1, 2, 112, 128, 3), np.uint8)
    _disc(images[0, 0], 63, 50, 6)                # columns 57 .. 69: both 64-bit words of its rows
    _disc(images[0, 0], 64, 90, 1)
    _disc(images[0, 1], 127, 60, 5)               # the last column of the second word
    _disc(images[0, 1], 70, 20, 9, hole=5)
    K = np.array([[128.0, 0, 64], [0, 128, 64], [0, 0, 1]])
    _params(core, images, K)
    bare, drawn = _bare_and_drawn(core, images, 3)
    want = ov.overlay_reference(bare["processed"], 3, bare["blobs"], bare["counts"], bare["status"])
    assert _first_difference(drawn["processed"], want) is None
    edge = ov.edge_pixels(ov.bo.binary_mask(bare["processed"][0, 0]))
    assert edge[:, 63].any() and edge[:, 64].any() and bare["counts"].min() >= 1


def test_one_golden_frame_at_its_own_size(core):
    g = load_golden("blobs_c3_calib_rot")
    images = g["images"][:1]
    core.set_image_params(images.shape[2], images.shape[3], g["K"], g["dist"], g["rotation"])
    bare, drawn = _bare_and_drawn(core, images, 3, M_max=g["ref_points"].shape[2])
    assert np.array_equal(bare["processed"], g["ref_frames"][:1]) and bare["counts"].sum() > 0
    want = ov.overlay_reference(bare["processed"], 3, bare["blobs"], bare["counts"], bare["status"])
    assert _first_difference(drawn["processed"], want) is None


def test_marks_only_for_stored_centroids(core):
    images = _shapes()
    _params(core, images)
    bare, drawn = _bare_and_drawn(core, images, 3, M_max=1)
    assert (bare["status"] & capi.BLOB_ST_POINT_OVERFLOW).any() and bare["counts"].max() == 1
    want = ov.overlay_reference(bare["processed"], 3, bare["blobs"], bare["counts"], bare["status"])
    assert _first_difference(drawn["processed"], want) is None
    full, _ = _bare_and_drawn(core, images, 3, M_max=16)
    every = ov.overlay_reference(full["processed"], 3, full["blobs"], full["counts"], full["status"])
    assert _first_difference(want, every) is not None          # fewer marks than centroids; `want` has every contour painted
    assert np.array_equal(full["processed"], bare["processed"]) and (full["counts"] > 1).any()


# ----------------------------------------------------------------------------- option hygiene
def test_unknown_bit_is_refused_and_zero_restores_the_bytes(core):
    images = _shapes()
    _params(core, images)
    with overlay(core, 3):
        for bad in (8, 16, 7 | 8, 1 << 31):
            assert core.lib.mocap_set_preview_overlay(core._h, bad) == capi.MOCAP_E_ARG
            with pytest.raises(capi.MocapError):
                core.set_preview_overlay(bad)
        assert core.preview_overlay == 3
        drawn = core.find_blobs(images, want_processed=True)["processed"]      # the refused calls changed nothing
    after = core.find_blobs(images, want_processed=True)["processed"]
    fresh = capi.MocapCore(0)
    try:
        _params(fresh, images)
        clean = fresh.find_blobs(images, want_processed=True)["processed"]
    finally:
        fresh.close()
    assert np.array_equal(after, clean) and _first_difference(drawn, clean) is not None


# ----------------------------------------------------------------------------- epipolar lines
def _project(K, R, t, X):
    Xc = X @ R.T + t
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)


def _translated_rig(axis, step=0.2, C=3):
    t = np.zeros((C, 3))
    t[:, axis] = step * np.arange(C)
    return np.stack([K64] * C), np.stack([np.eye(3)] * C), t


SEVEN = np.array([[0.5, 0.5, 2.0], [-0.4, 0.3, 2.2], [0.1, -0.5, 1.9], [-0.6, -0.4, 2.4], [0.55, -0.1, 2.1], [-0.1, 0.6, 2.3],
                  [0.3, 0.1, 1.8]])


def _line_case(core, K, R, t, X, drop=()):
    """One frame of the points X seen by every camera (integer-free float32 blobs), minus the (camera, point) pairs in `drop`;
    a second, empty frame.  Returns the pictures the core drew, the restatement's, and the frame path's answer."""
    C, M = len(K), len(X)
    blobs = np.full((2, C, M, 2), np.nan, np.float32)
    counts = np.zeros((2, C), np.int32)
    for c in range(C):
        uv = _project(K[c], R[c], t[c], X)
        keep = [m for m in range(M) if (c, m) not in drop]
        blobs[0, c, :len(keep)] = uv[keep]
        counts[0, c] = len(keep)
    assert (blobs[0][~np.isnan(blobs[0])] >= 0).all() and (blobs[0][~np.isnan(blobs[0])] < 64).all()
    core.set_cameras(K, R, t)
    res = core.match_triangulate(blobs, counts)
    black = np.zeros((2, C, 64, 64, 3), np.uint8)
    got = core.draw_epilines(black, blobs, counts, res["corr"], res["n_out"], res["status"])
    want = ov.draw_epilines(black, K, R, t, blobs, counts, res["corr"], res["n_out"], res["status"])
    assert not black.any()                                       # the caller's pictures are copied, not drawn into
    return got, want, res, (blobs, counts)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_lines_of_translated_rigs(core, axis):
    K, R, t = _translated_rig(axis)
    got, want, res, _ = _line_case(core, K, R, t, SEVEN)
    assert res["n_out"][0] == 7 and res["n_out"][1] == 0 and not res["status"].any()
    assert _first_difference(got, want) is None
    assert not got[0, 0].any() and got[0, 1].any() and got[0, 2].any()       # every root sits in camera 0
    assert not got[1].any()                                                  # n_pts = 0: untouched
    colours = {tuple(c) for c in got[0, 1].reshape(-1, 3)} - {(0, 0, 0)}
    assert colours == set(ov.PALETTE_BGR)                                    # seven points wrap the palette
    P = [ov.mo.projection_matrix(K[i], R[i], t[i]) for i in range(3)]
    first = int(np.flatnonzero(res["corr"][0, :, 0] == 0)[0])                 # the output point rooted in SEVEN[0]
    a, b, _ = ov.cr.compute_correspond_epilines(_project(K[0], R[0], t[0], SEVEN[:1]).astype(np.float32).reshape(1, 1, 2), 1,
                                                ov.cr.fundamental_from_projections(P[0], P[1]))[0, 0]
    if axis == 0:
        assert a == 0 and b != 0          # horizontal
    if axis == 1:
        assert b == 0 and a != 0          # vertical: the line the reference cannot draw
        col = ov.PALETTE_BGR[first % 6]
        assert ((got[0, 1] == col).all(axis=-1).sum(axis=0) == 64).any()
    if axis == 2:
        assert abs(a) == abs(b) != 0      # through the principal point at 45 degrees


def test_lines_of_a_ring_rig_with_per_camera_intrinsics(core):
    rig = synth.ring_rig(3, K=K64)
    K = np.array([[[64.0 + 3 * i, 0, 32 - i], [0, 62.0 + 5 * i, 32 + 2 * i], [0, 0, 1]] for i in range(3)])
    X = SEVEN[:5] * [1, 1, 0] * 0.8 + rig["centre"] + [[0, 0, 0.1 * i] for i in range(5)]
    got, want, res, _ = _line_case(core, K, rig["R"], rig["t"], X)
    assert res["n_out"][0] == 5 and not res["status"].any()
    assert _first_difference(got, want) is None and got[0, 1].any() and got[0, 2].any()


def test_a_point_rooted_in_camera_1_draws_only_in_camera_2(core):
    K, R, t = _translated_rig(0)
    got, want, res, _ = _line_case(core, K, R, t, SEVEN[:1], drop={(0, 0)})
    assert res["n_out"][0] == 1 and list(res["corr"][0, 0]) == [-1, 0, 0]
    assert _first_difference(got, want) is None
    assert not got[0, 0].any() and not got[0, 1].any() and got[0, 2].any()


def test_flagged_frames_are_untouched(core):
    K, R, t = _translated_rig(2)
    got, _, res, (blobs, counts) = _line_case(core, K, R, t, SEVEN)
    noise = np.random.default_rng(5).integers(0, 256, (2, 3, 64, 64, 3), dtype=np.uint8)
    flagged = core.draw_epilines(noise, blobs, counts, res["corr"], res["n_out"], np.array([capi.ST_CAND_OVERFLOW, 0], np.int32))
    assert np.array_equal(flagged, noise)
    drawn = core.draw_epilines(noise, blobs, counts, res["corr"], res["n_out"], res["status"])
    lines = got.any(axis=-1)
    assert np.array_equal(drawn[lines], got[lines]) and np.array_equal(drawn[~lines], noise[~lines])


def test_draw_epilines_dev_equals_host_form(core):
    import torch
    K, R, t = _translated_rig(2)
    got, _, res, (blobs, counts) = _line_case(core, K, R, t, SEVEN)
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("blobs", blobs), ("counts", counts), ("corr", res["corr"]), ("n", res["n_out"]), ("st", res["status"]))}
    n_px = 2 * 3 * 64 * 64 * 3
    d_bgr = torch.zeros(n_px + 64, dtype=torch.uint8, device=dev)
    d_bgr[n_px:] = 0xAB
    torch.cuda.synchronize()
    core.draw_epilines_dev(2, 64, d_bgr.data_ptr(), blobs.shape[2], d["blobs"].data_ptr(), d["counts"].data_ptr(),
                           res["corr"].shape[1], d["corr"].data_ptr(), d["n"].data_ptr(), d["st"].data_ptr())
    core.synchronize()
    out = d_bgr.cpu().numpy()
    assert np.array_equal(out[:n_px].reshape(got.shape), got) and (out[n_px:] == 0xAB).all()
    with pytest.raises(capi.MocapError):
        core.draw_epilines_dev(2, 0, d_bgr.data_ptr(), blobs.shape[2], d["blobs"].data_ptr(), d["counts"].data_ptr(),
                               res["corr"].shape[1], d["corr"].data_ptr(), d["n"].data_ptr(), d["st"].data_ptr())


# ----------------------------------------------------------------------------- chains
@functools.lru_cache(maxsize=None)
def _scene():
    rig = synth.ring_rig(3, K=K64)
    images, _ = synth.render_camera_frames(rig, 2, 4, seed=7, rows=48, cols=64, dist=NO_DIST, spot_sigma=(1.0, 1.6), dropout=0.0,
                                           half_extent=0.6, min_sep=0.25)
    images.setflags(write=False)
    return rig, images


def _scene_core(core):
    rig, images = _scene()
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_image_params(48, 64, rig["K"], [NO_DIST] * 3)
    return rig, images


def test_find_blobs_jpeg_encodes_the_annotated_frames(core):
    rig, images = _scene_core(core)
    with overlay(core, 3):
        staged = core.find_blobs(images, M_max=16, want_processed=True)
        chained = core.find_blobs_jpeg(images, M_max=16, quality=95)
    bare = core.find_blobs(images, M_max=16, want_processed=True)
    assert _first_difference(staged["processed"], ov.overlay_reference(bare["processed"], 3, bare["blobs"], bare["counts"])) is None
    assert _first_difference(staged["processed"], bare["processed"]) is not None
    assert chained["jpeg"] == core.encode_jpeg(staged["processed"], quality=95)["jpeg"]
    assert chained["jpeg"][0] == jr.encode_tiles(staged["processed"][0], 95)
    for key in ("blobs", "counts", "status", "n_contours"):
        assert np.array_equal(chained[key], bare[key]), key


def test_track_chain_draws_blobs_and_lines_into_the_stream(core):
    rig, images = _scene_core(core)
    plain = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95)
    with overlay(core, 7):
        first = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95)
        again = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95)
        annotated = core.find_blobs(images, M_max=16, want_processed=True)["processed"]
    assert plain["n_pts"].min() >= 2 and not plain["status"].any()
    for key in plain:
        if key not in ("jpeg", "jpeg_size"):
            assert np.array_equal(plain[key], first[key], equal_nan=True), key
    lined = core.draw_epilines(annotated, first["blobs"], first["counts"], first["corr"], first["n_pts"], first["status"])
    assert _first_difference(lined, ov.draw_epilines(annotated, rig["K"], rig["R"], rig["t"], first["blobs"], first["counts"],
                                                      first["corr"], first["n_pts"], first["status"])) is None
    assert _first_difference(lined, annotated) is not None
    want = core.encode_jpeg(lined, quality=95)["jpeg"]
    assert first["jpeg"] == want and [int(s) for s in first["jpeg_size"]] == [len(w) for w in want]
    assert again["jpeg"] == first["jpeg"] and first["jpeg"] != plain["jpeg"]
    # bits 1 and 2 alone: the stream of the annotated frames, no lines
    with overlay(core, 3):
        assert core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95)["jpeg"] == core.encode_jpeg(annotated, quality=95)["jpeg"]


# ----------------------------------------------------------------------------- helpers
def test_helpers_return_drawn_frames(core):
    rig, images = _scene_core(core)
    helpers.set_core(core)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist(), "distortion_coef": NO_DIST.tolist(), "rotation": 0}
                               for i in range(3)])
    poses = [{"R": rig["R"][i], "t": rig["t"][i]} for i in range(3)]
    try:
        frames0, points = helpers.camera_read_find_dots(images[0])
        assert all(p != [[None, None]] for p in points)
        given = [frames0[0], None, frames0[2]]
        err, xyz, back = helpers.find_point_correspondance_and_object_points([list(p) for p in points], poses, given)
        assert len(xyz) >= 2 and all(b is g for b, g in zip(back, given))          # option off: the very objects
        helpers.set_preview_overlay(capi.OVERLAY_CONTOURS | capi.OVERLAY_CENTRES | capi.OVERLAY_EPILINES)
        frames3, points3 = helpers.camera_read_find_dots(images[0])
        assert points3 == points
        blobs, counts, _ = helpers.pack_frame([list(p) for p in points])
        bare = np.stack(frames0)[None]
        assert _first_difference(np.stack(frames3)[None], ov.overlay_reference(bare, 3, blobs, counts)) is None
        given = [frames3[0], None, frames3[2]]
        err7, xyz7, drawn = helpers.find_point_correspondance_and_object_points([list(p) for p in points], poses, given)
        assert np.array_equal(xyz7, xyz) and np.array_equal(err7, err) and drawn[1] is None
        res = core.match_triangulate_auto(blobs, counts, gate_px=5.0)
        full = np.stack([frames3[0], np.zeros_like(frames3[0]), frames3[2]])[None]
        want = ov.draw_epilines(full, rig["K"], rig["R"], rig["t"], blobs, counts, res["corr"], res["n_out"], res["status"])
        assert np.array_equal(drawn[0], want[0, 0]) and np.array_equal(drawn[2], want[0, 2])
        assert _first_difference(drawn[2], frames3[2]) is not None and np.array_equal(given[2], frames3[2])
        jpeg, _ = helpers.get_frames_jpeg(images[0])
        assert jpeg == core.encode_jpeg(np.stack(frames3)[None], quality=95)["jpeg"][0]
        helpers.set_preview_overlay(0)
        frames_off, _ = helpers.camera_read_find_dots(images[0])
        assert np.array_equal(np.stack(frames_off), np.stack(frames0)) and core.preview_overlay == 0
        with pytest.raises(ValueError):
            helpers.set_preview_overlay(8)
    finally:
        helpers.set_preview_overlay(0)
        core.set_preview_overlay(0)
        helpers.set_core(None)
