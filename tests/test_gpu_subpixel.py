"""Grey-weighted sub-pixel centroids on the GPU (mocap_set_centroid_mode(MOCAP_CENTROID_WEIGHTED), csrc/blob_centroid.hip)
against tests/subpixel_reference.py, the NumPy statement that tests/test_subpixel_reference_cpu.py checks on the CPU.  Integer
sums and one IEEE division: every comparison is bit for bit, no tolerance.  The reference takes the processed frames of the
call in reference mode as its input -- tests/test_gpu_blobs.py pins those to the oracle byte for byte.  The session's core
is shared: every test leaves the mode at 0."""
import contextlib
import functools

import numpy as np
import pytest

import overlay_reference as ov
import subpixel_reference as sp
from conftest import load_golden
from mocap_core import capi, helpers, synth

pytestmark = pytest.mark.gpu

REF_K = np.array([[320.0, 0, 160], [0, 320, 160], [0, 0, 1]])
RESULT_KEYS = ("counts", "status", "n_contours")


@contextlib.contextmanager
def weighted(core):
    core.set_centroid_mode(capi.CENTROID_WEIGHTED)
    try:
        yield core
    finally:
        core.set_centroid_mode(capi.CENTROID_REFERENCE)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _both_modes(core, images, M_max=16, want_processed=True):
    """(reference mode's result, weighted mode's result, the restatement's blobs for the same pictures)."""
    core.set_centroid_mode(capi.CENTROID_REFERENCE)
    ref = core.find_blobs(images, M_max=M_max, want_processed=True)
    with weighted(core):
        got = core.find_blobs(images, M_max=M_max, want_processed=want_processed)
    want, counts, found = sp.blobs_from_processed(ref["processed"], M_max)
    return ref, got, (want, counts, found)


def _check_weighted(core, images, M_max=16, want_processed=True):
    ref, got, (want, counts, found) = _both_modes(core, images, M_max, want_processed)
    for key in RESULT_KEYS + (("processed",) if want_processed else ()):
        assert np.array_equal(got[key], ref[key]), key
    ok = (ref["status"] & capi.BLOB_ST_CAP_OVERFLOW) == 0
    assert np.array_equal(ref["counts"][ok], counts[ok])
    assert np.array_equal(((ref["status"] & capi.BLOB_ST_POINT_OVERFLOW) != 0)[ok], (found > M_max)[ok])
    assert _same_bits(got["blobs"][ok], want[ok])
    assert not got["blobs"][~ok].any() and not got["counts"][~ok].any()      # no centroids for a picture over the caps
    return ref, got


# ----------------------------------------------------------------------------- 1: the rendered 4-camera input
@functools.lru_cache(maxsize=None)
def _rendered():
    rig = synth.ring_rig(4)
    images, truth = synth.render_camera_frames(rig, 3, 6, seed=1)
    images.setflags(write=False)
    return rig, images, truth


def _rendered_params(core):
    rig, images, truth = _rendered()
    core.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 4)
    return rig, images, truth


@functools.lru_cache(maxsize=None)
def _rendered_reference(core):
    """Reference mode's result on the rendered input and the restatement's blobs, computed once for the tests that share it."""
    _, images, _ = _rendered_params(core)
    core.set_centroid_mode(capi.CENTROID_REFERENCE)
    ref = core.find_blobs(images, M_max=16, want_processed=True)
    want, counts, _ = sp.blobs_from_processed(ref["processed"], 16)
    assert np.array_equal(counts, ref["counts"]) and not ref["status"].any()
    want.setflags(write=False)
    return ref, want


def test_rendered_frames_equal_the_restatement(core):
    _, images, truth = _rendered_params(core)
    ref, want = _rendered_reference(core)
    with weighted(core):
        got = core.find_blobs(images, M_max=16, want_processed=True)
    for key in RESULT_KEYS + ("processed",):
        assert np.array_equal(got[key], ref[key]), key
    assert _same_bits(got["blobs"], want)
    assert ref["counts"].sum() >= 60 and not _same_bits(got["blobs"], ref["blobs"])
    # sub-pixel values, a pixel's fraction away from the integer centroids of the same slots
    valid = np.arange(16)[None, None, :] < ref["counts"][:, :, None]
    assert (got["blobs"][valid] != np.floor(got["blobs"][valid])).mean() > 0.9
    assert np.abs(got["blobs"][valid] - ref["blobs"][valid]).max() < 1.5


# ----------------------------------------------------------------------------- 2: holes, nesting, overflow of both kinds
def _noisy(core):
    g = load_golden("blobs_c1_noisy")
    core.set_image_params(240, 320, g["K"], g["dist"], g["rotation"])
    return g["images"]


def test_noisy_golden_frame_with_point_overflow(core):
    images = _noisy(core)
    ref, got = _check_weighted(core, images, M_max=4)
    assert (ref["status"] & capi.BLOB_ST_POINT_OVERFLOW).all() and (got["counts"] == 4).all()


def test_noisy_golden_frame_through_the_large_tables_and_a_frame_over_them(core):
    images = _noisy(core)
    grid = np.zeros_like(images)                      # 2 x 2 dots on a 7-pixel grid: 1 530 contours, the large tables hold 1 024
    for dy in range(2):
        for dx in range(2):
            grid[0, 0, 4 + dy::7, 4 + dx::7] = 255
    batch = np.concatenate([images, grid, images])    # the frame over the caps between two that are not
    ref, got = _check_weighted(core, batch, M_max=256)
    assert ref["n_contours"][0, 0] > 256 and ref["counts"][0, 0] == 209        # zero-area contours skipped in between, re-run taken
    assert ref["status"][1, 0] == capi.BLOB_ST_CAP_OVERFLOW and got["counts"][1, 0] == 0 and got["n_contours"][1, 0] == -1
    assert _same_bits(got["blobs"][2], got["blobs"][0]) and not _same_bits(got["blobs"][0], ref["blobs"][0])


# ----------------------------------------------------------------------------- 3: blank, saturated, a ring; 64-bit sums
def _disc(img, cx, cy, r, value=255, hole=0):
    yy, xx = np.mgrid[:img.shape[0], :img.shape[1]]
    d2 = (xx - cx) ** 2 + (yy - cy) ** 2
    img[(d2 <= r * r) & (d2 >= hole * hole)] = value


def test_blank_saturated_and_ring_frames(core):
    """The 5 x 5 kernel sums to zero: of a saturated frame the chain keeps the outline, so its window is the whole frame area
    and its pixels are the few on the edge."""
    images = np.zeros((1, 3, 240, 320, 3), np.uint8)
    images[0, 1] = 255
    _disc(images[0, 2], 150, 100, 30, hole=14)        # a ring: outer and hole contours with area
    _disc(images[0, 2], 40, 200, 9, value=120)
    core.set_image_params(240, 320, [REF_K] * 3, [synth.REFERENCE_DISTORTION] * 3)
    ref, got = _check_weighted(core, images)
    assert ref["counts"][0, 0] == 0 and not got["blobs"][0, 0].any() and ref["counts"][0, 1] >= 1 and ref["counts"][0, 2] >= 3


def test_sums_past_32_bits(core):
    """The 64-bit case.  No picture of 320 x 320 gets there through a zero-sum filter; a comb of 6-pixel stripes at 480 x 640
    does: one contour whose window is the whole frame area, a third of its pixels on, sum(w x) = 8.9e9 (1 468 border pairs:
    inside the 4 096 the tables hold at this size)."""
    rows, cols = 480, 640
    images = np.zeros((1, 1, rows, cols, 3), np.uint8)
    for k in range(6):
        images[0, 0, 4 + k:rows - 4:12, 4:cols - 4] = 255
    images[0, 0, 4:rows - 4, 4:12] = 255              # the back of the comb joins the stripes into one blob
    K = np.array([[cols * 1.0, 0, cols / 2], [0, cols * 1.0, cols / 2], [0, 0, 1]])
    core.set_image_params(rows, cols, [K], [synth.REFERENCE_DISTORTION])
    ref, got = _check_weighted(core, images)
    frame = ref["processed"][0, 0]
    sums = [sp.window_sums(sp.grey_plane(frame), w) for w in sp.windows_from_mask(ov.bo.binary_mask(frame))]
    assert ref["counts"][0, 0] == len(sums) >= 1 and max(s[0] for s in sums) < 2 ** 32 < max(min(s[1:]) for s in sums)


# ----------------------------------------------------------------------------- 4: rotation and per-camera intrinsics
def test_rotated_camera_and_distinct_intrinsics(core):
    rig = synth.ring_rig(3)
    images, _ = synth.render_camera_frames(rig, 2, 6, seed=12)
    Ks = np.array([[[268.66976067, 0, 123.58679484], [0, 268.57495496, 167.56126939], [0, 0, 1]],
                   [[269.95158059, 0, 139.37072352], [0, 270.09608831, 160.36482761], [0, 0, 1]],
                   REF_K])
    dists = np.array([synth.REFERENCE_DISTORTION, [-0.2, 0.1, 0.002, -0.001, 0.05], [0, 0, 0, 0, 0]])
    core.set_image_params(240, 320, Ks, dists, [2, 0, 2])
    ref, _ = _check_weighted(core, images)
    assert ref["counts"].min() >= 2


# ----------------------------------------------------------------------------- 5, 6: scheduling does not show
def test_blob_options_give_identical_results(core):
    """Without `processed` the dark-tile early-outs are live: the tiles they skip have no grey bytes, and none is read."""
    _, images, _ = _rendered_params(core)
    ref, want = _rendered_reference(core)
    try:
        with weighted(core):
            for option in (0, 1, 2):
                core.set_blob_options(skip_dark_tiles=option)
                got = core.find_blobs(images, M_max=16)
                for key in RESULT_KEYS:
                    assert np.array_equal(got[key], ref[key]), (option, key)
                assert _same_bits(got["blobs"], want), option
    finally:
        core.set_blob_options(skip_dark_tiles=True)


def test_a_frame_set_alone_and_inside_a_batch(core):
    _, images, _ = _rendered_params(core)
    _, want = _rendered_reference(core)
    with weighted(core):
        batch = core.find_blobs(images, M_max=16)
        for f in range(3):
            alone = core.find_blobs(images[f:f + 1], M_max=16)
            assert _same_bits(alone["blobs"][0], batch["blobs"][f]) and np.array_equal(alone["counts"][0], batch["counts"][f])
    assert _same_bits(batch["blobs"], want)


# ----------------------------------------------------------------------------- 7, 8: option hygiene
def test_back_to_reference_mode_equals_a_fresh_context(core):
    _, images, _ = _rendered_params(core)
    core.set_preview_overlay(3)
    try:
        with weighted(core):
            marked = core.find_blobs(images, M_max=16, want_processed=True)
        after = core.find_blobs(images, M_max=16, want_processed=True)
    finally:
        core.set_preview_overlay(0)
    fresh = capi.MocapCore(0)
    try:
        rig = _rendered()[0]
        fresh.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 4)
        fresh.set_preview_overlay(3)
        clean = fresh.find_blobs(images, M_max=16, want_processed=True)
    finally:
        fresh.close()
    for key in RESULT_KEYS + ("processed",):
        assert np.array_equal(after[key], clean[key]), key
    assert _same_bits(after["blobs"], clean["blobs"]) and not _same_bits(marked["blobs"], clean["blobs"])


def test_unknown_modes_are_refused_and_change_nothing(core):
    _, images, _ = _rendered_params(core)
    ref, want = _rendered_reference(core)
    for bad in (2, -1):
        assert core.lib.mocap_set_centroid_mode(core._h, bad) == capi.MOCAP_E_ARG
        with pytest.raises(capi.MocapError):
            core.set_centroid_mode(bad)
    assert core.centroid_mode == capi.CENTROID_REFERENCE
    assert _same_bits(core.find_blobs(images, M_max=16)["blobs"], ref["blobs"])
    with weighted(core):
        for bad in (2, -1):
            assert core.lib.mocap_set_centroid_mode(core._h, bad) == capi.MOCAP_E_ARG
            with pytest.raises(capi.MocapError):
                core.set_centroid_mode(bad)
        assert core.centroid_mode == capi.CENTROID_WEIGHTED
        assert _same_bits(core.find_blobs(images, M_max=16)["blobs"], want)


# ----------------------------------------------------------------------------- 9: every entry point, and the chain
def _valid(a, counts):
    return a[np.arange(a.shape[2])[None, None, :] < counts[:, :, None]]


def test_every_entry_point_that_makes_blobs_honours_the_mode(core):
    import torch
    rig, images, _ = _rendered_params(core)
    ref, want = _rendered_reference(core)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    plain = core.find_blobs_jpeg(images, M_max=16, quality=90)
    F, C, M = 3, 4, 16
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(np.array(images)).to(dev)
    d_blobs = torch.zeros((F, C, M, 2), dtype=torch.float32, device=dev)
    d_counts = torch.zeros((F, C), dtype=torch.int32, device=dev)
    d_status = torch.zeros((F, C), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with weighted(core):
        core.find_blobs_dev(F, d_img.data_ptr(), M, d_blobs.data_ptr(), d_counts.data_ptr(), d_status.data_ptr())
        core.synchronize()
        stream = core.find_blobs_jpeg(images, M_max=16, quality=90)
        live = core.track_frame_images(images, M_max=16, O_max=4)
        live_stream = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=90)
    assert np.array_equal(d_counts.cpu().numpy(), ref["counts"]) and _same_bits(d_blobs.cpu().numpy(), want)
    assert _same_bits(stream["blobs"], want) and stream["jpeg"] == plain["jpeg"]
    for res in (live, live_stream):
        assert np.array_equal(res["counts"], ref["counts"]) and not res["blob_status"].any()
        assert _same_bits(_valid(res["blobs"], ref["counts"]), _valid(want, ref["counts"]))
    assert live_stream["jpeg"] == plain["jpeg"]


def _median_distance(xyz, n_pts, truth_points):
    d = []
    for f in range(len(n_pts)):
        pts = xyz[f, :n_pts[f]]
        for X in truth_points[f]:
            if len(pts):
                d.append(np.linalg.norm(pts - X, axis=1).min())
    d = np.array(d)
    return float(np.median(d[d < 0.05])), int((d < 0.05).sum())     # markers the frame path found (5 cm: a wrong match is not one)


def test_chain_equals_its_stages_and_lands_closer_to_the_markers(core):
    rig, images, truth = _rendered_params(core)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_world_transform(None)
    coarse = core.track_frame_images(images, M_max=16, O_max=4)
    with weighted(core):
        chained = core.track_frame_images(images, M_max=16, O_max=4)
        staged_blobs = core.find_blobs(images, M_max=16)
        staged = core.track_frame(staged_blobs["blobs"], staged_blobs["counts"], O_max=4)
    assert np.array_equal(chained["counts"], staged_blobs["counts"])
    assert _same_bits(_valid(chained["blobs"], chained["counts"]), _valid(staged_blobs["blobs"], chained["counts"]))
    for key in ("xyz", "err", "corr", "n_pts", "status", "pos", "heading", "error", "droneIndex", "n_obj"):
        assert np.array_equal(chained[key], staged[key], equal_nan=True), key
    assert chained["n_pts"].min() >= 3 and not chained["status"].any()
    fine_m, fine_n = _median_distance(chained["xyz"], chained["n_pts"], truth["points_cam0"])
    coarse_m, coarse_n = _median_distance(coarse["xyz"], coarse["n_pts"], truth["points_cam0"])
    print(f"median 3-D distance to the markers: reference mode {coarse_m * 1e3:.3f} mm ({coarse_n} markers), "
          f"weighted mode {fine_m * 1e3:.3f} mm ({fine_n} markers)")
    assert fine_n >= 12 and coarse_n >= 12
    assert fine_m < coarse_m


# ----------------------------------------------------------------------------- 10: the overlay keeps truncating
def test_centre_marks_sit_at_the_truncated_stored_centroids(core):
    _, images, _ = _rendered_params(core)
    ref, want = _rendered_reference(core)
    core.set_preview_overlay(capi.OVERLAY_CENTRES)
    try:
        with weighted(core):
            drawn = core.find_blobs(images, M_max=16, want_processed=True)
    finally:
        core.set_preview_overlay(0)
    assert _same_bits(drawn["blobs"], want)
    marks = ov.overlay_reference(ref["processed"], 2, drawn["blobs"], drawn["counts"], drawn["status"])
    assert np.array_equal(drawn["processed"], marks)
    assert not np.array_equal(marks, ref["processed"])


# ----------------------------------------------------------------------------- helpers
def test_helpers_return_floats_in_weighted_mode_and_ints_by_default(core):
    rig, images, _ = _rendered()
    ref, want = _rendered_reference(core)
    helpers.set_core(core)
    helpers.set_camera_params([{"intrinsic_matrix": rig["K"][i].tolist(), "distortion_coef": list(synth.REFERENCE_DISTORTION),
                                "rotation": 0} for i in range(4)])
    poses = [{"R": rig["R"][i], "t": rig["t"][i]} for i in range(4)]
    try:
        _, ints = helpers.camera_read_find_dots(images[0], want_frames=False)
        helpers.set_centroid_mode(capi.CENTROID_WEIGHTED)
        _, floats = helpers.camera_read_find_dots(images[0], want_frames=False)
        tracked = helpers.camera_read_track(images[0], poses)[0]
        with pytest.raises(ValueError):
            helpers.set_centroid_mode(2)
        blobs, counts, rounded = helpers.pack_frame(floats)                     # float32 values: carried exactly
        assert not rounded and np.array_equal(counts[0], ref["counts"][0]) and ref["counts"][0].min() >= 1
        for c in range(4):
            n = int(ref["counts"][0, c])
            assert ints[c] == ref["blobs"][0, c, :n].astype(np.int64).tolist() and all(type(v) is int for p in ints[c] for v in p)
            assert floats[c] == want[0, c, :n].astype(np.float64).tolist() and all(type(v) is float for p in floats[c] for v in p)
            assert tracked[c] == floats[c] and _same_bits(blobs[0, c, :n], want[0, c, :n])
        helpers.set_centroid_mode(capi.CENTROID_REFERENCE)
        assert helpers.camera_read_find_dots(images[0], want_frames=False)[1] == ints and core.centroid_mode == 0
    finally:
        helpers.set_centroid_mode(capi.CENTROID_REFERENCE)
        core.set_centroid_mode(capi.CENTROID_REFERENCE)
        helpers.set_core(None)
