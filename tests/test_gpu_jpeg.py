"""The preview stream's JPEG encoder on the GPU (csrc/jpeg_kernels.hip) against tests/jpeg_reference.py, the NumPy
restatement that tests/test_jpeg_reference_cpu.py pins to libjpeg byte for byte, and against the committed goldens (which
carry that pin to machines without PIL).  Integer arithmetic throughout: the bar is byte identity of the whole file.
Shapes are the smallest that still reach every path: one MCU, a tile seam, several workgroups, the shortest scans there are,
codes and stuffed bytes across word and 16-byte piece boundaries, one full stream frame.

The shortest scans: the first block of each component codes its DC against 0.  A single all-black MCU takes 22 + 3 * 6
bits of luminance (DC -512 in category 10, then three zero differences, an EOB each) and 2 * 4 of chrominance: 48 bits, 6
bytes, no padding; all white takes 46 bits and 2 bits of padding.  Both end in the emit pass's second 32-bit word; with the
first DC that large no black or white image ends in the first.  A mid-grey MCU does: every DC is 0, 4 * 6 + 2 * 4 = 32
bits, the shortest scan there is, and it fills the first word exactly.  All three lie inside the first 16-byte piece of
the stuff pass.  Longer EOB-only scans (2 tiles of 32 x 48, 50 bytes) are images of the batch."""
import functools

import numpy as np
import pytest

import jpeg_reference as jr
from conftest import golden_names, load_golden
from mocap_core import capi, synth

pytestmark = pytest.mark.gpu


def _tiles(content, T, H, W, seed=3):
    if content == "grey":
        return np.full((T, H, W, 3), 128, np.uint8)
    return np.stack([jr.content(content, H, W, seed=seed + t) for t in range(T)])


# name -> (content, T, H, W, quality)
CASES = {
    "single_mcu": ("noise", 1, 16, 16, 95),
    "tile_seam": ("noise", 2, 16, 16, 75),
    "noise_q100": ("noise", 3, 32, 48, 100),
    "all_black": ("black", 1, 16, 16, 95),
    "all_white": ("white", 1, 16, 16, 95),
    "all_grey": ("grey", 1, 16, 16, 95),
    "checker_q100": ("checker", 2, 32, 48, 100),
    "stream_frame": ("dots", 2, 320, 320, 95),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    content, T, H, W, q = CASES[name]
    tiles = _tiles(content, T, H, W)
    tiles.setflags(write=False)
    return tiles, q, jr.encode_tiles(tiles, q)


BATCH_CONTENTS = ("noise", "black", "dots", "checker", "white")


@functools.lru_cache(maxsize=None)
def _batch():
    bgr = np.stack([_tiles(c, 2, 32, 48, seed=11) for c in BATCH_CONTENTS])
    bgr.setflags(write=False)
    return bgr, [jr.encode_tiles(bgr[f], 95) for f in range(len(BATCH_CONTENTS))]


def _check_files(core, res, want, H, W_total):
    bound = core.jpeg_bound(H, W_total)
    for f, ref in enumerate(want):
        assert res["sizes"][f] == len(ref), (f, int(res["sizes"][f]), len(ref))
        assert res["status"][f] == 0
        assert res["jpeg"][f] == ref, f"image {f}: first difference at byte " \
            f"{next((i for i, (a, b) in enumerate(zip(res['jpeg'][f], ref)) if a != b), min(len(ref), len(res['jpeg'][f])))}"
        assert bound >= len(ref)


@pytest.mark.parametrize("name", golden_names("jpeg_"))
def test_goldens(core, name):
    g = load_golden(name)
    T, H, W = g["tiles"].shape[:3]
    for i, q in enumerate(g["qualities"]):
        res = core.encode_jpeg(g["tiles"][None], quality=int(q))
        _check_files(core, res, [g[f"jpeg_{i}"].tobytes()], H, T * W)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(core, name):
    tiles, q, ref = _case(name)
    T, H, W = tiles.shape[:3]
    _check_files(core, core.encode_jpeg(tiles[None], quality=q), [ref], H, T * W)
    if name == "noise_q100":
        assert b"\xff\x00" in ref[jr.HEADER_BYTES:-2]      # the case does reach byte stuffing
    if name in ("all_black", "all_white"):
        assert len(ref) - jr.HEADER_BYTES - 2 == 6         # ... these end inside the second word (see above)
    if name == "all_grey":
        assert len(ref) - jr.HEADER_BYTES - 2 == 4         # ... and this one with the first


def test_batch_offsets_do_not_leak(core):
    bgr, refs = _batch()
    _check_files(core, core.encode_jpeg(bgr, quality=95), refs, 32, 96)


def _encode_dev(core, bgr, quality, capacity, guard=64, fill=0xAB):
    import torch
    dev = torch.device("cuda", 0)
    F, T, H, W = bgr.shape[:4]
    d_in = torch.from_numpy(np.ascontiguousarray(bgr)).to(dev)
    d_out = torch.full((F * capacity + guard,), fill, dtype=torch.uint8, device=dev)
    d_sizes = torch.zeros(F, dtype=torch.int64, device=dev)
    d_status = torch.full((F,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    core.encode_jpeg_dev(F, T, H, W, d_in.data_ptr(), quality, d_out.data_ptr(), capacity, d_sizes.data_ptr(), d_status.data_ptr())
    core.synchronize()
    return d_out.cpu().numpy(), d_sizes.cpu().numpy(), d_status.cpu().numpy()


def test_host_form_dev_form_reruns_and_other_stream_agree(core):
    import torch
    bgr, refs = _batch()
    cap = max(len(r) for r in refs) + 7
    runs = [_encode_dev(core, bgr, 95, cap), _encode_dev(core, bgr, 95, cap)]
    stream = torch.cuda.Stream()
    core.set_stream(stream.cuda_stream)
    try:
        runs.append(_encode_dev(core, bgr, 95, cap))
    finally:
        core.set_stream(0)
    host = core.encode_jpeg(bgr, quality=95, capacity=cap)
    for out, sizes, status in runs:
        assert np.array_equal(out, runs[0][0]) and not status.any()
        for f, ref in enumerate(refs):
            assert sizes[f] == len(ref) and out[f * cap:f * cap + len(ref)].tobytes() == ref == host["jpeg"][f]
            assert (out[f * cap + len(ref):(f + 1) * cap] == 0xAB).all()     # nothing written behind the file
        assert (out[len(refs) * cap:] == 0xAB).all()


def test_overflow_keeps_to_its_slot(core):
    first, q, ref0 = _case("noise_q100")
    second = _tiles("dots", 3, 32, 48, seed=5)
    ref1 = jr.encode_tiles(second, q)
    assert len(ref1) < len(ref0) - 1
    cap = len(ref0) - 1
    out, sizes, status = _encode_dev(core, np.stack([first, second]), q, cap)
    assert status[0] & capi.JPEG_ST_OVERFLOW and sizes[0] == len(ref0)
    assert out[:cap].tobytes() == ref0[:cap]
    assert status[1] == 0 and sizes[1] == len(ref1) and out[cap:cap + len(ref1)].tobytes() == ref1   # the next image is intact
    assert (out[cap + len(ref1):] == 0xAB).all()                                                     # rest of its slot and the guard
    assert core.jpeg_bound(32, 144) >= len(ref0)
    # a slot smaller than the header, in the last image of a batch: nothing lands in the guard
    out, sizes, status = _encode_dev(core, first[None], q, 100)
    assert status[0] & capi.JPEG_ST_OVERFLOW and sizes[0] == len(ref0) and out[:100].tobytes() == ref0[:100]
    assert (out[100:] == 0xAB).all()


def test_bad_arguments_are_refused_without_a_launch(core):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.zeros(32 * 32 * 3, dtype=torch.uint8, device=dev)
    d_out = torch.full((4096,), 0xAB, dtype=torch.uint8, device=dev)
    d_sizes = torch.full((1,), -7, dtype=torch.int64, device=dev)
    d_status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call(T=1, H=16, W=16, quality=95, out=d_out.data_ptr(), capacity=4096):
        return core.lib.mocap_encode_jpeg_dev(core._h, 1, T, H, W, capi._vp(d_in.data_ptr()), quality, capi._vp(out), capacity,
                                              capi._vp(d_sizes.data_ptr()), capi._vp(d_status.data_ptr()))
    assert call(H=24) == capi.MOCAP_E_ARG
    assert call(W=24) == capi.MOCAP_E_ARG
    assert call(quality=0) == capi.MOCAP_E_ARG
    assert call(quality=101) == capi.MOCAP_E_ARG
    assert call(T=0) == capi.MOCAP_E_ARG
    assert call(out=0) == capi.MOCAP_E_ARG
    assert call(capacity=0) == capi.MOCAP_E_ARG
    core.synchronize()
    assert (d_out.cpu().numpy() == 0xAB).all() and d_sizes.item() == -7 and d_status.item() == -7
    assert core.jpeg_bound(24, 16) == -1
    with pytest.raises(capi.MocapError):
        core.encode_jpeg(np.zeros((1, 1, 24, 16, 3), np.uint8))
    assert call() == 0      # the same buffers are fine with good arguments
    core.synchronize()
    assert d_sizes.item() > jr.HEADER_BYTES


def test_chain_raw_frames_to_payload_and_stream(core):
    rig = synth.ring_rig(2)
    images, _ = synth.render_camera_frames(rig, 2, 6, seed=7)
    core.set_cameras(rig["K"], rig["R"], rig["t"])
    core.set_image_params(240, 320, rig["K"], [synth.REFERENCE_DISTORTION] * 2)
    plain = core.track_frame_images(images, M_max=16, O_max=4)
    both = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95)
    for key in plain:
        assert np.array_equal(plain[key], both[key], equal_nan=True), key
    staged = core.find_blobs(images, M_max=16, want_processed=True)
    want = core.encode_jpeg(staged["processed"], quality=95)["jpeg"]
    assert both["jpeg"] == want and [int(s) for s in both["jpeg_size"]] == [len(w) for w in want]
    assert want[0] == jr.encode_tiles(staged["processed"][0], 95)
    blobs = core.find_blobs_jpeg(images, M_max=16, quality=95)
    assert blobs["jpeg"] == want
    for key in ("blobs", "counts", "status", "n_contours"):
        assert np.array_equal(blobs[key], staged[key]), key
    # a slot that is too small: the size still says what is needed, the payload is unchanged
    small = core.track_frame_images_jpeg(images, M_max=16, O_max=4, quality=95, capacity=700)
    assert [int(s) for s in small["jpeg_size"]] == [len(w) for w in want] and small["jpeg"][1] == want[1][:700]
    assert np.array_equal(small["xyz"], plain["xyz"], equal_nan=True)


def test_pil_decodes_the_device_stream(core):
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    tiles, q, _ = _case("stream_frame")
    rgb = np.ascontiguousarray(np.hstack(list(tiles))[..., ::-1])
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=2, optimize=False)
    ours = core.encode_jpeg(tiles[None], quality=q)["jpeg"][0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), np.asarray(Image.open(io.BytesIO(buf.getvalue()))))
