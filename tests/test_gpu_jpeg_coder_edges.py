"""The entropy coder of the preview stream's JPEG encoder (csrc/jpeg_kernels.hip) where generic images never take it: codes
with one, two and three ZRLs in both tables, lane codes that spill into the emit pass's third word, DC category 11, every
quality's divisors, the later rounds of the size and stuff passes, a capacity that cuts between a 0xFF and its 0x00 or inside
the EOI, a workspace left dirty by a longer scan.  The images are tests/jpeg_cases.py's (tests/test_jpeg_cases_cpu.py
proves without a GPU that they reach those paths); every assertion is byte identity with tests/jpeg_reference.py, plus
size and status."""
import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_reference as jr
from mocap_core import capi

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB


def _first_difference(got, ref):
    return next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), min(len(got), len(ref)))


def _lane_at(prof, byte):
    """Which lane code covers the first bit of unstuffed scan byte `byte`: (index, table, zigzag position, ZRLs, offset, length)."""
    i = int(np.searchsorted(prof["offset"], 8 * byte, side="right")) - 1
    c = prof["lanes"][i]
    return i, ("Y", "C")[c[2]], c[3], c[5], int(prof["offset"][i]), c[1]


def _explain(name, f, got, ref):
    at = _first_difference(got, ref)
    prof = jc.profiles(name)[f]
    scan_byte = at - jr.HEADER_BYTES
    if 0 <= scan_byte:
        scan_byte -= int((prof["ff_positions"] + np.arange(len(prof["ff_positions"])) + 1 < scan_byte).sum())    # 0x00s in front
        where = f"unstuffed scan byte {scan_byte}, lane code {_lane_at(prof, min(scan_byte, prof['nb'] - 1))}"
    else:
        where = "header"
    return f"{name} image {f}: {len(got)} bytes for {len(ref)}, first difference at byte {at} ({where})"


def _check_case(core, name):
    frames, q = jc.CASES[name]
    refs = jc.expected(name)
    res = core.encode_jpeg(frames, quality=q)
    for f, ref in enumerate(refs):
        assert res["sizes"][f] == len(ref), (name, f, int(res["sizes"][f]), len(ref))
        assert res["status"][f] == 0, (name, f)
        assert res["jpeg"][f] == ref, _explain(name, f, res["jpeg"][f], ref)
    assert core.jpeg_bound(frames.shape[2], frames.shape[1] * frames.shape[3]) >= max(len(r) for r in refs)


@pytest.mark.parametrize("name", sorted(jc.CASES))
def test_device_equals_restatement(core, name):
    for f, prof in enumerate(jc.profiles(name)):
        print(f"{name}[{f}]: {jr.profile_line(prof)}")
    _check_case(core, name)


def _encode_dev(core, frames, quality, capacity):
    """mocap_encode_jpeg_dev into slots of `capacity` bytes with a guard behind the last -> every byte of the buffer."""
    import torch
    dev = torch.device("cuda", 0)
    F, T, H, W = frames.shape[:4]
    d_in = torch.from_numpy(np.array(frames)).to(dev)        # a copy: the cases are read-only
    d_out = torch.full((F * capacity + GUARD,), FILL, dtype=torch.uint8, device=dev)
    d_sizes = torch.zeros(F, dtype=torch.int64, device=dev)
    d_status = torch.full((F,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    core.encode_jpeg_dev(F, T, H, W, d_in.data_ptr(), quality, d_out.data_ptr(), capacity, d_sizes.data_ptr(), d_status.data_ptr())
    core.synchronize()
    return d_out.cpu().numpy(), d_sizes.cpu().numpy(), d_status.cpu().numpy()


def sweep_capacities(ref):
    """Around the header's end, on either side of the first stuffed 0xFF (p keeps the file's first p bytes, so not the 0xFF;
    p + 1 keeps it and cuts before its 0x00), and from inside the EOI to one byte more than the file."""
    p = ref.index(b"\xff\x00", jr.HEADER_BYTES)
    size = len(ref)
    return [jr.HEADER_BYTES - 1, jr.HEADER_BYTES, jr.HEADER_BYTES + 1, p, p + 1] + list(range(size - 3, size + 2))


def test_capacity_cuts_at_every_seam(core):
    name = "single_coefficient_luma/q95"
    frames, q = jc.CASES[name]
    ref, = jc.expected(name)
    size = len(ref)
    caps = sweep_capacities(ref)
    p = caps[3]
    assert caps[:3] == [622, 623, 624] and ref[p:p + 2] == b"\xff\x00" and 624 < p < size - 3 and ref[-2:] == b"\xff\xd9"
    for cap in caps:
        out, sizes, status = _encode_dev(core, frames, q, cap)
        keep = min(size, cap)
        assert out[:keep].tobytes() == ref[:keep], f"capacity {cap}: first difference at byte {_first_difference(out[:keep].tobytes(), ref)}"
        assert sizes[0] == size, (cap, int(sizes[0]))
        assert bool(status[0] & capi.JPEG_ST_OVERFLOW) == (size > cap) and not status[0] & ~capi.JPEG_ST_OVERFLOW, (cap, int(status[0]))
        assert (out[keep:] == FILL).all(), f"capacity {cap}: byte {keep + int(np.nonzero(out[keep:] != FILL)[0][0])} was written"


def test_shorter_scans_do_not_see_what_longer_ones_left(core):
    """The emit pass ORs into words that only the size pass has zeroed, and only as many as the image needs: a short scan after
    a long one, and the long one again over what the short ones left."""
    grey = np.full((1, 1, 16, 16, 3), 128, np.uint8)
    want_grey = jr.encode_tiles(grey[0], 95)
    ctx = capi.MocapCore(device_id=0)           # a context of its own: its workspace has seen nothing else
    try:
        for step, name in enumerate(("long_scan/q100", None, "single_coefficient_luma/q95", "long_scan/q100", None,
                                     "single_coefficient_chroma/q95")):
            if name is None:
                res = ctx.encode_jpeg(grey, quality=95)
                assert res["jpeg"][0] == want_grey and res["sizes"][0] == len(want_grey) and res["status"][0] == 0, f"step {step}"
            else:
                _check_case(ctx, name)
    finally:
        ctx.close()


def test_reruns_and_a_second_stream_give_the_same_bytes(core):
    """The emit pass's atomic ORs land in any order; nothing of that order may show."""
    import torch
    for name in ("long_scan/q100", "single_coefficient_chroma/q95"):
        frames, q = jc.CASES[name]
        ref, = jc.expected(name)
        cap = len(ref) + 5
        runs = [_encode_dev(core, frames, q, cap), _encode_dev(core, frames, q, cap)]
        stream = torch.cuda.Stream()
        core.set_stream(stream.cuda_stream)
        try:
            runs.append(_encode_dev(core, frames, q, cap))
        finally:
            core.set_stream(0)
        for out, sizes, status in runs:
            assert np.array_equal(out, runs[0][0]) and sizes[0] == len(ref) and status[0] == 0
        assert runs[0][0][:len(ref)].tobytes() == ref, _explain(name, 0, runs[0][0][:len(ref)].tobytes(), ref)
        assert (runs[0][0][len(ref):] == FILL).all()
