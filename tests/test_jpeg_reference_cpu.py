"""The contract of the preview stream's encoder, without a GPU: tests/jpeg_reference.py (the NumPy restatement the device
encoder is compared with) writes the file libjpeg writes, byte for byte.  PIL (libjpeg-turbo) is the arbiter where it is
installed; the committed goldens (scripts/make_jpeg_golden.py, confirmed by PIL when written) carry the pin elsewhere."""
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_reference as jr
from conftest import golden_names, load_golden

SIZES = ((16, 16), (16, 32), (32, 48), (320, 640))
QUALITIES = (1, 50, 75, 95, 100)


def _pil_encode(bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("content", jr.CONTENTS)
def test_restatement_equals_pil_byte_for_byte(H, W, content):
    pytest.importorskip("PIL")
    img = jr.content(content, H, W)
    for q in QUALITIES:
        ours, pil = jr.encode(img, q), _pil_encode(img, q)
        assert ours[:jr.HEADER_BYTES] == pil[:jr.HEADER_BYTES], (q, "header")
        assert ours == pil, (q, len(ours), len(pil))


def test_grid_reaches_stuffing_zrl_and_blocks_without_eob():
    """A grid that never reaches these would pass an encoder that gets them wrong."""
    noise = jr.content("noise", 320, 640)
    assert b"\xff\x00" in jr.encode(noise, 100)[jr.HEADER_BYTES:-2]
    coef = jr.coefficients(noise, 100)
    assert (coef[:, :, 63] != 0).any(), "no block without EOB"
    _, _, syms = jr.scan_symbols(jr.coefficients(jr.content("dots", 320, 640), 95))
    assert 0xF0 in syms, "no ZRL in the dark frame"
    # ... and how deep the ZRLs go: the dark frame's stay in luminance and never reach three; the constructed images
    # (tests/jpeg_cases.py) reach one, two and three in a row in both tables, which scan_symbols' symbols state as well
    dark = jr.scan_profile(jr.coefficients(jr.content("dots", 320, 640), 95))
    assert dark["zrl_codes"][0][1] >= 1 and dark["zrl_codes"][0][3] == 0 and dark["zrl_codes"][1][1:] == [0, 0, 0]
    for t, name in ((0, "single_coefficient_luma/q95"), (1, "single_coefficient_chroma/q95")):
        frames, q = jc.CASES[name]
        prof, = jc.profiles(name)
        assert all(n >= 3 for n in prof["zrl_codes"][t][1:]), (name, prof["zrl_codes"][t])
        _, _, syms = jr.scan_symbols(jr.coefficients(np.hstack(list(frames[0])), q))
        text = bytes(syms)
        assert text.count(b"\xf0") == sum(z * n for tbl in prof["zrl_codes"] for z, n in enumerate(tbl))
        assert b"\xf0\xf0\xf0" in text and b"\xf0\xf0\xf0\xf0" not in text      # three in a row, never four (run <= 62)


def test_quality_outside_1_100_is_refused():
    for q in (0, 101, -5):
        with pytest.raises(ValueError):
            jr.quant_tables(q)
    with pytest.raises(ValueError):
        jr.encode(np.zeros((24, 16, 3), np.uint8), 95)


def test_goldens_equal_the_restatement():
    names = golden_names("jpeg_")
    assert len(names) >= 3
    for name in names:
        g = load_golden(name)
        for i, q in enumerate(g["qualities"]):
            assert jr.encode_tiles(g["tiles"], int(q)) == g[f"jpeg_{i}"].tobytes(), (name, int(q))
