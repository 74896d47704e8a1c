"""No GPU: the constructed images of tests/jpeg_cases.py reach the paths of the entropy coder they are meant for
(jpeg_reference.scan_profile), the profile is a statement about the encoder's own bytes, and the restatement writes on every
one of them the file libjpeg writes (PIL where it is installed; the committed goldens carry that pin elsewhere).  The
thresholds below are conditions the builders have to meet, not measurements of them."""
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_reference as jr
from conftest import load_golden

NAMES = sorted(jc.CASES)
TABLES = ((0, "luminance"), (1, "chrominance"))


def _all_profiles():
    return [(name, f, p) for name in NAMES for f, p in enumerate(jc.profiles(name))]


@pytest.mark.parametrize("name", NAMES)
def test_lane_codes_are_the_encoders_bytes(name):
    """The profile is tied to the encoder: its lane codes, concatenated, padded and stuffed, are pack_scan's bytes, and with
    the header and the EOI the file; lengths, offsets and the byte count follow from the same codes."""
    frames, q = jc.CASES[name]
    for f, prof in enumerate(jc.profiles(name)):
        coef = jr.coefficients(np.hstack(list(frames[f])), q)
        codes, lens, _ = jr.scan_symbols(coef)
        raw = jr.unstuffed_scan(prof["lanes"])
        assert jr.stuffed(raw) == jr.pack_scan(codes, lens)
        assert jr.header(frames.shape[2], frames.shape[1] * frames.shape[3], q) + jr.stuffed(raw) + b"\xff\xd9" == jc.expected(name)[f]
        assert prof["total_bits"] == int(lens.sum()) == int(prof["length"].sum())
        assert prof["nb"] == len(raw) and prof["pad_bits"] == 8 * len(raw) - prof["total_bits"]
        assert prof["offset"][0] == 0 and (np.diff(prof["offset"]) == prof["length"][:-1]).all()
        assert len(prof["ff_positions"]) == raw.count(b"\xff") == len(jc.expected(name)[f]) - jr.HEADER_BYTES - 2 - len(raw)
        assert prof["blocks"] == coef.shape[0] * 6
        # a lane code holds at most 3 ZRLs (11 bits), a 16-bit symbol and 10 value bits: what the device's 64-bit lane assumes
        assert 1 <= prof["length"].min() and prof["length"].max() <= 59


def test_profile_of_a_hand_made_scan():
    """One MCU by hand: Y00 = DC 3, +1 at 17, -2 at 63; the other blocks empty."""
    coef = np.zeros((1, 6, 64), np.int64)
    coef[0, 0, 0], coef[0, 0, 17], coef[0, 0, 63] = 3, 1, -2
    prof = jr.scan_profile(coef)
    # Y00: DC category 2 (011 + 11); run 16 = ZRL (11 bits) + 0/1 (00 + 1 bit); run 45 = 2 ZRLs + 13/2 (16 bits + 2); no EOB.
    # Y01: DC -3 (5 bits) + EOB (4); Y10, Y11: DC 0 (2) + EOB; Cb, Cr: DC 0 (2) + EOB (2)
    assert prof["length"].tolist() == [5, 14, 40, 5, 4, 2, 4, 2, 4, 2, 2, 2, 2]
    assert prof["offset"].tolist()[:5] == [0, 5, 19, 59, 64] and prof["table"].tolist() == [0] * 9 + [1] * 4
    assert prof["zrl_codes"] == [[0, 1, 1, 0], [0, 0, 0, 0]] and prof["runs"] == [{16, 45}, set()]
    assert prof["longest"] == [40, 2] and prof["two_word"] == [1, 0] and prof["three_word"] == [0, 0]   # 19 + 40 = 59: two words
    assert prof["dc_categories"] == [{0, 2}, {0}] and prof["ac_sizes"] == [{1, 2}, set()]
    assert prof["blocks"] == 6 and prof["blocks_without_eob"] == 1
    assert prof["total_bits"] == 88 and prof["nb"] == 11 and prof["pad_bits"] == 0 and len(prof["ff_positions"]) == 1
    assert jr.unstuffed_scan(prof["lanes"])[:3] == bytes([0b01111_111, 0b11111001, 0b00_1_11111])
    # DC 100 is category 7 (5 + 7 bits): the 40-bit code now starts at 12 + 14 = 26 and 26 + 40 > 64 takes a third word
    coef[0, 0, 0] = 100
    prof = jr.scan_profile(coef)
    assert prof["offset"].tolist()[:4] == [0, 12, 26, 66] and prof["three_word"] == [1, 0] and prof["two_word"] == [1, 0]
    assert prof["pad_bits"] == 2 and not jr.last_byte_is_ff(prof)


def test_every_path_is_reached_in_each_table():
    profs = _all_profiles()
    for t, table in TABLES:
        for z in (1, 2, 3):
            best = max(p["zrl_codes"][t][z] for _, _, p in profs)
            assert best >= 3, f"{table}: no case with 3 codes of {z} ZRLs"
        runs = set().union(*(p["runs"][t] for _, _, p in profs))
        assert {15, 16, 32, 48, 62} <= runs, (table, sorted(runs))
        assert max(p["three_word"][t] for _, _, p in profs) >= 3, f"{table}: fewer than 3 three-word lane codes in any case"
        assert max(p["longest"][t] for _, _, p in profs) >= 50, table
        assert any(11 in p["dc_categories"][t] for _, _, p in profs), f"{table}: DC category 11 not reached"
    assert any(10 in p["ac_sizes"][0] for _, _, p in profs), "AC size 10 not reached in luminance"
    assert any(p["blocks_without_eob"] for _, _, p in profs) and any(p["blocks"] > p["blocks_without_eob"] for _, _, p in profs)
    assert any(jr.last_byte_is_ff(p) for _, _, p in profs), "no case whose padded last byte is 0xFF"
    assert any(p["pad_bits"] == 0 for _, _, p in profs), "no case without padding"


def test_the_named_cases_sit_where_their_builders_say():
    """The GPU tests lean on particular cases for particular paths (the capacity sweep on the luminance image at quality 95)."""
    for t, name in ((0, "single_coefficient_luma/q95"), (1, "single_coefficient_chroma/q95")):
        prof, = jc.profiles(name)
        assert min(prof["zrl_codes"][t][1:]) >= 3 and prof["three_word"][t] >= 3 and prof["longest"][t] >= 50, name
    for t, name in ((0, "single_coefficient_luma/q1"), (1, "single_coefficient_chroma/q1")):
        prof, = jc.profiles(name)        # every divisor 255: nothing but the one coefficient survives, the runs are k - 1
        assert prof["runs"][t] == {k - 1 for k in jc.SINGLE_K} and prof["zrl_codes"][t] == [12, 12, 12, 12], name
    prof, = jc.profiles("single_coefficient_luma/q95")
    assert 10 in prof["ac_sizes"][0] and len(prof["ff_positions"]) >= 24          # dozens of stuffed bytes for the sweep
    prof, = jc.profiles("dc_swing/q100")
    assert 11 in prof["dc_categories"][0] and 11 in prof["dc_categories"][1]
    signs = {(c[2], c[0] >> 10 & 1) for c in prof["lanes"] if c[3] == 0 and c[6] == 11}     # a value's first bit: 1 = positive
    assert signs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    prof, = jc.profiles("shapes/ff_tail")
    assert jr.last_byte_is_ff(prof) and prof["pad_bits"] == 4
    assert [p["blocks"] for p in jc.profiles("shapes/batch3_t5_16x16")] == [30, 30, 30]


def test_long_scan_takes_the_later_rounds_of_both_serial_passes():
    prof, = jc.profiles("long_scan/q100")
    per_round = jr.ff_per_round(prof)
    assert len(per_round) >= 5 and (per_round > 0).all(), per_round
    assert per_round[1:].sum() > per_round[0]                       # most of the carried count is at work
    assert jr.ff_at_piece_offset(prof, 15, first_round=1) >= 1      # the 0x00 goes into the next lane's place
    assert jr.ff_at_piece_offset(prof, 0, first_round=1) >= 1
    assert prof["blocks"] > 1024 and prof["blocks_without_eob"] > 0          # a second round of the size pass, with full blocks
    assert int((prof["offset"][prof["offset"] >= 8 * jr.STUFF_ROUND_BYTES] & 31).max()) == 31


def test_quality_grid_covers_the_clamp_and_both_formulas():
    """q = 1 clamps every divisor to 255 and q = 2 all but one (10 * 2500 / 100 = 250); 24 is the first quality that clamps
    none (121 * 208 / 100 = 252) and has a truncated 5000 / q (208.3), 25 an exact one; 49 / 50 / 51 lie around the change from
    5000 / q to 200 - 2 q."""
    counts = {q: [int((t == 255).sum()) for t in jr.quant_tables(q)] for q in jc.GRID_QUALITIES}
    assert counts[1] == [64, 64] and counts[2] == [63, 64]
    assert counts[24] == counts[25] == [0, 0] and int(jr.quant_tables(24)[0].max()) == 252 and int(jr.quant_tables(25)[0].max()) == 242
    assert int(jr.quant_tables(23)[0].max()) == 255
    assert counts[49] == counts[50] == counts[51] == [0, 0]
    assert [jr.quant_tables(q)[0][0] for q in (49, 50, 51)] == [16, 16, 16] and jr.quant_tables(49)[0][63] != jr.quant_tables(50)[0][63]
    for content in ("noise", "checker"):
        files = [jc.expected(f"quality_grid/{content}/q{q}")[0] for q in jc.GRID_QUALITIES]
        assert len({f[:jr.HEADER_BYTES] for f in files}) >= 6         # (1 and 2 may share their tables)


def _pil_encode(bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pil_byte_for_byte(name):
    pytest.importorskip("PIL")
    frames, q = jc.CASES[name]
    for f, ours in enumerate(jc.expected(name)):
        pil = _pil_encode(np.hstack(list(frames[f])), q)
        assert ours[:jr.HEADER_BYTES] == pil[:jr.HEADER_BYTES], (f, "header")
        assert ours == pil, (f, len(ours), len(pil))


@pytest.mark.parametrize("golden", sorted(jc.GOLDEN))
def test_goldens_hold_the_builders_images_and_files(golden):
    g = load_golden(golden)
    tiles, qualities = jc.GOLDEN[golden]()
    assert np.array_equal(g["tiles"], tiles) and g["tiles"].dtype == np.uint8
    assert g["qualities"].tolist() == list(qualities)
    for i, q in enumerate(qualities):
        assert g[f"jpeg_{i}"].tobytes() == jc.expected(f"{golden[len('jpeg_'):]}/q{q}")[0], (golden, q)
