"""Constructed images for the preview stream's entropy coder (csrc/jpeg_kernels.hip), plain NumPy.

Noise, dots, a checkerboard and flat images never reach the coder's rare paths: a code with two or three ZRL symbols, a lane
code long enough to spill into a third 32-bit word of the emit pass, the chrominance ZRL, DC category 11, the later rounds of
the stuff pass.  The builders here put images ON those paths; jpeg_reference.scan_profile() says what a scan reaches, and
tests/test_jpeg_cases_cpu.py holds every builder to what it is meant for.

A builder returns (tiles [T][H][W][3] uint8, qualities it is meant for); `shapes` returns several by name, batches among them, and `CASES`
flattens all of it to name -> (frames [F][T][H][W][3], quality).  What a case SHOULD give never comes from the device: expected()
is jpeg_reference.encode_tiles, computed once per case and shared; do not write into it.
"""
import functools

import numpy as np

import jpeg_reference as jr

# zigzag positions of the single coefficients: run = k - 1, so 15 / 16, 31 / 32 and 47 / 48 sit on either side of a ZRL count
SINGLE_K = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
SINGLE_A = (120, -120, 60, -60, 20, -20, 9, -9)
SINGLE_QUALITIES = (100, 95, 75, 1)
GRID_QUALITIES = (1, 2, 24, 25, 49, 50, 51)


def basis_block(k, amplitude):
    """8 x 8 samples 128 + A * cos * cos of the DCT basis function at zigzag position k (|A| <= 127), float64."""
    v, u = divmod(int(jr.ZIGZAG[k]), 8)
    x = (2 * np.arange(8) + 1) * np.pi / 16
    return 128.0 + amplitude * np.outer(np.cos(v * x), np.cos(u * x))


def _single_plane():
    """[16][384]: 96 blocks, one coefficient each, amplitudes fastest."""
    blocks = [basis_block(k, a) for k in SINGLE_K for a in SINGLE_A]
    rows = [np.hstack(blocks[r * 48:(r + 1) * 48]) for r in range(2)]
    return np.clip(np.rint(np.vstack(rows)), 0, 255)


def _split(img, T):
    return np.ascontiguousarray(np.stack(np.split(img, T, axis=1))).astype(np.uint8)


def single_coefficient_luma():
    """Grey blocks with one luminance coefficient each: 2 tiles of 16 x 192."""
    grey = _single_plane()
    return _split(np.repeat(grey[..., None], 3, axis=2), 2), SINGLE_QUALITIES


def single_coefficient_chroma():
    """The same coefficients in Cb, with Y = Cr = 128: Cb is upsampled 2 x 2 and converted to BGR (JFIF's inverse; blue clips
    for the largest amplitudes, which only adds coefficients).  2 tiles of 32 x 384."""
    cb = np.kron(_single_plane(), np.ones((2, 2))) - 128.0
    bgr = np.stack([128 + 1.772 * cb, 128 - 0.344136 * cb, np.full_like(cb, 128.0)], axis=2)
    return _split(np.clip(np.rint(bgr), 0, 255), 2), SINGLE_QUALITIES


def dc_swing():
    """Rows of MCUs that alternate between two flat colours, each row in both orders: the DC differences of luminance
    (black / white: -1024 <-> 1016) and of both chrominance planes (blue / yellow, red / cyan) are in category 11 with
    either sign at quality 100.  2 tiles of 96 x 32."""
    pairs = (((255, 0, 0), (0, 255, 255)), ((0, 0, 255), (255, 255, 0)), ((0, 0, 0), (255, 255, 255)))
    rows = []
    for first, second in pairs:
        for a, b in ((first, second), (second, first)):
            row = np.empty((16, 64, 3), np.uint8)
            for m in range(4):
                row[:, 16 * m:16 * m + 16] = a if m % 2 == 0 else b
            rows.append(row)
    return _split(np.vstack(rows), 2), (100,)


def long_scan():
    """Uniform noise at quality 100, 2 tiles of 160 x 144: 1 080 blocks (a second round of the size pass) and a scan of
    several rounds of the stuff pass."""
    return np.stack([jr.content("noise", 160, 144, seed=41 + t) for t in range(2)]), (100,)


def quality_grid(content):
    """32 x 48, 2 tiles: below 50 (5000 / q, truncated at 24 and exact at 25), at the clamp to 255 (q = 1 clamps every
    divisor, q = 2 all but one, 24 is the first quality that clamps none) and around the change of formula at 50."""
    return np.stack([jr.content(content, 32, 48, seed=23 + t) for t in range(2)]), GRID_QUALITIES


def shapes():
    """name -> (frames [F][T][H][W][3], quality): one MCU per tile and an odd MCU count, one MCU column, a batch whose
    four-MCU workgroups straddle two images twice (5 MCUs each), and one MCU whose scan ends in four 1 bits of a value and
    four of padding: the padded last byte is 0xFF and takes a stuffed 0x00 in front of the EOI (of the noise seeds 0 .. 399
    about one in eight ends so; this one has the fewest pad bits)."""
    def noise(T, H, W, seed):
        return np.stack([jr.content("noise", H, W, seed=seed + t) for t in range(T)])
    return {
        "t5_16x16": (noise(5, 16, 16, 61)[None], 95),
        "t1_64x16": (noise(1, 64, 16, 67)[None], 95),
        "batch3_t5_16x16": (np.stack([noise(5, 16, 16, 71 + 5 * f) for f in range(3)]), 95),
        "ff_tail": (noise(1, 16, 16, 365)[None], 100),
    }


def _build():
    out = {}
    for name, builder in (("single_coefficient_luma", single_coefficient_luma), ("single_coefficient_chroma", single_coefficient_chroma),
                          ("dc_swing", dc_swing), ("long_scan", long_scan)):
        tiles, qualities = builder()
        for q in qualities:
            out[f"{name}/q{q}"] = (tiles[None], q)
    for content in ("noise", "checker"):
        tiles, qualities = quality_grid(content)
        for q in qualities:
            out[f"quality_grid/{content}/q{q}"] = (tiles[None], q)
    for name, (frames, q) in shapes().items():
        out[f"shapes/{name}"] = (frames, q)
    for frames, _ in out.values():
        frames.setflags(write=False)
    return out


CASES = _build()
GOLDEN = {"jpeg_single_coefficient_luma": single_coefficient_luma, "jpeg_single_coefficient_chroma": single_coefficient_chroma,
          "jpeg_dc_swing": dc_swing}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The files of a case, one per image."""
    frames, q = CASES[name]
    return tuple(jr.encode_tiles(frames[f], q) for f in range(frames.shape[0]))


@functools.lru_cache(maxsize=None)
def profiles(name):
    """scan_profile() of every image of a case."""
    frames, q = CASES[name]
    return tuple(jr.scan_profile(jr.coefficients(np.hstack(list(frames[f])), q)) for f in range(frames.shape[0]))
