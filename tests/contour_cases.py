"""Crafted masks for the contour kernel (csrc/blob_kernels.hip, blob_contour_kernel), plain NumPy, deterministic.

The whole-image tests reach the kernel only behind a 9x9 Gaussian, which leaves no isolated pixels, no one-pixel lines, no
diagonal contacts, no pixel on two borders, nothing placed on a word seam and no table filled to its cap.  This table holds
those masks.  It is shared by tests/test_contour_cases_cpu.py (the two CPU references agree on it, and every case reaches
the edge its name claims) and tests/test_gpu_contour_kernel.py (the device against the C oracle, exactly).

Next to every mask stand two counts that neither reference computes:
    count_pairs     horizontal pairs = foreground pixels with background at the left, plus those with background at the
                    right, on the zero-padded image: what the kernel's pair table has to hold (P_cap)
    count_contours  borders = 8-connected foreground components + 4-connected background components of the zero-padded
                    image - 1 (the outside): what its contour table has to hold (N_cap)
and, for the named cases, the figures their construction gives in closed form (`pairs`, `contours`, `centroids`).

CENTROIDS ARE NOT RATIONAL CENTROIDS.  The expected centroid of a contour is what the references compute with OpenCV's own
arithmetic, int(a10 * (1/6) / (a00 * 0.5)) in double precision with the constant 0.1666...67, not the exact quotient of the
polygon sums: where the exact centroid is an integer the product with the rounded 1/6 may fall just below it.  The
`truncation` cases sit there on purpose and take their expected values from the references alone.
"""
import numpy as np
from scipy import ndimage

SIZES = (320, 352, 832)          # named topologies: a common edge, one whose last 64-bit mask word is half used, the largest
LDS_CAP = 160 * 1024
SMALL_TABLES = (1024, 128)       # the product's first pass and its second (csrc/blob_capi.hip)
LARGE_TABLES = (8192, 1024)


def lds_bytes(S, P_cap, N_cap):
    """blob_contour_lds_bytes restated (the probe exports the product's own; the GPU test compares the two)."""
    SP = S + 2
    stride = (SP + 31) // 32 + 1
    return 24 * N_cap + 4 * SP * stride + 12 * P_cap + 4 * N_cap + 4 * (4 * N_cap + 1) + 64


def large_tables(S):
    """The largest tables used at edge S: the product's large ones where they fit LDS next to the padded mask, else halved
    pair tables with a contour table of a quarter of them at most (832: 4096 / 256)."""
    P, N = LARGE_TABLES
    while lds_bytes(S, P, N) > LDS_CAP:
        P //= 2
        N = min(N, P // 16)
    return P, N


def pack(masks):
    """[n][S][S] (0 / non-zero) -> uint64 [n][S][ceil(S / 64)], bit x of word x / 64, as the mask kernel writes them."""
    m = np.asarray(masks) != 0
    n, S, _ = m.shape
    words = (S + 63) // 64
    padded = np.zeros((n, S, words * 64), dtype=np.uint8)
    padded[:, :, :S] = m
    return np.ascontiguousarray(np.packbits(padded, axis=2, bitorder="little")).view("<u8").reshape(n, S, words)


def count_pairs(masks):
    m = np.asarray(masks) != 0
    p = np.pad(m, ((0, 0), (0, 0), (1, 1)))
    return ((p[:, :, 1:-1] & ~p[:, :, :-2]).sum(axis=(1, 2)) + (p[:, :, 1:-1] & ~p[:, :, 2:]).sum(axis=(1, 2))).astype(np.int64)


def count_contours(masks):
    out = np.zeros(len(masks), dtype=np.int64)
    for i, m in enumerate(np.asarray(masks) != 0):
        p = np.pad(m, 1)
        out[i] = ndimage.label(p, structure=np.ones((3, 3)))[1] + ndimage.label(~p)[1] - 1
    return out


class Case:
    """A named batch of masks of one size.  pairs / contours / centroids: per-mask figures the construction gives in closed
    form (None where the case states none); min_pairs: a lower bound the case promises instead; overflows: the case is
    meant to exceed even the largest tables (every other case must fit them)."""

    def __init__(self, name, masks, pairs=None, contours=None, centroids=None, min_pairs=None, overflows=False):
        self.name = name
        self.overflows = overflows
        self.masks = np.ascontiguousarray(masks, dtype=np.uint8)
        if self.masks.ndim == 2:
            self.masks = self.masks[None]
        n = len(self.masks)

        def per_mask(v):
            return None if v is None else np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)).copy()
        self.pairs, self.contours, self.centroids = per_mask(pairs), per_mask(contours), per_mask(centroids)
        self.min_pairs = min_pairs
        self.S = self.masks.shape[1]

    def __repr__(self):
        return "%s@%d" % (self.name, self.S)


# ------------------------------------------------------------------------------------------------ exhaustive small patterns
def patterns4(codes=None):
    """[n][4][4]: bit 4 y + x of the code = pixel (y, x); all 65 536 codes by default."""
    codes = np.arange(1 << 16, dtype=np.uint32) if codes is None else np.asarray(codes, dtype=np.uint32)
    return ((codes[:, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1, 4, 4)


def embed(patterns, S, y, x):
    n, h, w = patterns.shape
    out = np.zeros((n, S, S), dtype=np.uint8)
    out[:, y:y + h, x:x + w] = patterns
    return out


SEAM_S, SEAM_X, SEAM_Y = 72, 62, 30           # pattern columns 62..65 straddle the seam of the 64-bit mask words
EXHAUSTIVE_CHUNK = 8192                       # masks per batch: 42 MB of bytes at S = 72
OFFSET_SAMPLE = 2048
OFFSET_XS = tuple(range(26, 34)) + tuple(range(58, 67)) + (SEAM_S - 4,)   # the padded 32-bit words are shifted by one
OFFSET_YS = (0, SEAM_S - 4)                                                # pixel; x = 68, y = 68: bottom-right corner
SMALL_TABLES_4X4 = (32, 8)                    # a 4x4 pattern has <= 2 runs per row = 16 pairs, <= 8 borders; 4 N <= P


def exhaustive_chunks(S):
    """All 4x4 patterns as the whole image (S = 4) or across the word seam (S = 72), in chunks."""
    for lo in range(0, 1 << 16, EXHAUSTIVE_CHUNK):
        p = patterns4(np.arange(lo, lo + EXHAUSTIVE_CHUNK))
        yield lo, (p if S == 4 else embed(p, S, SEAM_Y, SEAM_X))


def offset_sample_codes():
    return np.random.default_rng(20240611).choice(1 << 16, OFFSET_SAMPLE, replace=False)


def offset_batches():
    p = patterns4(offset_sample_codes())
    for y in OFFSET_YS:
        for x in OFFSET_XS:
            yield (y, x), embed(p, SEAM_S, y, x)


# ------------------------------------------------------------------------------------------------------- random dense masks
DENSITIES = (0.3, 0.5, 0.7)
RANDOM8_N = 50000
RANDOM_SIZES = (30, 31, 32, 33, 62, 63, 64, 65)   # row stride of the padded mask and its spare word change here
RANDOM_SIZED_N = 384    # per size: a mask has 14 .. 66 times the pixels of an 8x8 one and up to ~600 borders; the references'
                        # time per mask grows alike, and 8 sizes x 384 keep both test files within seconds


def random_masks(S, n, seed):
    rng = np.random.default_rng(seed)
    dens = np.repeat(DENSITIES, -(-n // len(DENSITIES)))[:n]
    return (rng.random((n, S, S)) < dens[:, None, None]).astype(np.uint8)


def random8():
    return random_masks(8, RANDOM8_N, 8)


def random_sized(S):
    return random_masks(S, RANDOM_SIZED_N, 1000 + S)


# -------------------------------------------------------------------------------------------------------- named topologies
def _blank(S, n=None):
    return np.zeros((S, S) if n is None else (n, S, S), dtype=np.uint8)


def rings_mask(S, cy, cx, R, t):
    """Square bands of thickness t around (cy, cx), alternately foreground and background from the Chebyshev radius R
    inwards.  Returns mask, pairs, contours (closed form)."""
    yy, xx = np.mgrid[0:S, 0:S]
    d = np.maximum(abs(yy - cy), abs(xx - cx))
    m = ((d <= R) & (((R - d) // t) % 2 == 0)).astype(np.uint8)
    pairs = contours = 0
    for b in range(0, R // t + 1, 2):
        ro, ri = R - b * t, R - (b + 1) * t    # band = ri < d <= ro
        if ri < 0:
            pairs += 2 * (2 * ro + 1)           # the solid centre square
            contours += 1
        else:
            pairs += 4 * (2 * ri + 1) + 4 * (ro - ri)
            contours += 2
    return m, pairs, contours


def comb_mask(S, y0, x0, teeth, h):
    """A spine 3 rows thick with `teeth` one-pixel teeth of height h, one column apart: one outer border."""
    m = _blank(S)
    m[y0 + h:y0 + h + 3, x0:x0 + 2 * teeth - 1] = 1
    m[y0:y0 + h, x0:x0 + 2 * teeth - 1:2] = 1
    return m, 6 + 2 * teeth * h


def spiral_mask(S, y0, x0, size):
    """A one-pixel wall spiralling inwards with a one-pixel channel between the turns: one component, no hole."""
    m = _blank(S)
    moves = [size - 1] * 3
    for k in range(size - 3, 0, -2):
        moves += [k, k]
    y, x, dy, dx = y0, x0, 0, 1
    m[y, x] = 1
    for k in moves:                      # right, down, left, up, ... each wall two short of the one it runs along
        for _ in range(k):
            y += dy
            x += dx
            m[y, x] = 1
        dy, dx = dx, -dy
    return m


def bars_mask(S, pairs, h_max=256):
    """Vertical one-pixel bars one column apart, pairs / 2 pixels in all: 2 pairs per pixel, one contour per bar."""
    assert pairs % 2 == 0
    m = _blank(S)
    left, x = pairs // 2, 1
    h_max = min(h_max, S - 2)
    while left > 0:
        h = min(left, h_max)
        m[1:1 + h, x] = 1
        left -= h
        x += 2
    assert x <= S
    return m, -(-(pairs // 2) // h_max)


def dots_mask(S, n, per_row=32):
    """n isolated pixels on a grid of pitch 2: 2 n pairs, n contours, no centroid."""
    m = _blank(S)
    i = np.arange(n)
    m[1 + 2 * (i // per_row), 1 + 2 * (i % per_row)] = 1
    return m


def named_cases(S):
    """The named topologies at edge S, sized to the largest tables that fit there (large_tables(S))."""
    P_max, N_max = large_tables(S)
    c = S // 2
    out = []
    # single pixels: the four corners, and both sides of the 32- and 64-bit word seams
    spots = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)] + [(c, x) for x in (31, 32, 63, 64)]
    m = _blank(S, len(spots))
    for i, (y, x) in enumerate(spots):
        m[i, y, x] = 1
    out.append(Case("single_pixels", m, 2, 1, 0))
    out.append(Case("full", np.ones((S, S), np.uint8), 2 * S, 1, 1))
    m = np.ones((S, S), np.uint8)
    m[1:-1, 1:-1] = 0
    out.append(Case("border_frame", m, 4 * S - 4, 2, 2))
    # one-pixel lines: a00 = 0, a contour without a centroid
    L = 200
    m = _blank(S, 4)
    m[0, c, 5:S - 5] = 1
    m[1, 20:20 + L, 63] = 1
    i = np.arange(L)
    m[2, 20 + i, 20 + i] = 1
    m[3, 20 + i, 20 + L - 1 - i] = 1
    out.append(Case("lines_h_v_diag_anti", m, [2, 2 * L, 2 * L, 2 * L], 1, 0))
    # two squares in contact through one diagonal step, which falls on the word seam: one outer border
    a = 10
    m = _blank(S)
    m[40:40 + a, 64 - a:64] = 1
    m[40 + a:40 + 2 * a, 64:64 + a] = 1
    out.append(Case("diagonal_squares", m, 4 * a, 1, 1))
    # one-pixel holes touching diagonally: the background is 4-connected, so each is a hole of its own
    m = _blank(S, 2)
    m[:, 50:62, 26:38] = 1
    m[0, 55, 31] = m[0, 56, 32] = 0
    m[1, 54, 30] = m[1, 55, 31] = m[1, 56, 32] = 0
    out.append(Case("diagonal_holes_2_3", m, [24 + 4, 24 + 6], [3, 4], [3, 4]))
    # a ring one pixel thick: its outer and its hole border share every pixel
    m = _blank(S)
    m[30:50, 25:40] = 1
    m[31:49, 26:39] = 0
    out.append(Case("thin_ring", m, 4 * 20 - 4, 2, 2))
    # ring, hole, island, ... : thickness 2, seven borders deep
    m, p, n = rings_mask(S, 100, 100, 13, 2)
    out.append(Case("nested_depth_7", m, p, n, n))
    assert n == 7
    # one-pixel rings one pixel apart: every pixel on two borders, pairs >> contours.  r rings carry 8 r^2 pairs: 32 rings
    # fill the 8 192-pair table exactly; 50 rings (20 000 pairs) fit no table and must come back as a table overflow
    r = int(np.sqrt(P_max // 8))
    m, p, n = rings_mask(S, 120, 130, 2 * r - 1, 1)
    assert n == 2 * r and p == 8 * r * r
    out.append(Case("nested_rings_%d" % r, m, p, n, n))
    m, p, n = rings_mask(S, 120, 130, 99, 1)
    assert n == 100 and p == 20000
    out.append(Case("nested_rings_50", m, p, n, n, overflows=True))
    # checkerboard: one 8-connected component, every interior background pixel a hole: contours ~ pairs / 2
    k = 2 * (int(np.sqrt(2 * (N_max - 1))) // 2) + 2
    while 1 + (k - 2) ** 2 // 2 > N_max:
        k -= 2
    yy, xx = np.mgrid[0:k, 0:k]
    m = _blank(S)
    m[10:10 + k, 20:20 + k] = (yy + xx) % 2 == 0
    out.append(Case("checkerboard_%d" % k, m, k * k, 1 + (k - 2) ** 2 // 2, 1 + (k - 2) ** 2 // 2))
    # grid of isolated pixels: N_max contours, no centroid
    g = int(np.sqrt(N_max))
    out.append(Case("isolated_grid_%d" % (g * g), dots_mask(S, g * g, g), 2 * g * g, g * g, 0))
    # one border with thousands of pairs: the last pointer-jumping rounds, the minimum of one long cycle
    teeth, h = (60, 50) if P_max >= 8192 else (40, 50)
    m, p = comb_mask(S, 30, 30, teeth, h)
    out.append(Case("comb", m, p, 1, 1))
    size, least = (101, 4000) if P_max >= 8192 else (81, 2500)
    out.append(Case("spiral", spiral_mask(S, 40, 60, size), None, 1, 1, min_pairs=least))
    # siblings whose starts lie on one row (reverse discovery order), free and inside one hole
    m = _blank(S, 2)
    for i in range(7):
        m[:, 60:63 + i, 30 + 6 * i:33 + 6 * i] = 1
    m[1, 50:80, 20:80] = 1
    m[1, 52:78, 22:78] = 0
    for i in range(7):
        m[1, 60:63 + i, 30 + 6 * i:33 + 6 * i] = 1
    out.append(Case("siblings_free_in_hole", m, [7 * 6 + 2 * sum(range(7)), 7 * 6 + 2 * sum(range(7)) + 2 * 30 + 2 * 26], [7, 9], [7, 9]))
    # the left walk of the parent rule.  [0]: blobs whose start row passes through the hole of a thin ring: the one inside
    # the hole meets a pixel that lies on both borders of the ring through its hole side (child of the hole), the one right
    # of the ring through its outer side (sibling).  [1]: a hole start in a run whose inner pixels lie on another hole's
    # border (the hole above the run): the hole is still a child of the block's outer border
    m = _blank(S, 2)
    m[0, 30:50, 25:45] = 1
    m[0, 31:49, 26:44] = 0
    m[0, 35:38, 33:36] = 1
    m[0, 35:38, 50:53] = 1
    m[1, 60:74, 20:50] = 1
    m[1, 62:64, 32:35] = 0
    m[1, 64:67, 40:43] = 0
    out.append(Case("left_walk_outer_hole", m, [4 * 20 - 4 + 12, 2 * 14 + 2 * 2 + 2 * 3], [4, 3], [4, 3]))
    # centroid truncation (see the header): rectangles and rectangular holes with an integer / a half centroid, up to S - 1
    m = _blank(S, 6)
    m[0, 30:41, 10:21] = 1
    m[1, 30:42, 10:22] = 1
    m[2, S - 9:S, S - 9:S] = 1
    m[3, S - 10:S, S - 10:S] = 1
    m[4, S - 40:S, S - 40:S] = 1
    m[4, S - 12:S - 1, S - 12:S - 1] = 0
    m[5, S - 40:S, S - 40:S] = 1
    m[5, S - 13:S - 1, S - 13:S - 1] = 0
    out.append(Case("truncation", m, [22, 24, 18, 20, 80 + 22, 80 + 24], [1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 2]))
    return out


SMALL_NAMES = ("single_pixels", "full", "border_frame", "lines_h_v_diag_anti", "diagonal_squares", "diagonal_holes_2_3", "thin_ring",
               "nested_depth_7", "siblings_free_in_hole", "left_walk_outer_hole", "truncation")


def all_named():
    """Every named case at 320 and 832, the small ones also at 352."""
    out = []
    for S in SIZES:
        out += [c for c in named_cases(S) if S != 352 or c.name in SMALL_NAMES]
    return out


# --------------------------------------------------------------------------------------------------------------------- caps
CAP_S = 320
CAP_TIERS = (((64, 16), SMALL_TABLES), (SMALL_TABLES, LARGE_TABLES))   # (first pass, second pass) table sizes


def cap_batch(first, second):
    """Masks at and just over the tables of a first pass (P1, N1) and of a second pass (P2, N2), mixed with fitting ones.
    Returns masks, pairs, contours (closed form)."""
    (P1, N1), (P2, N2) = first, second
    masks, pairs, conts = [], [], []

    def add(m, p, n):
        masks.append(m)
        pairs.append(p)
        conts.append(n)
    add(dots_mask(CAP_S, 3), 6, 3)                               # fits
    for P in (P1, P1 + 2, P2, P2 + 2):                           # pairs exactly at the cap / one pixel more
        m, n = bars_mask(CAP_S, P)
        add(m, P, n)
    add(_blank(CAP_S), 0, 0)                                     # empty image between them
    for N in (N1, N1 + 1, N2, N2 + 1):                           # contours exactly at the cap / one more
        add(dots_mask(CAP_S, N), 2 * N, N)
    m = _blank(CAP_S)
    m[100:110, 100:120] = 1
    add(m, 20, 1)                                                # fits, last of the batch
    return np.stack(masks), np.array(pairs), np.array(conts)
