"""NumPy restatement of the baseline JPEG file libjpeg writes with its defaults (what cv.imencode('.jpg', img) and
PIL's save(..., 'JPEG', quality=q, subsampling=2, optimize=False) produce): baseline sequential, YCbCr 4:2:0, JDCT_ISLOW,
Annex-K Huffman tables, no restart markers, JFIF 1.01 APP0.  Whole file, any H and W that are multiples of 16, any
quality 1..100.  Every step is integer arithmetic, so the target is byte identity (tests/test_jpeg_reference_cpu.py
checks it against PIL; the device encoder is checked against this file).  Test code: the product never imports it."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]

HEADER_BYTES = 623


def quant_tables(quality):
    """(luma, chroma) divisors in natural order (jcparam.c: jpeg_quality_scaling + jpeg_add_quant_table, baseline clamp)."""
    if not 1 <= quality <= 100:
        raise ValueError("quality must be 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (STD_LUMA, STD_CHROMA))


def huffman_codes(bits, vals):
    """symbol -> (code, length) of a table given as Annex C counts and values (jchuff.c: jpeg_make_c_derived_tbl)."""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(H, W, quality):
    """The 623 bytes in front of the scan: SOI, APP0, DQT 0, DQT 1, SOF0, DHT DC0 AC0 DC1 AC1, SOS."""
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        n = 19 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def ycc(bgr):
    """jccolor.c rgb_ycc_convert; channel 2 of the BGR frame is R.  int64 planes Y, Cb, Cr."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample(p):
    """jcsample.c h2v2_downsample: bias 1, 2, 1, 2 ... along every output row."""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, rows):
    """One pass of jfdctint.c along the last axis of d [..., 8]."""
    s = 11 if rows else 15
    t0, t1, t2, t3 = d[..., 0] + d[..., 7], d[..., 1] + d[..., 6], d[..., 2] + d[..., 5], d[..., 3] + d[..., 4]
    t7, t6, t5, t4 = d[..., 0] - d[..., 7], d[..., 1] - d[..., 6], d[..., 2] - d[..., 5], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    if rows:
        o[..., 0] = (t10 + t11) << 2
        o[..., 4] = (t10 - t11) << 2
    else:
        o[..., 0] = _descale(t10 + t11, 2)
        o[..., 4] = _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[..., 2] = _descale(z1 + t13 * 6270, s)
    o[..., 6] = _descale(z1 - t12 * 15137, s)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = _descale(t4 + z1 + z3, s)
    o[..., 5] = _descale(t5 + z2 + z4, s)
    o[..., 3] = _descale(t6 + z2 + z3, s)
    o[..., 1] = _descale(t7 + z1 + z4, s)
    return o


def fdct(blocks):
    """jfdctint.c on blocks [..., 8, 8] of samples (level shift inside): rows, then columns; output scaled by 8."""
    d = _dct_pass(blocks.astype(np.int64) - 128, True)
    return np.swapaxes(_dct_pass(np.swapaxes(d, -1, -2), False), -1, -2)


def quantise(coef, q):
    """jcdctmgr.c: sign(c) * ((|c| + 4Q) / (8Q)); coef [..., 8, 8], q [64] natural order -> [..., 64] zigzag order."""
    c = coef.reshape(coef.shape[:-2] + (64,))
    v = np.sign(c) * ((np.abs(c) + 4 * q) // (8 * q))
    return v[..., ZIGZAG]


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def coefficients(bgr, quality):
    """Quantised zigzag coefficients in scan order: [MCUs][6][64] (Y00 Y01 Y10 Y11 Cb Cr)."""
    H, W = bgr.shape[:2]
    if H % 16 or W % 16 or H < 16 or W < 16:
        raise ValueError("H and W must be multiples of 16")
    ql, qc = quant_tables(quality)
    y, cb, cr = ycc(bgr)
    yq = quantise(fdct(_blocks(y)), ql)                    # [H/8][W/8][64]
    cbq = quantise(fdct(_blocks(downsample(cb))), qc)      # [H/16][W/16][64]
    crq = quantise(fdct(_blocks(downsample(cr))), qc)
    my, mx = H // 16, W // 16
    out = np.empty((my, mx, 6, 64), np.int64)
    out[:, :, 0] = yq[0::2, 0::2]
    out[:, :, 1] = yq[0::2, 1::2]
    out[:, :, 2] = yq[1::2, 0::2]
    out[:, :, 3] = yq[1::2, 1::2]
    out[:, :, 4] = cbq
    out[:, :, 5] = crq
    return out.reshape(my * mx, 6, 64)


_DC = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
_AC = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def scan_symbols(coef):
    """jchuff.c encode_one_block over [MCUs][6][64]: the (code, length) pairs of the scan, and the symbols' byte values
    (tests look for ZRL 0xF0 there)."""
    codes, lens, syms = [], [], []

    def put(code, n):
        codes.append(code)
        lens.append(n)

    def put_value(v, n):
        if n:
            put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)

    last_dc = [0, 0, 0]
    comp_of = (0, 0, 0, 0, 1, 2)
    for mcu in coef:
        for b in range(6):
            blk = mcu[b]
            comp = comp_of[b]
            tbl = 0 if comp == 0 else 1
            diff = int(blk[0]) - last_dc[comp]
            last_dc[comp] = int(blk[0])
            n = abs(diff).bit_length()
            put(*_DC[tbl][n])
            put_value(diff, n)
            prev = 0
            for k in np.nonzero(blk[1:])[0] + 1:
                run = int(k) - prev - 1
                while run > 15:
                    put(*_AC[tbl][0xF0])
                    syms.append(0xF0)
                    run -= 16
                v = int(blk[k])
                n = abs(v).bit_length()
                put(*_AC[tbl][run << 4 | n])
                syms.append(run << 4 | n)
                put_value(v, n)
                prev = int(k)
            if prev < 63:
                put(*_AC[tbl][0])
                syms.append(0)
    return np.array(codes, np.int64), np.array(lens, np.int64), syms


def pack_scan(codes, lens):
    """MSB-first bit string, last byte padded with 1 bits, every 0xFF followed by 0x00."""
    total = int(lens.sum())
    idx = np.repeat(np.arange(len(lens)), lens)
    starts = np.cumsum(lens) - lens
    pos = np.arange(total) - starts[idx]
    bits = ((codes[idx] >> (lens[idx] - 1 - pos)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    raw = np.packbits(bits)
    out = np.zeros((len(raw), 2), np.uint8)
    out[:, 0] = raw
    keep = np.ones((len(raw), 2), bool)
    keep[:, 1] = raw == 0xFF
    return out[keep].tobytes()


STUFF_ROUND_BYTES = 1024 * 16     # scan bytes one round of the device's stuff pass takes: 1 024 lanes, a 16-byte piece each


def lane_codes(coef):
    """The scan of [MCUs][6][64] cut the way the device cuts it: one "lane code" per zigzag position that codes anything.
    Position 0 is the DC code plus its value bits; a non-zero AC position is its ZRL symbols, its run/size symbol and its
    value bits; position 63, when zero, is the EOB.  Written from the coefficients on its own, not from scan_symbols():
    tests/test_jpeg_cases_cpu.py requires that the lane codes, concatenated, are pack_scan()'s bytes.
    -> list of (bits, length, table, position, run, zrls, size); run and zrls are -1 for DC codes and EOBs."""
    out = []
    last_dc = [0, 0, 0]
    for mcu in np.asarray(coef).tolist():
        for b, blk in enumerate(mcu):
            comp = (0, 0, 0, 0, 1, 2)[b]
            tbl = min(comp, 1)
            diff = blk[0] - last_dc[comp]
            last_dc[comp] = blk[0]
            size = abs(diff).bit_length()
            code, n = _DC[tbl][size]
            out.append((code << size | ((diff if diff >= 0 else diff - 1) & ((1 << size) - 1)), n + size, tbl, 0, -1, -1, size))
            prev = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    continue
                run = k - prev - 1
                prev = k
                bits, n = 0, 0
                zc, zn = _AC[tbl][0xF0]
                for _ in range(run // 16):
                    bits, n = bits << zn | zc, n + zn
                size = abs(v).bit_length()
                c, cn = _AC[tbl][(run % 16) << 4 | size]
                bits = (bits << cn | c) << size | ((v if v >= 0 else v - 1) & ((1 << size) - 1))
                out.append((bits, n + cn + size, tbl, k, run, run // 16, size))
            if blk[63] == 0:
                c, cn = _AC[tbl][0]
                out.append((c, cn, tbl, 63, -1, -1, 0))
    return out


def scan_profile(coef):
    """Which paths of the device's entropy coder the scan of [MCUs][6][64] reaches (csrc/jpeg_kernels.hip: the emit pass
    writes a lane code into up to three 32-bit words, ac_code loops once per ZRL, the stuff pass takes STUFF_ROUND_BYTES per
    round in 16-byte pieces).  Per-table entries are indexed 0 = luminance, 1 = chrominance."""
    lanes = lane_codes(coef)
    length = np.array([c[1] for c in lanes], np.int64)
    offset = np.cumsum(length) - length
    table = np.array([c[2] for c in lanes], np.int64)
    zrls = np.array([c[5] for c in lanes], np.int64)
    is_dc = np.array([c[3] == 0 for c in lanes])
    total = int(length.sum())
    span = (offset & 31) + length
    raw = np.frombuffer(unstuffed_scan(lanes), np.uint8)
    coef = np.asarray(coef)
    prof = {
        "lanes": lanes, "length": length, "offset": offset, "table": table,
        "zrl_codes": [[int(((table == t) & (zrls == z)).sum()) for z in range(4)] for t in range(2)],
        "runs": [{c[4] for c in lanes if c[2] == t and c[4] >= 0} for t in range(2)],
        "longest": [int(length[table == t].max()) if (table == t).any() else 0 for t in range(2)],
        "three_word": [int(((table == t) & (span > 64)).sum()) for t in range(2)],
        "two_word": [int(((table == t) & (span > 32)).sum()) for t in range(2)],
        "dc_categories": [{c[6] for c in lanes if c[2] == t and c[3] == 0} for t in range(2)],
        "ac_sizes": [{c[6] for c in lanes if c[2] == t and c[4] >= 0} for t in range(2)],
        "blocks": int(is_dc.sum()),
        "blocks_without_eob": int((coef[:, :, 63] != 0).sum()),
        "total_bits": total, "nb": (total + 7) // 8, "pad_bits": (-total) % 8,
        "ff_positions": np.nonzero(raw == 0xFF)[0],
    }
    assert prof["nb"] == len(raw)
    return prof


def unstuffed_scan(lanes):
    """The lane codes as one MSB-first bit string, its last byte padded with 1 bits; no 0x00s inserted."""
    text = "".join(format(c[0], "0%db" % c[1]) for c in lanes)
    text += "1" * ((-len(text)) % 8)
    return int(text, 2).to_bytes(len(text) // 8, "big")


def stuffed(raw):
    return bytes(raw).replace(b"\xff", b"\xff\x00")


def ff_per_round(prof):
    """0xFF bytes each round of the stuff pass meets (the later rounds start from the carried count of the earlier ones)."""
    rounds = max(1, -(-prof["nb"] // STUFF_ROUND_BYTES))
    return np.bincount(prof["ff_positions"] // STUFF_ROUND_BYTES, minlength=rounds)


def ff_at_piece_offset(prof, at, first_round=0):
    """0xFF bytes at byte `at` of their 16-byte piece, in rounds first_round and later."""
    p = prof["ff_positions"]
    return int(((p % 16 == at) & (p // STUFF_ROUND_BYTES >= first_round)).sum())


def last_byte_is_ff(prof):
    return len(prof["ff_positions"]) > 0 and int(prof["ff_positions"][-1]) == prof["nb"] - 1


def profile_line(prof):
    """One line for a test to print before it asserts on the device."""
    t = ("Y", "C")
    return " ".join(
        [f"blocks={prof['blocks']} no_eob={prof['blocks_without_eob']} nb={prof['nb']} pad={prof['pad_bits']}"]
        + [f"{t[i]}:zrl0123={prof['zrl_codes'][i]} longest={prof['longest'][i]} w3={prof['three_word'][i]} w2={prof['two_word'][i]} "
           f"dc<={max(prof['dc_categories'][i])} ac<={max(prof['ac_sizes'][i], default=0)}" for i in range(2)]
        + [f"ff/round={ff_per_round(prof).tolist()} ff@15={ff_at_piece_offset(prof, 15)} ff@0={ff_at_piece_offset(prof, 0)} "
           f"last_ff={last_byte_is_ff(prof)}"])


def encode(bgr, quality=95):
    """The whole file for one BGR image [H][W][3] uint8."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    codes, lens, _ = scan_symbols(coefficients(bgr, quality))
    return header(bgr.shape[0], bgr.shape[1], quality) + pack_scan(codes, lens) + b"\xff\xd9"


def encode_tiles(tiles, quality=95):
    """tiles [T][H][W][3] (the blob stage's `processed` for one frame set) -> the file of their np.hstack."""
    return encode(np.hstack(list(np.asarray(tiles))), quality)


# ---------------------------------------------------------------- test contents (shared by the CPU and the GPU tests)
CONTENTS = ("black", "white", "noise", "dots", "checker")


def content(name, H, W, seed=0):
    """A BGR test image [H][W][3]: all black, all 255, uniform noise, a dark frame with a few bright dots and low noise
    (what the stream looks like), a pure-colour checkerboard at 1-pixel pitch (saturated chroma, maximum swings)."""
    rng = np.random.default_rng(seed + 1000 * CONTENTS.index(name))
    if name == "black":
        return np.zeros((H, W, 3), np.uint8)
    if name == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if name == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if name == "dots":
        img = rng.integers(0, 4, (H, W, 3)).astype(np.int64)
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(max(2, H * W // 4096)):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.0, 3.5)
            img += (255 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r)))[..., None].astype(np.int64)
        return np.clip(img, 0, 255).astype(np.uint8)
    if name == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        cols = np.array([[255, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 255]], np.uint8)
        return cols[((yy + xx) & 1) + 2 * ((yy // 8 + xx // 8) & 1)]
    raise KeyError(name)
