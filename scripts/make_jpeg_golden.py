"""Writes tests/golden/jpeg_*.npz: small tile sets and the JPEG files libjpeg writes for them (the preview stream's contract,
tests/jpeg_reference.py).  Run where PIL is installed: every golden is encoded by the NumPy restatement AND by PIL
(libjpeg-turbo), and nothing is written unless the two agree byte for byte -- the goldens carry the libjpeg pin to machines
without PIL.  Usage: python scripts/make_jpeg_golden.py"""
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases as jc  # noqa: E402
import jpeg_reference as jr  # noqa: E402

# name -> (content, tiles, H, W, qualities), or -> a builder of tests/jpeg_cases.py (constructed images: long zero runs
# in either table, DC category 11), which brings its qualities along
CASES = {
    "jpeg_t2_16x16_noise": ("noise", 2, 16, 16, (95, 50)),
    "jpeg_t3_32x48_noise": ("noise", 3, 32, 48, (95, 100)),
    "jpeg_t2_64x64_dots": ("dots", 2, 64, 64, (95, 30)),
    **jc.GOLDEN,
}


def case_tiles(name):
    """-> tiles [T][H][W][3], qualities"""
    if callable(CASES[name]):
        return CASES[name]()
    content, T, H, W, qualities = CASES[name]
    return np.stack([jr.content(content, H, W, seed=17 + t) for t in range(T)]), qualities


def pil_encode(bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality, subsampling=2, optimize=False)
    return buf.getvalue()


def main():
    for name in CASES:
        tiles, qualities = case_tiles(name)
        out = {"tiles": tiles, "qualities": np.array(qualities, dtype=np.int32)}
        for i, q in enumerate(qualities):
            ours, pil = jr.encode_tiles(tiles, q), pil_encode(np.hstack(list(tiles)), q)
            if ours != pil:
                raise SystemExit(f"{name} quality {q}: the restatement and PIL disagree; nothing written for this case")
            out[f"jpeg_{i}"] = np.frombuffer(ours, dtype=np.uint8)
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **out)
        print(name, [len(out[f"jpeg_{i}"]) for i in range(len(qualities))], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
