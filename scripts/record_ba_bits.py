"""Record (GPU box) what tests/test_gpu_ba_bits.py compares against: the cases of tests/ba_bits_cases.py through one build of the library.

   python scripts/record_ba_bits.py --lib PATH --out FILE [--arrays]

PATH is a libmocap_core.so with the C ABI of include/mocap_core.h -- for tests/golden/ba_schur_bits.json a build of the commit BEFORE
the change under test, never the branch's own.  --arrays writes every output value (as float.hex) instead of its SHA-256: run it once
per library and diff the two files to see which output moved first.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--arrays", action="store_true")
    a = ap.parse_args()
    os.environ["MOCAP_CORE_LIB"] = os.path.abspath(a.lib)      # read when mocap_core.capi is imported
    import numpy as np
    import torch  # noqa: F401  (the HIP runtime PyTorch ships is loaded first, as in the tests)
    import ba_bits_cases
    from mocap_core import capi
    assert capi.LIB_PATH == os.environ["MOCAP_CORE_LIB"]
    core = capi.MocapCore(0)
    try:
        if a.arrays:
            rec = ba_bits_cases.run_cases(core, digest=lambda v: [float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel()])
        else:
            rec = ba_bits_cases.run_cases(core)
    finally:
        core.close()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases of {a.lib} -> {a.out}")
    if not a.arrays:
        ba_bits_cases.check_not_vacuous(rec)


if __name__ == "__main__":
    main()
