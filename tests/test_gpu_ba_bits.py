"""The joint bundle adjustment and the lens calibration hold their bits across commits: every output of the cases of
tests/ba_bits_cases.py against tests/golden/ba_schur_bits.json, which scripts/record_ba_bits.py wrote on an MI355X from the library of
the commit before the two solvers were given one Schur loop and one set of kernels.  The other tests of the two sections compare with
50-digit values inside a tolerance and check bits from call to call only; a sum taken in another order passes them all."""
import json
import os

import pytest

import ba_bits_cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_schur_bits.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def record(core):
    from mocap_core import capi
    c = capi.MocapCore(core.device_id)      # a context of this module's own: cameras set here stay here
    try:
        return ba_bits_cases.run_cases(c)
    finally:
        c.close()


def test_the_cases_are_the_recorded_ones_and_not_vacuous(record):
    assert sorted(record) == sorted(GOLDEN) and len(record) == 12 + 28 + 6 + 6
    ba_bits_cases.check_not_vacuous(GOLDEN)
    ba_bits_cases.check_not_vacuous(record)


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_bits_are_those_of_the_recorded_library(record, key):
    got, want = record[key], GOLDEN[key]
    print(key, {k: got[k] for k in ba_bits_cases.CLEAR})
    for k in ba_bits_cases.CLEAR:
        assert got[k] == want[k], k
    assert got["digest"] == want["digest"]
