"""The work counters of tknnRadiusKnn, tknnKnn, tknnPeriodicKnn and tknnBatchKnn against tests/golden/rknn_counters.json: the same
rows from the same work.  The fixture was recorded (tests/golden/make_rknn_counters.py) on the build BEFORE the four calls came
to share one walk, one seed and one lane kernel template, so a rule that tests another box, merges at another moment or hands
another query to the lane kernel shows here even where the rows stay right.  20 000 points, some thirty calls.
"""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_rknn_counters as gen  # noqa: E402

pytestmark = pytest.mark.gpu

with open(gen.OUT) as _fh:
    GOLDEN = json.load(_fh)
CASES = list(gen.cases())


@pytest.fixture(scope="module")
def engines():
    eng = gen.Engines()
    yield eng
    eng.close()


def test_the_fixture_holds_every_case():
    assert sorted(GOLDEN) == sorted(c[0] for c in CASES)
    for name, call, *_ in CASES:
        must = {"total", "full_rows", "lane_rows"} | (set() if call == "radius_knn" else {"tightened_rows"})  # functions of the rows alone
        assert must <= set(GOLDEN[name]) <= set(gen.COUNTERS), name


@pytest.mark.parametrize("name,call,own,k,radius,forced", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_counters_are_the_recorded_ones(engines, name, call, own, k, radius, forced):
    info = engines.run(call, own, k, radius, forced)
    got = {c: int(info[c]) for c in GOLDEN[name]}
    print(name, got)
    assert got == GOLDEN[name]
