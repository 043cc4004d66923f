"""The launch plan the full-length parity fixtures were cleared with (round 6).

The K-split / tile plan of every matrix launch fixes the fp32 summation order.  Round 5 measured that an equally valid other plan
(weight-gradient K splits that fill 80 % of a round instead of 93 %, an A/B switch since removed) moves the fp32-MFMA mode's 240-iteration trajectory (fixture G21) from 3.6e-4 to 1.04e-3 on the logits --
so G20 / G21 / G22 / G23 pin ONE plan per (mode, batch), and a change of the plan rules must re-clear them
(`tests/test_gpu_fulllength.py`) and then refresh `tests/golden/plan_fingerprint.json` with `tools/plan_fingerprint.py --write`.
This test fails when the plan differs from the recorded one (reference loop: `/root/reference/src/util/evaluate.py:207-281`).
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_launch_plan_matches_the_one_the_fixtures_were_cleared_with(golden_dir):
    path = os.path.join(golden_dir, 'plan_fingerprint.json')
    if not os.path.exists(path):
        pytest.skip('tests/golden/plan_fingerprint.json not recorded yet (tools/plan_fingerprint.py --write on the GPU box)')
    want = json.load(open(path))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import plan_fingerprint
    got = plan_fingerprint.fingerprints()
    diff = {k: (want.get(k), got[k]) for k in got if want.get(k) != got[k]}
    assert not diff, ('the launch plan changed -- re-clear tests/test_gpu_fulllength.py under the new plan, then run '
                      'tools/plan_fingerprint.py --write', diff)
