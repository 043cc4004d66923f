"""Writes tests/golden/eval_options_calls.json: what the evaluation path hands to `finetune_object_steps`, `finetune_object` and
`merge_objects` over the matrix of `tests/test_eval_options_host.py`.  Run it on the commit whose calls are the reference (the
fixture in the tree was written on the parent of the commit that introduced `eval_options.py`); the test replays the matrix.

    python tools/debug/eval_options_record.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import pytest                                              # noqa: E402

import test_eval_options_host as matrix                     # noqa: E402

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else matrix.GOLDEN
    mp = pytest.MonkeyPatch()
    try:
        rec = matrix.record_all(mp)
    finally:
        mp.undo()
    with open(out, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in rec.items()) + '\n}\n')
    print(out, os.path.getsize(out), 'bytes,', len(rec), 'cases')
