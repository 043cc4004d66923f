"""What the soft boundary-F loss costs beside the other losses: batch 3 at 480 x 854, one engine, one process, the kinds
interleaved (the layout of tools/bootstrap_time.py).

Two states of the same network and frames: `random` (the synthetic parent state) and `fitted` (after FIT_ITERS fine-tune
iterations with cross_entropy on the frames).  Per state and kind:
  loss_us    the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward)
  step_ms    the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync),
             every kind from the same weights (STEP_KINDS only)
Rounds alternate the kinds; medians are reported, with the spread of the rounds.

--parent DIR: a built checkout of the commit before this feature.  The fine-tune step with `cross_entropy` selected is then
timed in fresh subprocesses, this tree and DIR in turn, `rounds` times each (the way of tools/adapt_time.py): the step of this
commit should lie within the parent's run-to-run range.
    python tools/boundary_time.py [--steps 20] [--rounds 5] [--out profiles/boundary_time.txt] [--parent DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, '.')
from eosvos_amd import synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

H, W, B = 480, 854, 3
REPS, FIT_ITERS = 50, 50
KINDS = ('cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy', 'boundary_f_2', 'boundary_f_8', 'boundary_f_16',
         'cross_entropy_and_boundary_f_8')
STEP_KINDS = ('cross_entropy', 'boundary_f_8', 'cross_entropy_and_boundary_f_8')
DEV = 'cuda:0'

CHILD = r'''
import sys, time
sys.path.insert(0, sys.argv[1])
from eosvos_amd import synthetic
from eosvos_amd.engine import Engine
H, W, B, steps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
eng = Engine('resnet50', H, W, max_batch=B, device='cuda:0')
eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
x, y = synthetic.synthetic_frames(B, H, W, seed=5)
x, y = x.cuda(), y.cuda()
eng.set_loss('cross_entropy')
for _ in range(5):
    eng.finetune_step(x, y, sync_loss=False)
eng.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    eng.finetune_step(x, y, sync_loss=False)
eng.synchronize()
print('STEP_MS', 1e3 * (time.perf_counter() - t0) / steps)
eng.close()
'''


def loss_us(eng, kind, y):
    for _ in range(3):
        eng.loss(kind, y)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        eng.loss(kind, y)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / REPS


def step_ms(eng, kind, x, y, params, steps):
    eng.set_params(params)
    eng.set_loss(kind)
    for _ in range(3):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def child_step(tree, steps):
    p = subprocess.run([sys.executable, '-c', CHILD, tree, str(H), str(W), str(B), str(steps)], cwd=tree, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f'boundary_time: the child in {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
    return float([l for l in p.stdout.splitlines() if l.startswith('STEP_MS')][-1].split()[1])


def span(v, digits):
    return f'{statistics.median(v):.{digits}f} [{min(v):.{digits}f} .. {max(v):.{digits}f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the boundary kinds')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('boundary_time: needs the GPU (there is nothing to time without one)')
    lines, out = [], {'height': H, 'width': W, 'batch': B, 'steps': a.steps, 'rounds': a.rounds, 'reps': REPS, 'states': {}}
    if a.parent:                                             # first, before this process holds the GPU's memory itself
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(child_step(os.getcwd(), a.steps))
            off['parent'].append(child_step(os.path.abspath(a.parent), a.steps))
        lines.append('fine-tune step with cross_entropy selected, one subprocess per figure, the trees in turn, ms per step, '
                     'median [min .. max]:')
        for k, v in off.items():
            lines.append(f'  {k:10s} {span(v, 3)}')
            print(lines[-1], flush=True)
        out['cross_entropy_step_ms'] = {k: [round(t, 4) for t in v] for k, v in off.items()}
    eng = Engine('resnet50', H, W, max_batch=B, device=DEV)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    x, y = synthetic.synthetic_frames(B, H, W, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    for state in ('random', 'fitted'):
        if state == 'fitted':
            eng.set_loss('cross_entropy')
            for _ in range(FIT_ITERS):
                eng.finetune_step(x, y, sync_loss=False)
        params = eng.get_params().clone()
        res = {k: {'loss_us': [], 'step_ms': []} for k in KINDS}
        for _ in range(a.rounds):
            eng.set_params(params)
            eng.forward(x, want_logits=False)
            for k in KINDS:
                res[k]['loss_us'].append(loss_us(eng, k, y))
            for k in STEP_KINDS:
                res[k]['step_ms'].append(step_ms(eng, k, x, y, params, a.steps))
        eng.set_params(params)
        eng.set_loss('cross_entropy')
        st = {}
        for k in KINDS:
            st[k] = {'loss_us': [round(t, 1) for t in res[k]['loss_us']], 'step_ms': [round(t, 3) for t in res[k]['step_ms']]}
            step = f"   step {span(res[k]['step_ms'], 3)} ms" if k in STEP_KINDS else ''
            lines.append(f"{state:7s} {k:32s} loss {span(res[k]['loss_us'], 1)} us{step}")
            print(lines[-1], flush=True)
        out['states'][state] = st
    eng.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(f'tools/boundary_time.py: batch {B} at {H} x {W}, {a.rounds} interleaved rounds, {a.steps} steps / {REPS} loss '
                    'evaluations each, median [min .. max]\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
