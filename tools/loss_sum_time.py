"""What a weighted sum of losses costs beside its terms: batch 3 at 480 x 854, one engine, one process, the spellings
interleaved (the layout of tools/boundary_time.py).

Two states of the same network and frames: `random` (the synthetic parent state) and `fitted` (after FIT_ITERS fine-tune
iterations with cross_entropy on the frames).  Per state and spelling:
  loss_us    the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward)
  host_us    the host's time to enqueue one of those evaluations (`Engine.loss`: name resolution, ctypes, the launches); where
             it reaches loss_us the figure is the host's, not the device's
  step_ms    the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync),
             every spelling from the same weights (STEP_KINDS only)
Rounds alternate the spellings; medians are reported, with the spread of the rounds.  `excess` is a sum's loss_us minus the
sum of its terms' own loss_us in the same round: the combine launch (one streaming pass over the terms' gradient slices) plus
what the terms lose by writing to a slice instead of the gradient buffer.  `cross_entropy+dice` stands beside the hard-wired
`cross_entropy_and_dice`, which has its own kernels and bits.

--parent DIR: a built checkout of the commit before this feature.  `bench.py --gpus 1` (the default path: no sum set) is then
run in fresh subprocesses, this tree and DIR in turn, `rounds` times each: the step time of this commit should lie within the
parent's run-to-run range.
    python tools/loss_sum_time.py [--steps 20] [--rounds 5] [--out profiles/loss_sum_time.txt] [--parent DIR]"""
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
JF = 'lovasz_hinge+boundary_f'
SUMS = {JF: ('lovasz_hinge', 'boundary_f'), 'cross_entropy+dice': ('cross_entropy', 'dice')}
KINDS = ('cross_entropy', 'dice', 'lovasz_hinge', 'boundary_f', JF, 'cross_entropy+dice', 'cross_entropy_and_dice')
STEP_KINDS = ('cross_entropy', JF)
DEV = 'cuda:0'


def loss_us(eng, kind, y):
    for _ in range(3):
        eng.loss(kind, y)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(REPS):
        eng.loss(kind, y)
    host = 1e6 * (time.perf_counter() - t0) / REPS           # what the host needs to enqueue one evaluation
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / REPS, host


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


def bench_step_ms(tree, steps):
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '5'], cwd=tree,
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(f'loss_sum_time: bench.py in {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
    res = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{') and '"value"' in l][-1]
    return 1e3 / res['value']                                # finetune_iters/s -> ms per step


def span(v, digits):
    return f'{statistics.median(v):.{digits}f} [{min(v):.{digits}f} .. {max(v):.{digits}f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the loss sums')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loss_sum_time: needs the GPU (there is nothing to time without one)')
    lines, out = [], {'height': H, 'width': W, 'batch': B, 'steps': a.steps, 'rounds': a.rounds, 'reps': REPS, 'states': {}}
    if a.parent:                                             # first, before this process holds the GPU's memory itself
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(bench_step_ms(os.getcwd(), a.bench_steps))
            off['parent'].append(bench_step_ms(os.path.abspath(a.parent), a.bench_steps))
        lines.append(f'bench.py --gpus 1 --steps {a.bench_steps} (no sum set), one subprocess per figure, the trees in turn, ms per '
                     'step, median [min .. max]:')
        for k, v in off.items():
            lines.append(f'  {k:10s} {span(v, 3)}')
            print(lines[-1], flush=True)
        out['bench_step_ms'] = {k: [round(t, 4) for t in v] for k, v in off.items()}
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
        res = {k: {'loss_us': [], 'host_us': [], 'step_ms': []} for k in KINDS}
        excess = {k: [] for k in SUMS}
        for _ in range(a.rounds):
            eng.set_params(params)
            eng.forward(x, want_logits=False)
            for k in KINDS:
                dev, host = loss_us(eng, k, y)
                res[k]['loss_us'].append(dev)
                res[k]['host_us'].append(host)
            for k, terms in SUMS.items():
                excess[k].append(res[k]['loss_us'][-1] - sum(res[t]['loss_us'][-1] for t in terms))
            for k in STEP_KINDS:
                res[k]['step_ms'].append(step_ms(eng, k, x, y, params, a.steps))
        eng.set_params(params)
        eng.set_loss('cross_entropy')
        st = {}
        for k in KINDS:
            st[k] = {'loss_us': [round(t, 1) for t in res[k]['loss_us']], 'host_us': [round(t, 1) for t in res[k]['host_us']],
                     'step_ms': [round(t, 3) for t in res[k]['step_ms']]}
            more = f"   host {statistics.median(res[k]['host_us']):.1f} us"
            more += f"   excess over its terms {span(excess[k], 1)} us" if k in SUMS else ''
            if k in STEP_KINDS:
                more += f"   step {span(res[k]['step_ms'], 3)} ms"
            lines.append(f"{state:7s} {k:26s} loss {span(res[k]['loss_us'], 1)} us{more}")
            print(lines[-1], flush=True)
            if k in SUMS:
                st[k]['excess_us'] = [round(t, 1) for t in excess[k]]
        out['states'][state] = st
    eng.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(f'tools/loss_sum_time.py: batch {B} at {H} x {W}, {a.rounds} interleaved rounds, {a.steps} steps / {REPS} loss '
                    'evaluations each, median [min .. max]; the weights (all 1 here) are untuned and no J&F figure exists\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
