"""What the topology-aware centreline loss `cldice` costs: batch 3 at 480 x 854, depths 3, 5 (the default there) and 16.

The driver runs every GPU step as a subprocess of its own under a time limit of its own and stops at the first one that fails
(a non-zero exit, a signal or the limit): nothing more is started on the GPU after that.
  bench     with --parent DIR (a built checkout of the commit before this feature): `bench.py --gpus 1` (no cldice term set) in
            fresh subprocesses, this tree and DIR in turn, `rounds` times each.  An unchanged cross_entropy step must lie inside
            the parent's own run-to-run range; both ranges are reported.
  measure   one engine, one process, the kinds interleaved round by round, medians with the spread of the rounds:
    loss_us     the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward): the
                3 k + 8 launches of `cldice_<k>` per depth beside cross_entropy, boundary_f and surface in the same rounds.  The
                cost does not depend on the logits (no data-dependent path), so one state of the weights is timed.
    step_ms     the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync)
                under dice+0.5*cldice_<k>, beside cross_entropy, every kind from the same weights
    python tools/cldice_time.py [--steps 20] [--rounds 5] [--out profiles/cldice_time.txt] [--parent DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

H, W, B = 480, 854, 3
REPS = 50
DEPTHS = (3, 5, 16)
DEV = 'cuda:0'
BENCH_LIMIT, MEASURE_LIMIT = 300, 600        # seconds, per subprocess


def span(v, digits):
    return f'{statistics.median(v):.{digits}f} [{min(v):.{digits}f} .. {max(v):.{digits}f}]'


# ---- the driver ------------------------------------------------------------------------------------------------------------
def run_step(what, cmd, cwd, limit):
    """One GPU step: its own process, its own time limit; anything but a clean exit ends the whole run."""
    try:
        p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    except OSError as e:
        raise SystemExit(f'cldice_time: {what}: {e}')
    if p.returncode != 0:
        raise SystemExit(f'cldice_time: {what} ended with status {p.returncode}; nothing more is run.\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}')
    return p.stdout


def bench_step_ms(tree, steps):
    out = run_step(f'bench.py in {tree}', [sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', '5'], tree,
                   BENCH_LIMIT)
    res = [json.loads(l) for l in out.splitlines() if l.startswith('{') and '"value"' in l][-1]
    return 1e3 / res['value']                                # finetune_iters/s -> ms per step


def drive(a):
    lines, out = [], {'height': H, 'width': W, 'batch': B, 'steps': a.steps, 'rounds': a.rounds, 'reps': REPS}
    if a.parent:
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(bench_step_ms(os.getcwd(), a.bench_steps))
            off['parent'].append(bench_step_ms(os.path.abspath(a.parent), a.bench_steps))
        lines.append(f'bench.py --gpus 1 --steps {a.bench_steps} (no cldice term set), one subprocess per figure, the trees in turn, ms '
                     'per step, median [min .. max]:')
        for k, v in off.items():
            lines.append(f'  {k:10s} {span(v, 3)}')
        lo, hi = min(off['parent']), max(off['parent'])
        med = statistics.median(off['this tree'])
        lines.append(f"  this tree's median {med:.3f} is {'inside' if lo <= med <= hi else 'OUTSIDE'} the parent's range [{lo:.3f} .. {hi:.3f}]")
        print('\n'.join(lines), flush=True)
        out['bench_step_ms'] = {k: [round(t, 4) for t in v] for k, v in off.items()}
    text = run_step('the measure step', [sys.executable, os.path.abspath(__file__), '--stage', 'measure', '--steps', str(a.steps),
                                         '--rounds', str(a.rounds)], os.getcwd(), MEASURE_LIMIT)
    print(text, flush=True)
    body = text.splitlines()
    out['measure'] = json.loads(body[-1])
    lines += body[:-1]
    print(json.dumps(out))
    if a.out:
        with open(a.out, 'w') as f:
            f.write(f'tools/cldice_time.py: batch {B} at {H} x {W}, {a.rounds} interleaved rounds, {a.steps} steps / {REPS} evaluations '
                    'each, median [min .. max]; the depth and the weight 0.5 are untuned and no J&F figure exists\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


# ---- the measure step ------------------------------------------------------------------------------------------------------
def measure(a):
    import torch
    sys.path.insert(0, '.')
    from eosvos_amd import synthetic
    from eosvos_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('cldice_time: needs the GPU (there is nothing to time without one)')
    names = [f'cldice_{k}' for k in DEPTHS]

    def timed(call):
        for _ in range(3):
            call()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.synchronize()
        s.record()
        for _ in range(REPS):
            call()
        e.record()
        e.synchronize()
        return 1e3 * s.elapsed_time(e) / REPS

    def step_ms(kind, params):
        eng.set_params(params)
        eng.set_loss(kind)
        for _ in range(3):
            eng.finetune_step(x, y, sync_loss=False)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.finetune_step(x, y, sync_loss=False)
        eng.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps

    eng = Engine('resnet50', H, W, max_batch=B, device=DEV)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    x, y = synthetic.synthetic_frames(B, H, W, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    others = ('cross_entropy', 'dice', 'boundary_f', 'surface')
    step_kinds = ['cross_entropy'] + ['dice+0.5*' + n for n in names]
    params = eng.get_params().clone()
    loss = {k: [] for k in others + tuple(names)}
    steps = {k: [] for k in step_kinds}
    for _ in range(a.rounds):
        eng.set_params(params)
        eng.forward(x, want_logits=False)
        for k in loss:
            loss[k].append(timed(lambda: eng.loss(k, y)))
        for k in step_kinds:
            steps[k].append(step_ms(k, params))
    eng.set_params(params)
    eng.set_loss('cross_entropy')
    eng.set_loss_cldice(0)
    lines = ['launches per evaluation: ' + ', '.join(f'cldice_{k} {3 * k + 8}' for k in DEPTHS) + ' (3 k + 8)']
    lines += [f'{k:32s} loss {span(v, 1)} us' for k, v in loss.items()]
    lines += [f'{k:32s} step {span(v, 3)} ms' for k, v in steps.items()]
    out = {'launches': {f'cldice_{k}': 3 * k + 8 for k in DEPTHS},
           'loss_us': {k: [round(t, 1) for t in v] for k, v in loss.items()},
           'step_ms': {k: [round(t, 3) for t in v] for k, v in steps.items()}}
    eng.close()
    print('\n'.join(lines))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--out', default=None)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the cldice loss')
    ap.add_argument('--stage', default='drive', choices=('drive', 'measure'))
    a = ap.parse_args()
    (measure if a.stage == 'measure' else drive)(a)


if __name__ == '__main__':
    main()
