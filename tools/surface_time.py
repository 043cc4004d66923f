"""What the distance-weighted surface loss costs: batch 3 at 480 x 854, caps 16 / 64 / the frame-size default / 4095.

The driver runs every GPU step as a subprocess of its own under a time limit of its own and stops at the first one that fails
(a non-zero exit, a signal or the limit): nothing more is started on the GPU after that.
  bench     with --parent DIR (a built checkout of the commit before this feature): `bench.py --gpus 1` (no surface loss set) in
            fresh subprocesses, this tree and DIR in turn, `rounds` times each.  An unchanged cross_entropy step must lie inside
            the parent's own run-to-run range; both ranges are reported.
  measure   one engine, one process, the kinds interleaved round by round, medians with the spread of the rounds:
    transform   one transform for both directions (eosvos_surface_weights, c only: one column pass over two 16-bit planes, one
                row pass choosing the plane by the pixel's own class) beside the two runs it replaces (eosvos_distance_sq twice,
                foreground -> background and background -> foreground; the select that would still have to merge them is not
                counted), on the same targets.  The decision between the two is taken on these figures.
    loss_us     the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward), on
                the `random` state (the synthetic parent state) and the `fitted` one (after FIT_ITERS cross_entropy
                iterations), beside cross_entropy, boundary_f and lovasz_hinge in the same rounds
    step_ms     the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync)
                under surface_<cap> and dice+0.5*surface_<cap>, beside cross_entropy, every kind from the same weights
    python tools/surface_time.py [--steps 20] [--rounds 5] [--out profiles/surface_time.txt] [--parent DIR]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

H, W, B = 480, 854, 3
REPS, FIT_ITERS = 50, 50
CAPS = (16, 64, 0, 4095)                     # 0: the frame-size default
DEV = 'cuda:0'
BENCH_LIMIT, MEASURE_LIMIT = 300, 900        # seconds, per subprocess


def cap_name(cap, default):
    return f'surface_{cap}' if cap else f'surface (default {default})'


def span(v, digits):
    return f'{statistics.median(v):.{digits}f} [{min(v):.{digits}f} .. {max(v):.{digits}f}]'


# ---- the driver ------------------------------------------------------------------------------------------------------------
def run_step(what, cmd, cwd, limit):
    """One GPU step: its own process, its own time limit; anything but a clean exit ends the whole run."""
    try:
        p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=cwd, capture_output=True, text=True)
    except OSError as e:
        raise SystemExit(f'surface_time: {what}: {e}')
    if p.returncode != 0:
        raise SystemExit(f'surface_time: {what} ended with status {p.returncode}; nothing more is run.\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}')
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
        lines.append(f'bench.py --gpus 1 --steps {a.bench_steps} (no surface loss set), one subprocess per figure, the trees in turn, ms '
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
            f.write(f'tools/surface_time.py: batch {B} at {H} x {W}, {a.rounds} interleaved rounds, {a.steps} steps / {REPS} evaluations '
                    'each, median [min .. max]; the cap and the weight 0.5 are untuned and no J&F figure exists\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


# ---- the measure step ------------------------------------------------------------------------------------------------------
def measure(a):
    import torch
    sys.path.insert(0, '.')
    from eosvos_amd import surface, synthetic
    from eosvos_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit('surface_time: needs the GPU (there is nothing to time without one)')
    default = surface.default_cap(H, W)
    names = [cap_name(c, default) for c in CAPS]
    spell = {cap_name(c, default): (f'surface_{c}' if c else 'surface') for c in CAPS}

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
        eng.set_loss_surface(0)
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
    lines, out = [], {'default_cap': default, 'transform_us': {}, 'states': {}}

    # one transform for both directions, or two runs
    ym = y.reshape(B, H, W).contiguous()
    c0 = torch.empty(B, H, W, dtype=torch.int32, device=DEV)
    c1 = torch.empty_like(c0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib, h = eng.lib, eng.h

    def one(cap):
        assert lib.eosvos_surface_weights(h, p(ym), B, H, W, cap, None, p(c0), None) == 0

    def two(cap):
        assert lib.eosvos_distance_sq(h, p(ym), B, H, W, ctypes.c_float(0.5), 0, cap, p(c0)) == 0
        assert lib.eosvos_distance_sq(h, p(ym), B, H, W, ctypes.c_float(0.5), 1, cap, p(c1)) == 0

    tr = {n: {'one': [], 'two': []} for n in names}
    for _ in range(a.rounds):
        for n, c in zip(names, CAPS):
            cap = c or default
            tr[n]['one'].append(timed(lambda: one(cap)))
            tr[n]['two'].append(timed(lambda: two(cap)))
    one(default)
    two(default)
    eng.synchronize()
    merged = torch.where(ym >= 0.5, c1, c0)                  # what the two runs give once merged: the same integers
    assert torch.equal(merged, eng.surface_weights(ym, cap=default)[0])
    lines.append('the transform alone, us per call (targets of the synthetic frames, no void label):')
    for n in names:
        lines.append(f"  {n:28s} one transform {span(tr[n]['one'], 1)}   two runs of eosvos_distance_sq {span(tr[n]['two'], 1)}")
        out['transform_us'][n] = {k: [round(t, 1) for t in v] for k, v in tr[n].items()}

    others = ('cross_entropy', 'boundary_f', 'lovasz_hinge')
    step_kinds = ['cross_entropy'] + [spell[n] for n in names] + ['dice+0.5*' + spell[n] for n in names]
    for state in ('random', 'fitted'):
        if state == 'fitted':
            eng.set_loss('cross_entropy')
            for _ in range(FIT_ITERS):
                eng.finetune_step(x, y, sync_loss=False)
        params = eng.get_params().clone()
        loss = {k: [] for k in others + tuple(names)}
        steps = {k: [] for k in step_kinds}
        for _ in range(a.rounds):
            eng.set_params(params)
            eng.forward(x, want_logits=False)
            for k in others:
                loss[k].append(timed(lambda: eng.loss(k, y)))
            for n in names:
                eng.set_loss_surface(0)
                loss[n].append(timed(lambda: eng.loss(spell[n], y)))
            for k in step_kinds:
                steps[k].append(step_ms(k, params))
        eng.set_params(params)
        eng.set_loss('cross_entropy')
        eng.set_loss_surface(0)
        for k in loss:
            lines.append(f'{state:7s} {k:28s} loss {span(loss[k], 1)} us')
        for k in step_kinds:
            lines.append(f'{state:7s} {k:28s} step {span(steps[k], 3)} ms')
        out['states'][state] = {'loss_us': {k: [round(t, 1) for t in v] for k, v in loss.items()},
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
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the surface loss')
    ap.add_argument('--stage', default='drive', choices=('drive', 'measure'))
    a = ap.parse_args()
    (measure if a.stage == 'measure' else drive)(a)


if __name__ == '__main__':
    main()
