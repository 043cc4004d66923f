"""What the bootstrapped cross-entropy costs beside the other losses: batch 3 at 480 x 854, one engine, one process, the kinds
interleaved (the layout of tools/lovasz_time.py).

Two states of the same network and frames: `random` (the synthetic parent state) and `fitted` (after FIT_ITERS fine-tune
iterations with cross_entropy on the frames: almost every pixel is classified correctly, the case the loss is for).  Per
state and kind:
  loss_us    the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward)
  step_ms    the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync),
             every kind from the same weights
Rounds alternate the kinds; medians are reported, with the spread of the rounds.
    python tools/bootstrap_time.py [steps] [rounds] [out.txt]"""
import json
import sys
import time

import torch

sys.path.insert(0, '.')
from eosvos_amd import synthetic  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

H, W, B = 480, 854, 3
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
REPS, FIT_ITERS = 50, 50
KINDS = ('cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy_25', 'bootstrapped_cross_entropy_10')
DEV = 'cuda:0'


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


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


def step_ms(eng, kind, x, y, params):
    eng.set_params(params)
    eng.set_loss(kind)
    for _ in range(3):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bootstrap_time: needs the GPU (there is nothing to time without one)')
    eng = Engine('resnet50', H, W, max_batch=B, device=DEV)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    x, y = synthetic.synthetic_frames(B, H, W, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    out = {'height': H, 'width': W, 'batch': B, 'steps': STEPS, 'rounds': ROUNDS, 'reps': REPS, 'states': {}}
    lines = []
    for state in ('random', 'fitted'):
        if state == 'fitted':
            eng.set_loss('cross_entropy')
            for _ in range(FIT_ITERS):
                eng.finetune_step(x, y, sync_loss=False)
        params = eng.get_params().clone()
        logits = eng.forward(x)
        wrong = float(((logits >= 0) != (y >= 0.5)).float().mean())
        res = {k: {'loss_us': [], 'step_ms': []} for k in KINDS}
        for _ in range(ROUNDS):
            eng.set_params(params)
            eng.forward(x, want_logits=False)
            for k in KINDS:
                res[k]['loss_us'].append(loss_us(eng, k, y))
            for k in KINDS:
                res[k]['step_ms'].append(step_ms(eng, k, x, y, params))
        eng.set_params(params)
        eng.set_loss('cross_entropy')
        st = {'pixels_misclassified': round(wrong, 5)}
        for k in KINDS:
            st[k] = {'loss_us': round(median(res[k]['loss_us']), 1), 'loss_us_range': [round(min(res[k]['loss_us']), 1), round(max(res[k]['loss_us']), 1)],
                     'step_ms': round(median(res[k]['step_ms']), 3), 'step_ms_range': [round(min(res[k]['step_ms']), 3), round(max(res[k]['step_ms']), 3)]}
            lines.append(f"{state:7s} {k:30s} loss {st[k]['loss_us']:8.1f} us [{st[k]['loss_us_range'][0]:.1f} .. {st[k]['loss_us_range'][1]:.1f}]   "
                         f"step {st[k]['step_ms']:7.3f} ms [{st[k]['step_ms_range'][0]:.3f} .. {st[k]['step_ms_range'][1]:.3f}]   "
                         f"loss / step {1e-1 * st[k]['loss_us'] / st[k]['step_ms']:.2f} %")
            print(lines[-1], flush=True)
        lines.append(f'{state:7s} pixels on the wrong side of the threshold: {100 * wrong:.3f} %')
        print(lines[-1], flush=True)
        out['states'][state] = st
    eng.close()
    print(json.dumps(out))
    if OUT:
        with open(OUT, 'w') as f:
            f.write(f'tools/bootstrap_time.py: batch {B} at {H} x {W}, {ROUNDS} interleaved rounds, {STEPS} steps / {REPS} loss evaluations each\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
