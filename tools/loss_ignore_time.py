"""What the void label (`ignore`) costs: batch 3 at 480 x 854, one engine, one process, the variants interleaved.

Per loss kind, the loss launches alone (device events around REPS back-to-back evaluations on the logits of one forward):
  plain      eosvos_loss
  ign0       eosvos_loss_ignore on the same masks (no void pixel)
  ign30      eosvos_loss_ignore with 30 % of the pixels void
and the whole fine-tune step (forward + loss + backward + update; host clock around STEPS steps ending in a sync) with BCE:
ignore off, and on with 30 % void, from the same weights.  Rounds alternate the variants; medians and the spread of the rounds.
    python tools/loss_ignore_time.py [steps] [rounds] [out.txt]"""
import json
import sys
import time

import torch

sys.path.insert(0, '.')
from eosvos_amd import synthetic  # noqa: E402
from eosvos_amd.engine import LOSS_KINDS, Engine  # noqa: E402

H, W, B = 480, 854, 3
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
REPS, IGN = 50, 255.0
DEV = 'cuda:0'


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def loss_us(eng, kind, y, ignore):
    for _ in range(3):
        eng.loss(kind, y, ignore)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        eng.loss(kind, y, ignore)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / REPS


def step_ms(eng, x, y, ignore, params):
    eng.set_params(params)
    eng.set_loss('cross_entropy', ignore)
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
        raise SystemExit('loss_ignore_time: needs the GPU (there is nothing to time without one)')
    eng = Engine('resnet50', H, W, max_batch=B, device=DEV)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    x, y = synthetic.synthetic_frames(B, H, W, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    y30 = torch.where(torch.rand(y.shape, generator=torch.Generator().manual_seed(1)).to(DEV) < 0.3, torch.full_like(y, IGN), y)
    params = eng.get_params().clone()
    variants = (('plain', y, None), ('ign0', y, IGN), ('ign30', y30, IGN))
    res = {k: {v[0]: [] for v in variants} for k in LOSS_KINDS}
    steps = {'off': [], 'on30': []}
    for _ in range(ROUNDS):
        eng.set_params(params)
        eng.forward(x, want_logits=False)
        for k in LOSS_KINDS:
            for tag, masks, ign in variants:
                res[k][tag].append(loss_us(eng, k, masks, ign))
        steps['off'].append(step_ms(eng, x, y, None, params))
        steps['on30'].append(step_ms(eng, x, y30, IGN, params))
    eng.set_params(params)
    eng.set_loss('cross_entropy')
    eng.close()
    out = {'height': H, 'width': W, 'batch': B, 'steps': STEPS, 'rounds': ROUNDS, 'reps': REPS, 'loss_us': {}, 'bce_step_ms': {}}
    lines = []
    for k in LOSS_KINDS:
        out['loss_us'][k] = {t: [round(median(v), 1), round(min(v), 1), round(max(v), 1)] for t, v in res[k].items()}
        lines.append(f'{k:30s} ' + '   '.join(f'{t} {m:7.1f} us [{lo:.1f} .. {hi:.1f}]' for t, (m, lo, hi) in out['loss_us'][k].items()))
        print(lines[-1], flush=True)
    for t, v in steps.items():
        out['bce_step_ms'][t] = [round(median(v), 3), round(min(v), 3), round(max(v), 3)]
        lines.append(f'fine-tune step, cross_entropy, ignore {t:5s} {median(v):7.3f} ms [{min(v):.3f} .. {max(v):.3f}]')
        print(lines[-1], flush=True)
    print(json.dumps(out))
    if OUT:
        with open(OUT, 'w') as f:
            f.write(f'tools/loss_ignore_time.py: batch {B} at {H} x {W}, {ROUNDS} interleaved rounds, {STEPS} steps / {REPS} loss evaluations each\n')
            f.write('\n'.join(lines) + '\n' + json.dumps(out) + '\n')


if __name__ == '__main__':
    main()
