"""Frozen-encoder fine-tuning (`parent_model.train_encoder: False`, `eosvos_set_trainable_from`) against the full step at
480 x 854: ms per fine-tune step at batch 1 and 3 for R50 / R101 DeepLabV3+ and R50 DeepLabV3, encoder trainable and
frozen, and meta-tasks/s with one task per rank (batch 1, 5 inner steps + the meta frame, outer step included).
Interleaved rounds (trainable, frozen, trainable, frozen ...), median of the rounds.
    python tools/frozen_encoder_time.py [steps] [rounds]"""
import json
import sys
import time

import torch

sys.path.insert(0, '.')
from eosvos_amd import synthetic, topology  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.meta_run import MetaTrainer  # noqa: E402

H, W = 480, 854
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEV = 'cuda:0'


def engine(encoder, batch, frozen):
    eng = Engine(encoder, H, W, max_batch=batch, device=DEV)
    if frozen:
        eng.set_trainable_from(topology.trainable_from(encoder, False))
    eng.load_model_state(synthetic.synthetic_state(encoder), synthetic.synthetic_lrs(encoder))
    return eng


def step_ms(eng, batch):
    x, y = synthetic.synthetic_frames(batch, H, W, seed=5)
    x, y = x.to(DEV), y.to(DEV)
    for _ in range(3):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        eng.finetune_step(x, y, sync_loss=False)
    eng.synchronize()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def tasks_per_s(eng, encoder, iters=6):
    mt = MetaTrainer(eng, meta_batch_size=1)
    tr = topology.trainable(encoder)[eng.train_from:]
    lrs = synthetic.synthetic_lrs(encoder)[len(topology.trainable(encoder)) - len(tr):]
    mt.load_state(synthetic.synthetic_state(encoder), lrs)
    x, y = synthetic.synthetic_frames(1, H, W, seed=6)
    task = (x.to(DEV), y.to(DEV), torch.flip(x, dims=[3]).contiguous().to(DEV), torch.flip(y, dims=[3]).contiguous().to(DEV))
    mt.meta_iteration([task])
    mt.meta_iteration([task])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        mt.meta_iteration([task])
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t0)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


out = {'height': H, 'width': W, 'steps': STEPS, 'rounds': ROUNDS, 'ms_per_step': {}, 'meta_tasks_per_s': {}}
for encoder in ('resnet50', 'resnet101', 'deeplabv3_resnet50'):
    for batch in (1, 3):
        ms = {False: [], True: []}
        engs = {f: engine(encoder, batch, f) for f in (False, True)}
        for _ in range(ROUNDS):
            for f in (False, True):
                ms[f].append(step_ms(engs[f], batch))
        for e in engs.values():
            e.close()
        full, frozen = median(ms[False]), median(ms[True])
        out['ms_per_step'][f'{encoder}_b{batch}'] = {'trainable': round(full, 3), 'frozen': round(frozen, 3),
                                                     'saving': round(1.0 - frozen / full, 3)}
        print(encoder, batch, out['ms_per_step'][f'{encoder}_b{batch}'], flush=True)
    if encoder == 'resnet50':
        tps = {}
        for f in (False, True):
            e = engine(encoder, 1, f)
            tps['frozen' if f else 'trainable'] = round(tasks_per_s(e, encoder), 2)
            e.close()
        out['meta_tasks_per_s'][encoder] = tps
        print(encoder, 'meta tasks/s', tps, flush=True)
print(json.dumps(out))
