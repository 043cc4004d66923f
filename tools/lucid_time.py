"""Times of the lucid first-frame synthesis at 480 x 854, batch 3: the plate, the compose launch, a round-0 batch beside today's
`FirstFrameAugmenter.batch`, and the fine-tune with lucid off against another checkout's.

  python tools/lucid_time.py [--out profiles/lucid_time.txt] [--rounds 5] [--reps 20] [--parent DIR]

Timed, on a synthetic frame with a 120 x 160 object (example parameters, untuned):
  plate          `Engine.lucid_plate`: once per (sequence, object)
  compose        `Engine.lucid_compose` for 1, 2 and 3 samples: one launch, with the host read of the counts and without
  round-0 batch  `FirstFrameAugmenter.batch` (today's, = samples 0), and `evaluate.lucid_batches` with samples 2 and 3 (the first
                 3 - samples from today's path)
Each figure is the median [min .. max] over `rounds` interleaved rounds of `reps` calls ending in a device synchronise.

--parent DIR: a built checkout of the commit before this feature.  `finetune_object` (lucid off, `random_train_transform`, 2
frames, `iters` round-0 iterations and one inferred frame) is timed in subprocesses, this tree and DIR in turn, `rounds` times
each: the off path should lie within the parent's run-to-run range."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eosvos_amd import lucid, synthetic  # noqa: E402
from eosvos_amd.custom_transforms import FirstFrameAugmenter  # noqa: E402
from eosvos_amd.evaluate import device_augment, lucid_batches  # noqa: E402
from eosvos_amd.networks import DeepLabV3Plus  # noqa: E402

H, W, BATCH = 480, 854, 3
BN = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
L = dict(lucid.DEFAULTS)                                 # example values, untuned

OFF_CHILD = r'''
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
from eosvos_amd import config, synthetic, topology
from eosvos_amd.evaluate import finetune_object
from eosvos_amd.helper_func import init_parent_model
from eosvos_amd.meta_optim import MetaOptimizer
H, W, iters = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', f'num_epochs.eval={iters}'])
cfg['train_early_stopping_cfg'] = {'patience': None, 'min_loss_improv': 0.001}
model, _ = init_parent_model(architecture='DeepLabV3Plus', encoder='resnet50', train_encoder=True, decoder_norm_layer='BatchNorm2d',
                             replace_batch_with_group_norms=False,
                             batch_norm={'accum_stats': False, 'learn_weight': False, 'learn_bias': False},
                             roi_pool_output_sizes=None, eval_augment_rpn_proposals_mode=None, box_nms_thresh=None, maskrcnn_loss=None)
sd = synthetic.synthetic_state('resnet50')
msd = {}
for (n, _), lr in zip(topology.trainable('resnet50'), synthetic.synthetic_lrs('resnet50')):
    msd['log_init_lr_' + n.replace('.', '-')] = lr.clone()
for n, _ in topology.trainable('resnet50'):
    msd['model_init_' + n.replace('.', '-')] = sd[n].clone()
model.load_state_dict(sd)
mo = MetaOptimizer(model, init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
                   use_log_init_lr=False, max_lr=None)
frames, gt = synthetic.synthetic_frames(2, H, W, seed=3)
frames = frames.cuda()
finetune_object(model, mo, msd, frames, gt[0], cfg)
torch.cuda.synchronize()
t0 = time.perf_counter()
probs, hist = finetune_object(model, mo, msd, frames, gt[0], cfg)
torch.cuda.synchronize()
print(json.dumps({'ms_per_iteration': 1e3 * (time.perf_counter() - t0) / len(hist[0]), 'iterations': len(hist[0])}))
model.close_engines()
'''


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def fmt(t):
    return f'{statistics.median(t):7.3f} [{min(t):.3f} .. {max(t):.3f}]'


def off_path(tree, iters):
    p = subprocess.run([sys.executable, '-c', OFF_CHILD, tree, str(H), str(W), str(iters)], cwd=tree, capture_output=True, text=True,
                       timeout=300)
    rows = [l for l in p.stdout.splitlines() if l.startswith('{')]
    if p.returncode != 0 or not rows:
        raise SystemExit(f'off-path run in {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
    return json.loads(rows[-1])['ms_per_iteration']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lucid_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the lucid synthesis')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/lucid_time.py needs a GPU: nothing is measured without one')
    model = DeepLabV3Plus('resnet50', 1, batch_norm=BN, max_batch=BATCH)
    model.load_state_dict(synthetic.synthetic_state('resnet50'))
    eng = model._ensure_engine(H, W, BATCH)
    frame = synthetic.synthetic_frames(1, H, W)[0].cuda()
    gt = torch.zeros(1, 1, H, W, device='cuda')
    gt[:, :, 180:300, 350:510] = 1.0                                # a 120 x 160 object
    fr, m = frame[0].contiguous(), gt[0].contiguous()
    n_mask, centre = lucid.mask_geometry(m)
    plate = eng.lucid_plate(fr, m, L['dilate'])
    rng = random.Random(1)
    prm = [lucid.sample_matrices(lucid.draw_sample(rng, L), H, W, centre) for _ in range(BATCH)]
    today = FirstFrameAugmenter(eng)
    plain = device_augment(model)
    steps = [('eosvos_lucid_plate', lambda: eng.lucid_plate(fr, m, L['dilate']))]
    for n in (1, 2, 3):
        steps.append((f'eosvos_lucid_compose, {n} sample(s), counts read', lambda n=n: eng.lucid_compose(fr, m, plate, prm[:n])))
        steps.append((f'eosvos_lucid_compose, {n} sample(s), no read', lambda n=n: eng.lucid_compose(fr, m, plate, prm[:n], read_counts=False)))
    steps.append(('round-0 batch, samples 0 (FirstFrameAugmenter.batch)', lambda: today.batch(fr, m, BATCH)))
    for n in (2, 3):
        fn = lucid_batches(model, plain, frame, gt, BATCH, dict(L, samples=n))
        fn(1)                                                       # builds the plate
        steps.append((f'round-0 batch, samples {n}', lambda fn=fn: fn(1)))
    times = {name: [] for name, _ in steps}
    random.seed(1)
    for name, fn in steps:                                          # warm-up of every shape
        for _ in range(3):
            fn()
    for _ in range(a.rounds):
        for name, fn in steps:
            times[name].append(timed(fn, a.reps))
    lines = [f'tools/lucid_time.py: batch {BATCH} at {H} x {W}, {a.rounds} interleaved rounds of {a.reps} calls, ms per call: median [min .. max]',
             f'  lucid = {L} with `samples` as named (example values, untuned); a 120 x 160 object, {len(lucid.levels(H, W))} pyramid levels']
    for name, _ in steps:
        lines.append(f'  {name:<54} {fmt(times[name])}')
    record = {'height': H, 'width': W, 'batch': BATCH, 'rounds': a.rounds, 'reps': a.reps, 'lucid': L,
              'ms_per_call': {k: [round(v, 4) for v in t] for k, t in times.items()}}
    model.close_engines()
    if a.parent:
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(off_path(ROOT, a.iters))
            off['parent'].append(off_path(os.path.abspath(a.parent), a.iters))
        lines.append(f'off path, `finetune_object` (lucid off, random_train_transform, {a.iters} round-0 iterations + 1 inferred frame), one '
                     'subprocess per figure, the trees in turn, ms per iteration:')
        for k, t in off.items():
            lines.append(f'  {k:<54} {fmt(t)}')
        record['off_path_ms_per_iteration'] = {k: [round(v, 4) for v in t] for k, t in off.items()}
    lines.append(json.dumps(record))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
