"""Times of the distance gate of online adaptation at 480 x 854 with 2 propagated frames (the OnA batch of 3): the distance
transform, the gated targets beside today's `propagation_targets` and the numpy twin, and `finetune_object` with online
adaptation on and the gate off against another checkout's.

  python tools/adapt_time.py [--out profiles/adapt_time.txt] [--rounds 5] [--reps 20] [--parent DIR]

Timed, on two probability maps with a 120 x 160 blob and a 20 x 20 blob far from it, anchored by the same blob 8 pixels over
(neg_dist 220 / erode 15: OnAVOS's published 480p values, an example, untuned):
  distance_sq      `Engine.distance_sq` at limit 220, seeds = the blobs
  adapt_targets    `Engine.adapt_targets` at neg_dist 220 with erode 0 and 15, with the host read of the counts (what a round
                   pays) and without; `Engine.propagation_targets` (the band alone, what a round pays today) in the same run
  twin             `adapt.targets_host` (numpy), erode 0 and 15, on the same maps, once per round
Each figure is the median [min .. max] over `rounds` interleaved rounds of `reps` calls ending in a device synchronise.

--parent DIR: a built checkout of the commit before this feature.  `finetune_object` (e-OSVOS-OnA: step 5, batch 3,
`random_train_transform`, 7 frames = round 0 and one adaptation round of `iters` iterations each, the gate off) is timed in
subprocesses, this tree and DIR in turn, `rounds` times each: the off path should lie within the parent's run-to-run range."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eosvos_amd import adapt, synthetic  # noqa: E402
from eosvos_amd.networks import DeepLabV3Plus  # noqa: E402

H, W, FRAMES = 480, 854, 2
BN = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
IGNORE = 255.0
LO, HI = 0.3, 0.7
ITERATION_MS = 8.76                                      # README: one fine-tune iteration at batch 3, 480 x 854

OFF_CHILD = r'''
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
from eosvos_amd import config, synthetic, topology
from eosvos_amd.evaluate import finetune_object
from eosvos_amd.helper_func import init_parent_model
from eosvos_amd.meta_optim import MetaOptimizer
H, W, iters = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
cfg = config.parse_cli(['with', 'DAVIS-2017', 'e-OSVOS-OnA', f'num_epochs.eval={iters}', f'eval_online_adapt.num_epochs={iters}'])
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
frames, gt = synthetic.synthetic_frames(1, H, W, seed=3)
frames = torch.cat([torch.roll(frames, shifts=4 * i, dims=3) for i in range(7)]).cuda()
finetune_object(model, mo, msd, frames, gt[0], cfg)
torch.cuda.synchronize()
t0 = time.perf_counter()
probs, hist = finetune_object(model, mo, msd, frames, gt[0], cfg)
torch.cuda.synchronize()
n = sum(len(h) for h in hist)
print(json.dumps({'ms_per_iteration': 1e3 * (time.perf_counter() - t0) / n, 'iterations': n, 'rounds': len(hist)}))
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


def maps():
    """(probs, anchors) (2, 1, H, W): uncertain noise, the object, a look-alike 300 pixels away; the anchor is the object 8 over."""
    rng = np.random.RandomState(1)
    probs = (0.45 * rng.rand(FRAMES, 1, H, W)).astype(np.float32)
    probs[:, :, 180:300, 200:360] = 0.95
    probs[:, :, 100:120, 700:720] = 0.95
    anchors = np.zeros((FRAMES, 1, H, W), dtype=np.float32)
    anchors[:, :, 180:300, 192:352] = 0.95
    return probs, anchors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'adapt_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the distance gate')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/adapt_time.py needs a GPU: nothing is measured without one')
    model = DeepLabV3Plus('resnet50', 1, batch_norm=BN, max_batch=3)
    model.load_state_dict(synthetic.synthetic_state('resnet50'))
    eng = model._ensure_engine(H, W, 3)
    probs, anchors = maps()
    pd, ad = torch.from_numpy(probs).cuda(), torch.from_numpy(anchors).cuda()
    prm = {e: {'neg_dist': 220, 'erode': e} for e in (0, 15)}
    twin = {e: adapt.targets_host(probs, anchors, LO, HI, prm[e], IGNORE) for e in prm}
    for e in prm:                                                   # what is timed computes what the twin computes
        got, n = eng.adapt_targets(pd, ad, LO, HI, prm[e], IGNORE)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), twin[e][0].view(np.uint32)) and n == twin[e][1].tolist(), e
    steps = [('eosvos_distance_sq, limit 220', lambda: eng.distance_sq(pd, HI, limit=220)),
             ('eosvos_propagation_targets (the band alone), counts read', lambda: eng.propagation_targets(pd, LO, HI, IGNORE))]
    for e in prm:
        steps.append((f'eosvos_adapt_targets, neg_dist 220 erode {e}, counts read', lambda e=e: eng.adapt_targets(pd, ad, LO, HI, prm[e], IGNORE)))
        steps.append((f'eosvos_adapt_targets, neg_dist 220 erode {e}, no read',
                      lambda e=e: eng.adapt_targets(pd, ad, LO, HI, prm[e], IGNORE, counts=False)))
    times = {name: [] for name, _ in steps}
    host = {e: [] for e in prm}
    for name, fn in steps:                                          # warm-up of every shape
        for _ in range(3):
            fn()
    for _ in range(a.rounds):
        for name, fn in steps:
            times[name].append(timed(fn, a.reps))
        for e in prm:
            t0 = time.perf_counter()
            adapt.targets_host(probs, anchors, LO, HI, prm[e], IGNORE)
            host[e].append(1e3 * (time.perf_counter() - t0))
    lines = [f'tools/adapt_time.py: {FRAMES} propagated frames at {H} x {W}, {a.rounds} interleaved rounds of {a.reps} calls, ms per call: '
             'median [min .. max]',
             f'  band ({LO}, {HI}); a 120 x 160 blob and a 20 x 20 blob 300 pixels from it; neg_dist 220 / erode 15 are example values, '
             f'untuned; positives kept per frame: {twin[15][1].tolist()}']
    for name, _ in steps:
        lines.append(f'  {name:<62} {fmt(times[name])}')
    for e in prm:
        lines.append(f'  {"adapt.targets_host (numpy twin), erode " + str(e) + ", one call per round":<62} {fmt(host[e])}')
    per_round = statistics.median(times['eosvos_adapt_targets, neg_dist 220 erode 15, counts read'])
    lines.append(f'  per adaptation round: one adapt_targets call = {per_round:.3f} ms beside eval_online_adapt.num_epochs x {ITERATION_MS} ms '
                 f'= {10 * ITERATION_MS:.1f} ms of iterations at the OnA default of 10 ({100 * per_round / (10 * ITERATION_MS):.2f} %)')
    record = {'height': H, 'width': W, 'frames': FRAMES, 'rounds': a.rounds, 'reps': a.reps, 'band': [LO, HI],
              'ms_per_call': {k: [round(v, 4) for v in t] for k, t in times.items()},
              'twin_ms_per_call': {str(e): [round(v, 2) for v in t] for e, t in host.items()}}
    model.close_engines()
    if a.parent:
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(off_path(ROOT, a.iters))
            off['parent'].append(off_path(os.path.abspath(a.parent), a.iters))
        lines.append(f'off path, `finetune_object` (e-OSVOS-OnA, the gate off: round 0 and one adaptation round of {a.iters} iterations, 6 inferred '
                     'frames), one subprocess per figure, the trees in turn, ms per iteration:')
        for k, t in off.items():
            lines.append(f'  {k:<62} {fmt(t)}')
        record['off_path_ms_per_iteration'] = {k: [round(v, 4) for v in t] for k, t in off.items()}
    lines.append(json.dumps(record))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
