"""Times of the layered lucid synthesis at 480 x 854, batch 3: the layered launch beside `eosvos_lucid_compose` in the same run,
a round-0 batch with and without layers, the fine-tune with `layers` off against another checkout's, and `bench.py` beside it.

  python tools/lucid_layers_time.py [--out profiles/lucid_layers_time.txt] [--rounds 5] [--reps 20] [--parent DIR] [--bench-steps 60]

Timed, on a synthetic frame with a 120 x 160 target and three other objects beside it (example parameters, untuned):
  compose        `Engine.lucid_compose` for 1, 2 and 3 samples, and `Engine.lucid_compose_layers` with 1, 2, 3 and 4 layers for
                 1, 2 and 3 samples: one launch each, no host read (the read costs what it costs in tools/lucid_time.py)
  round-0 batch  `evaluate.lucid_batches` with samples 2 and 3, without layers and with 1 and 3 other objects
Each figure is the median [min .. max] over `rounds` interleaved rounds of `reps` calls ending in a device synchronise: the
protocol of tools/lucid_time.py, whose off-path child this tool runs as well.

--parent DIR: a built checkout of the commit before this feature.  `finetune_object` (`lucid` and `layers` off) is timed in
subprocesses, this tree and DIR in turn (which of the two goes first alternates), `rounds` times each: this tree's median has to lie inside the parent's own
[min .. max].  `bench.py --gpus 1` runs once in each tree as well."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from lucid_time import BATCH, BN, H, W, fmt, off_path, timed  # noqa: E402

from eosvos_amd import lucid, lucid_layers, synthetic  # noqa: E402
from eosvos_amd.evaluate import device_augment, lucid_batches  # noqa: E402
from eosvos_amd.networks import DeepLabV3Plus  # noqa: E402

L = dict(lucid.DEFAULTS)                                 # example values, untuned
FRONT = lucid_layers.DEFAULTS['front']
BOXES = [(180, 300, 350, 510), (60, 170, 100, 260), (250, 420, 560, 700), (330, 460, 120, 300)]    # the target, then the others


def bench(tree, steps, warmup):
    p = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)], cwd=tree,
                       capture_output=True, text=True, timeout=900)
    rows = [l for l in p.stdout.splitlines() if l.startswith('{')]
    if p.returncode != 0 or not rows:
        raise SystemExit(f'bench.py in {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
    return json.loads(rows[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'lucid_layers_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the layered synthesis')
    ap.add_argument('--bench-steps', type=int, default=60)
    ap.add_argument('--bench-warmup', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/lucid_layers_time.py needs a GPU: nothing is measured without one')
    model = DeepLabV3Plus('resnet50', 1, batch_norm=BN, max_batch=BATCH)
    model.load_state_dict(synthetic.synthetic_state('resnet50'))
    eng = model._ensure_engine(H, W, BATCH)
    frame = synthetic.synthetic_frames(1, H, W)[0].cuda()
    masks = torch.zeros(len(BOXES), 1, H, W, device='cuda')
    for i, (y0, y1, x0, x1) in enumerate(BOXES):
        masks[i, :, y0:y1, x0:x1] = 1.0
    fr, gt, others = frame[0].contiguous(), masks[:1].contiguous(), masks[1:].contiguous()
    ids = lucid_layers.layer_map(gt[0], others)
    geo = lucid_layers.geometry(ids, len(BOXES))
    centres = [g[1] for g in geo]
    m = gt[0].contiguous()
    plate1 = eng.lucid_plate(fr, m, L['dilate'])
    plate = eng.lucid_plate(fr, (ids != 0).float().unsqueeze(0), L['dilate'])
    rng = random.Random(1)
    draws = [lucid_layers.draw_sample(rng, L, FRONT, len(BOXES) - 1) for _ in range(BATCH)]
    one = [lucid.sample_matrices(d, H, W, centres[1]) for d in draws]
    steps = []
    for n in (1, 2, 3):
        steps.append((f'eosvos_lucid_compose, {n} sample(s)', lambda n=n: eng.lucid_compose(fr, m, plate1, one[:n], read_counts=False)))
    for n_layers in (1, 2, 3, 4):
        prm = [lucid_layers.sample_layers(dict(d, others=d['others'][:n_layers - 1]), H, W, centres) for d in draws]
        for n in (1, 2, 3):
            steps.append((f'eosvos_lucid_compose_layers, {n_layers} layer(s), {n} sample(s)',
                          lambda n=n, prm=prm: eng.lucid_compose_layers(fr, ids, plate, prm[:n], read_counts=False)))
    plain = device_augment(model)
    for n in (2, 3):
        for n_others in (0, 1, 3):
            lay = {} if not n_others else {'layers': {'others': n_others, 'front': FRONT}, 'lucid_others': others}
            fn = lucid_batches(model, plain, frame, gt, BATCH, dict(L, samples=n), **lay)
            fn(1)                                                       # builds the plate
            steps.append((f'round-0 batch, samples {n}, {n_others} other object(s)', lambda fn=fn: fn(1)))
    times = {name: [] for name, _ in steps}
    random.seed(1)
    for name, fn in steps:                                              # warm-up of every shape
        for _ in range(3):
            fn()
    for _ in range(a.rounds):
        for name, fn in steps:
            times[name].append(timed(fn, a.reps))
    lines = [f'tools/lucid_layers_time.py: batch {BATCH} at {H} x {W}, {a.rounds} interleaved rounds of {a.reps} calls, ms per call: median [min .. max]',
             f'  lucid = {L} with `samples` as named, front = {FRONT} (example values, untuned); a 120 x 160 target and 3 other objects; '
             'no launch below waits for its counts']
    for name, _ in steps:
        lines.append(f'  {name:<58} {fmt(times[name])}')
    record = {'height': H, 'width': W, 'batch': BATCH, 'rounds': a.rounds, 'reps': a.reps, 'lucid': L,
              'ms_per_call': {k: [round(v, 4) for v in t] for k, t in times.items()}}
    model.close_engines()
    if a.parent:
        parent = os.path.abspath(a.parent)
        off = {'this tree': [], 'parent': []}
        for r in range(a.rounds):                                       # the trees in turn, the one that goes first alternating:
            for k in (('this tree', 'parent') if r % 2 == 0 else ('parent', 'this tree')):     # the second child meets a warmer GPU
                off[k].append(off_path(ROOT if k == 'this tree' else parent, a.iters))
            print(f"off path: this tree {off['this tree'][-1]:.3f} ms, parent {off['parent'][-1]:.3f} ms", flush=True)
        lines.append(f'off path, `finetune_object` (lucid and layers off, random_train_transform, {a.iters} round-0 iterations + 1 inferred '
                     'frame), one subprocess per figure, the trees in turn and the first of each pair alternating, ms per iteration:')
        for k, t in off.items():
            lines.append(f'  {k:<58} {fmt(t)}')
        inside = min(off['parent']) <= statistics.median(off['this tree']) <= max(off['parent'])
        lines.append(f'  this tree\'s median inside the parent\'s [min .. max]: {inside}')
        record['off_path_ms_per_iteration'] = {k: [round(v, 4) for v in t] for k, t in off.items()}
        lines.append(f'bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}, one run per tree in this session:')
        record['bench'] = {}
        for k, tree in (('this tree', ROOT), ('parent', parent)):
            res = bench(tree, a.bench_steps, a.bench_warmup)
            record['bench'][k] = {key: res[key] for key in ('metric', 'value', 'unit', 'steps', 'warmup', 'ms_per_step', 'dtype')}
            head = json.dumps(record['bench'][k])
            lines.append(f'  {k:<58} {head}')
            print(lines[-1], flush=True)
    lines.append(json.dumps(record))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
