"""Time per frame of the hole filling (`eosvos_fill_holes`) at 480 x 854.

  python tools/holes_time.py [--out profiles/holes_time.txt] [--rounds 5] [--reps 10]

Scene: that of tools/components_time.py -- per object a disc that drifts 6 pixels per frame, a larger static look-alike disc of
the same label far from it and speckle (2 % of the pixels per object) -- with holes punched into the discs: about 2 % of the disc
pixels drop below the threshold, singly and in 2 x 2 clumps; 8 frames, 1 and 3 objects.
Timed, HIP events around `reps` calls on the engine's stream after a warm-up of every path, `rounds` interleaved rounds, median
[min .. max] of the milliseconds per frame:
  holes    `Engine.fill_holes` on the 8 frames, connectivity 4 and 8, with the previous-frame rule off (prev_overlap 0: one
           launch set for all frames) and on (prev_overlap 0.5: overlap count and apply frame by frame); max_area 64,
           max_rel_area 0.05 (example values, untuned)
  filter   `Engine.filter_components` without the gate (min_rel_area 0.05, largest_only), the stage this one sits beside
  merge    `evaluate.merge_objects` without the stage and with it
and with the wall clock, one call on one frame (frames 0 and 1 with the rule on): `holes.fill_host`, the numpy twin on the host.
Every device result is compared with the twin before it is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eosvos_amd import components, holes  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.evaluate import merge_objects  # noqa: E402

H, W = 480, 854
FRAMES = 8


def scene(n_obj):
    """Per-object probabilities (n_obj, FRAMES, H, W) fp32 whose merge has the blobs, the speckle and the holes described above."""
    rng = np.random.default_rng(11 + n_obj)
    yy, xx = np.mgrid[0:H, 0:W]
    probs = np.zeros((n_obj, FRAMES, H, W), dtype=np.float32)
    for o in range(n_obj):
        cy, cx = 120 + 120 * o, 150
        for f in range(FRAMES):
            disc = (yy - cy) ** 2 + (xx - cx - 6 * f) ** 2 < 40 ** 2
            alike = (yy - cy) ** 2 + (xx - 700) ** 2 < 55 ** 2
            speckle = rng.random((H, W)) < 0.02
            seeds = rng.random((H, W)) < 0.01                        # single pixels, and 2 x 2 clumps around a third of them
            big = seeds & (rng.random((H, W)) < 0.3)
            clump = seeds | np.roll(big, 1, axis=0) | np.roll(big, 1, axis=1) | np.roll(big, (1, 1), axis=(0, 1))
            probs[o, f] = np.where((disc | alike | speckle) & ~((disc | alike) & clump), 0.9 - 0.1 * o, 0.1)
    return torch.from_numpy(probs).cuda()


def event_ms(fn, reps, frames):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / (reps * frames)


def fmt(t):
    return f'{statistics.median(t):8.4f} [{min(t):.4f} .. {max(t):.4f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'holes_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/holes_time.py needs a GPU: nothing is measured without one')
    lines = [f'tools/holes_time.py: eosvos_fill_holes at {H} x {W}, {FRAMES} frames per call; max_area 64, max_rel_area 0.05 and '
             'prev_overlap 0.5 are example values, untuned',
             f'{a.rounds} interleaved rounds of {a.reps} calls between HIP events, ms per frame: median [min .. max]; host twin: wall clock']
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths, host, same = {}, {}, {}
    for n_obj in (1, 3):
        probs = scene(n_obj)
        per_object = [probs[o] for o in range(n_obj)]
        labels = merge_objects(eng, per_object)
        lab_np = labels.cpu().numpy()
        paths[(n_obj, 'merge, no stage')] = lambda p=per_object: merge_objects(eng, p)
        cpar = dict(components.DEFAULTS, min_rel_area=0.05, largest_only=True)
        paths[(n_obj, 'filter c8 gate 0')] = lambda x=labels, p=cpar: eng.filter_components(x, **p)
        for conn in (4, 8):
            for ov in (0.0, 0.5):
                params = dict(holes.DEFAULTS, connectivity=conn, max_area=64, max_rel_area=0.05, prev_overlap=ov)
                key = f'c{conn} overlap {ov}'
                got, filled = eng.fill_holes(labels, return_filled=True, **params)
                t0 = time.perf_counter()
                holes.fill_host(lab_np[:2] if ov else lab_np[:1], params)
                host[(n_obj, key)] = (time.perf_counter() - t0) * 1e3 / (2 if ov else 1)
                full = holes.fill_host(lab_np, params)
                same[(n_obj, key)] = (bool(np.array_equal(got.cpu().numpy(), full)), int(filled.sum()), int((lab_np == 0).sum()))
                paths[(n_obj, 'holes ' + key)] = lambda x=labels, p=params: eng.fill_holes(x, **p)
                if conn == 8:
                    paths[(n_obj, 'merge + holes ' + key)] = lambda q=per_object, p=params: merge_objects(eng, q, holes=p)
    for fn in paths.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(event_ms(fn, a.reps, FRAMES))
    for n_obj in (1, 3):
        lines.append(f'n_obj {n_obj}')
        for (n, path), t in times.items():
            if n == n_obj:
                lines.append(f'  {path:<30} {fmt(t)}')
        for (n, key), ms in host.items():
            if n == n_obj:
                ok, cnt, bg = same[(n, key)]
                lines.append(f'  host twin {key:<20} {ms:8.1f}    device == twin on all {FRAMES} frames: {ok}; {cnt} of {bg} background pixels filled')
    lines.append(json.dumps({'height': H, 'width': W, 'frames': FRAMES, 'rounds': a.rounds, 'reps': a.reps,
                             'ms_per_frame': {f'n_obj {n} / {p}': [round(v, 5) for v in t] for (n, p), t in times.items()},
                             'host_ms_per_frame': {f'n_obj {n} / {k}': round(v, 2) for (n, k), v in host.items()},
                             'device_equals_twin': all(v[0] for v in same.values())}))
    eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
