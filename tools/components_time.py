"""Time per frame of the connected-component clean-up (`eosvos_filter_components`) at 480 x 854.

  python tools/components_time.py [--out profiles/components_time.txt] [--rounds 5] [--reps 10]

Scene: per object a disc that drifts 6 pixels per frame, a larger static look-alike disc of the same label far from it and
speckle (2 % of the pixels per object) -- the maps a merge leaves behind; 8 frames, 1 and 3 objects.
Timed, HIP events around `reps` calls on the engine's stream after a warm-up of every path, `rounds` interleaved rounds, median
[min .. max] of the milliseconds per frame:
  device  `Engine.filter_components` on the 8 frames, connectivity 4 and 8, gate 0 (one labelling + one filter launch pair for
          all frames) and gate 24 (the filter frame by frame), with min_rel_area 0.05 and largest_only (example values, untuned)
  ids     `Engine.label_components` alone
  merge   `evaluate.merge_objects` without the stage -- what the merge costs before this stage existed -- and with it
and with the wall clock, one call on one frame (frames 0 and 1 for the gate): `components.filter_host`, the numpy twin on the host.
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
from eosvos_amd import components  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.evaluate import merge_objects  # noqa: E402

H, W = 480, 854
FRAMES = 8


def scene(n_obj):
    """Per-object probabilities (n_obj, FRAMES, H, W) fp32 whose merge has the blobs and the speckle described above."""
    rng = np.random.default_rng(11 + n_obj)
    yy, xx = np.mgrid[0:H, 0:W]
    probs = np.zeros((n_obj, FRAMES, H, W), dtype=np.float32)
    for o in range(n_obj):
        cy, cx = 120 + 120 * o, 150
        for f in range(FRAMES):
            disc = (yy - cy) ** 2 + (xx - cx - 6 * f) ** 2 < 40 ** 2
            alike = (yy - cy) ** 2 + (xx - 700) ** 2 < 55 ** 2
            speckle = rng.random((H, W)) < 0.02
            probs[o, f] = np.where(disc | alike | speckle, 0.9 - 0.1 * o, 0.1)
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
    ap.add_argument('--out', default=os.path.join('profiles', 'components_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/components_time.py needs a GPU: nothing is measured without one')
    lines = [f'tools/components_time.py: eosvos_filter_components at {H} x {W}, {FRAMES} frames per call; min_rel_area 0.05 and '
             'largest_only are example values, untuned',
             f'{a.rounds} interleaved rounds of {a.reps} calls between HIP events, ms per frame: median [min .. max]; host twin: wall clock']
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths, host, same = {}, {}, {}
    for n_obj in (1, 3):
        probs = scene(n_obj)
        per_object = [probs[o] for o in range(n_obj)]
        labels = merge_objects(eng, per_object)
        lab_np = labels.cpu().numpy()
        paths[(n_obj, 'merge, no stage')] = lambda p=per_object: merge_objects(eng, p)
        paths[(n_obj, 'ids c8')] = lambda x=labels: eng.label_components(x, 8)
        for conn in (4, 8):
            for gate in (0, 24):
                params = dict(components.DEFAULTS, connectivity=conn, gate=gate, min_rel_area=0.05, largest_only=True)
                key = f'c{conn} gate {gate}'
                got, removed = eng.filter_components(labels, return_removed=True, **params)
                t0 = time.perf_counter()
                components.filter_host(lab_np[:2] if gate else lab_np[:1], params)
                host[(n_obj, key)] = (time.perf_counter() - t0) * 1e3 / (2 if gate else 1)
                full = components.filter_host(lab_np, params)
                same[(n_obj, key)] = (bool(np.array_equal(got.cpu().numpy(), full)), int(removed.sum()), int((lab_np != 0).sum()))
                paths[(n_obj, 'device ' + key)] = lambda x=labels, p=params: eng.filter_components(x, **p)
                if (conn, gate) == (8, 24):
                    paths[(n_obj, 'merge + stage ' + key)] = lambda q=per_object, p=params: merge_objects(eng, q, components=p)
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
                lines.append(f'  {path:<28} {fmt(t)}')
        for (n, key), ms in host.items():
            if n == n_obj:
                ok, rem, fg = same[(n, key)]
                lines.append(f'  host twin {key:<18} {ms:8.1f}    device == twin on all {FRAMES} frames: {ok}; {rem} of {fg} object pixels zeroed')
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
