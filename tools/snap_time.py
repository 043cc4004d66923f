"""Time per frame of the superpixel snapping (`eosvos_snap_labels`) and of the superpixels alone (`eosvos_superpixels`) at
480 x 854.

  python tools/snap_time.py [--out profiles/snap_time.txt] [--rounds 5] [--reps 10]

Scene: per object a coloured disc that drifts 6 pixels per frame on a gradient, +-12 noise on every channel; the per-object
probabilities are the discs shifted by (2, -3) with 3 % speckle, so that the merge has a boundary to move and clusters to
outvote; 8 frames, 1 and 3 objects.
Timed, HIP events around `reps` calls on the engine's stream after a warm-up of every path, `rounds` interleaved rounds, median
[min .. max] of the milliseconds per frame:
  snap         `Engine.snap_labels` on the 8 frames: step 16, 5 iterations, compactness 10, min_share 0.5 (example values,
               untuned); also step 8 and step 32
  superpixels  `Engine.superpixels` alone, the same parameters
  filter       `Engine.filter_components` without the gate (min_rel_area 0.05, largest_only) and
  holes        `Engine.fill_holes` (max_area 64, max_rel_area 0.05), the stages this one sits beside
  merge        `evaluate.merge_objects` without the stage and with it (this includes `snap.quantise`, torch ops)
and with the wall clock, one call on one frame: `snap.snap_host`, the numpy twin on the host.
Every device result is compared with the twin before it is timed (all frames at step 16, the first two at the other steps)."""
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
from eosvos_amd import components, holes, snap  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.evaluate import merge_objects  # noqa: E402

H, W = 480, 854
FRAMES = 8


def scene(n_obj):
    """(frames (FRAMES, 3, H, W) fp32 in [0, 1], per-object probabilities (n_obj, FRAMES, H, W) fp32), both on the device."""
    rng = np.random.default_rng(23 + n_obj)
    yy, xx = np.mgrid[0:H, 0:W]
    colours = [(220, 40, 40), (40, 60, 230), (40, 200, 60)]
    frames = np.zeros((FRAMES, 3, H, W), dtype=np.float32)
    probs = np.zeros((n_obj, FRAMES, H, W), dtype=np.float32)
    for f in range(FRAMES):
        img = np.stack([60 + 60 * xx // (W - 1), 80 + 40 * yy // (H - 1), np.full((H, W), 100)]).astype(np.int64)
        for o in range(n_obj):
            disc = (yy - 100 - 140 * o) ** 2 + (xx - 200 - 6 * f - 150 * o) ** 2 < 60 ** 2
            img[:, disc] = np.array(colours[o])[:, None]
            seen = np.roll(disc, (2, -3), axis=(0, 1)) ^ (rng.random((H, W)) < 0.03)
            probs[o, f] = np.where(seen, 0.9 - 0.1 * o, 0.1)
        frames[f] = np.clip(img + rng.integers(-12, 13, size=img.shape), 0, 255) / 255.0
    return torch.from_numpy(frames).cuda(), torch.from_numpy(probs).cuda()


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
    ap.add_argument('--out', default=os.path.join('profiles', 'snap_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/snap_time.py needs a GPU: nothing is measured without one')
    lines = [f'tools/snap_time.py: eosvos_snap_labels / eosvos_superpixels at {H} x {W}, {FRAMES} frames per call; step 16, 5 iterations, '
             'compactness 10 and min_share 0.5 are example values, untuned',
             f'{a.rounds} interleaved rounds of {a.reps} calls between HIP events, ms per frame: median [min .. max]; host twin: wall clock']
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths, host, same = {}, {}, {}
    for n_obj in (1, 3):
        frames, probs = scene(n_obj)
        per_object = [probs[o] for o in range(n_obj)]
        labels = merge_objects(eng, per_object)
        rgb = snap.quantise(frames)
        rgb_np, lab_np = rgb.cpu().numpy(), labels.cpu().numpy()
        paths[(n_obj, 'merge, no stage')] = lambda p=per_object: merge_objects(eng, p)
        cpar = dict(components.DEFAULTS, min_rel_area=0.05, largest_only=True)
        paths[(n_obj, 'filter c8 gate 0')] = lambda x=labels, p=cpar: eng.filter_components(x, **p)
        hpar = dict(holes.DEFAULTS, max_area=64, max_rel_area=0.05)
        paths[(n_obj, 'holes c8 overlap 0')] = lambda x=labels, p=hpar: eng.fill_holes(x, **p)
        for step in (16, 8, 32):
            params = dict(snap.DEFAULTS, step=step)
            key = f'S{step} T5 m10'
            got, changed = eng.snap_labels(rgb, labels, n_obj=n_obj, return_changed=True, **params)
            ids = eng.superpixels(rgb, step=step)
            if step == 16:
                t0 = time.perf_counter()
                snap.snap_host(rgb_np[:1], lab_np[:1], params, n_obj=n_obj)
                host[(n_obj, key)] = (time.perf_counter() - t0) * 1e3
            k = FRAMES if step == 16 else 2                         # the twin takes about a second per frame
            want_ids = snap.superpixels_host(rgb_np[:k], params)
            want = snap.snap_host(rgb_np[:k], lab_np[:k], params, n_obj=n_obj, ids=want_ids)
            same[(n_obj, key)] = (bool(np.array_equal(got[:k].cpu().numpy(), want) and np.array_equal(ids[:k].cpu().numpy(), want_ids)),
                                  k, int(changed.sum()), int(lab_np.size))
            paths[(n_obj, 'snap ' + key)] = lambda r=rgb, x=labels, n=n_obj, p=params: eng.snap_labels(r, x, n_obj=n, **p)
            paths[(n_obj, 'superpixels ' + key)] = lambda r=rgb, s=step: eng.superpixels(r, step=s)
            if step == 16:
                paths[(n_obj, 'merge + snap ' + key)] = lambda q=per_object, fr=frames, p=params: merge_objects(eng, q, fr, snap=p)
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
        for (n, key), (ok, k, cnt, total) in same.items():
            if n == n_obj:
                ms = f'{host[(n, key)]:8.1f}' if (n, key) in host else '       -'
                lines.append(f'  host twin {key:<20} {ms}    device == twin (ids and maps) on the first {k} frames: {ok}; {cnt} of {total} pixels changed')
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
