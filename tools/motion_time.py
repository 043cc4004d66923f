"""Time per frame of the block motion (`eosvos_block_motion`), of the warp (`eosvos_warp_labels`) and of `merge_objects` with
the component filter's gate on, with and without `motion`, at 480 x 854.

  python tools/motion_time.py [--out profiles/motion_time.txt] [--rounds 5] [--reps 10] [--parent DIR]

Scene: per object a textured disc that drifts 20 pixels per frame on a gradient, +-12 noise on every channel, the noise of the
background fixed over the frames; the per-object probabilities are the discs with 1 % speckle; 8 frames, 1 and 3 objects.
Timed, HIP events around `reps` calls on the engine's stream after a warm-up of every path, `rounds` interleaved rounds, median
[min .. max] of the milliseconds per frame:
  vectors      `Engine.block_motion` on the 8 frames (7 searches): block 8 / 16, radius 16 / 32, bias 2 (example values,
               untuned)
  warp         `Engine.warp_labels` on the 8 frames
  merge        `evaluate.merge_objects` with `components = {gate: 8}`: without `motion` (one batched filter call) and with it
               (`snap.quantise`, the vectors, then one filter call and one warp per frame)
and with the wall clock, one frame against its predecessor: `motion.vectors_host`, the numpy twin on the host (radius 16).
Every device result is compared with the twin before it is timed: at radius 16 on the first two frames, at radius 32 on their
upper left 128 x 192 pixels (the twin takes (2 R + 1)^2 passes over the frame).
`--parent DIR`: a checkout of the parent commit with its library built.  The `merge` path without `motion` is then also measured
there, in a process of its own before and after this one's rounds, with the same scene and the same code below (`--merge-only`):
the condition is that `motion` off costs nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

H, W = 480, 854
FRAMES = 8
GATE = 8


def scene(n_obj):
    """(frames (FRAMES, 3, H, W) fp32 in [0, 1], per-object probabilities (n_obj, FRAMES, H, W) fp32), both on the device."""
    rng = np.random.default_rng(29 + n_obj)
    yy, xx = np.mgrid[0:H, 0:W]
    back = np.stack([60 + 60 * xx // (W - 1), 80 + 40 * yy // (H - 1), np.full((H, W), 100)]).astype(np.int64) + \
        rng.integers(-12, 13, size=(3, H, W))
    tex = rng.integers(0, 256, size=(3, 3, 121, 121))
    frames = np.zeros((FRAMES, 3, H, W), dtype=np.float32)
    probs = np.zeros((n_obj, FRAMES, H, W), dtype=np.float32)
    for f in range(FRAMES):
        img = back.copy()
        for o in range(n_obj):
            cy, cx = 100 + 140 * o, 150 + 20 * f + 150 * o
            disc = (yy - cy) ** 2 + (xx - cx) ** 2 < 60 ** 2
            patch = np.zeros((3, H, W), dtype=np.int64)
            patch[:, cy - 60:cy + 61, cx - 60:cx + 61] = tex[o]
            img[:, disc] = patch[:, disc]
            probs[o, f] = np.where(disc ^ (rng.random((H, W)) < 0.01), 0.9 - 0.1 * o, 0.1)
        frames[f] = np.clip(img, 0, 255) / 255.0
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


def run_rounds(paths, rounds, reps):
    for fn in paths.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(event_ms(fn, reps, FRAMES))
    return times


def merge_only(root, rounds, reps):
    """The `merge` path without `motion` on the package under `root`: one JSON line {path: [ms per frame per round]}."""
    sys.path.insert(0, root)
    from eosvos_amd import components
    from eosvos_amd.engine import Engine
    from eosvos_amd.evaluate import merge_objects
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths = {}
    for n_obj in (1, 3):
        frames, probs = scene(n_obj)
        per_object = [probs[o] for o in range(n_obj)]
        cpar = dict(components.DEFAULTS, gate=GATE)
        paths[f'n_obj {n_obj} / merge + filter gate {GATE}'] = lambda p=per_object, fr=frames, c=cpar: merge_objects(eng, p, fr, keep=(0,), components=c)
    times = run_rounds(paths, rounds, reps)
    eng.close()
    print(json.dumps(times))


def parent_run(parent, rounds, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--merge-only', '--root', parent, '--rounds', str(rounds),
                          '--reps', str(reps)], check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'motion_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--merge-only', action='store_true')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/motion_time.py needs a GPU: nothing is measured without one')
    if a.merge_only:
        return merge_only(a.root, a.rounds, a.reps)
    before = parent_run(a.parent, a.rounds, a.reps) if a.parent else None
    sys.path.insert(0, a.root)
    from eosvos_amd import components, motion, snap
    from eosvos_amd.engine import Engine
    from eosvos_amd.evaluate import merge_objects
    lines = [f'tools/motion_time.py: eosvos_block_motion / eosvos_warp_labels at {H} x {W}, {FRAMES} frames per call; block, radius and '
             f'bias 2 are example values, untuned; gate {GATE}',
             f'{a.rounds} interleaved rounds of {a.reps} calls between HIP events, ms per frame: median [min .. max]; host twin: wall clock']
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths, host, same = {}, {}, {}
    for n_obj in (1, 3):
        frames, probs = scene(n_obj)
        per_object = [probs[o] for o in range(n_obj)]
        labels = merge_objects(eng, per_object)
        rgb = snap.quantise(frames)
        rgb_np = rgb.cpu().numpy()
        cpar = dict(components.DEFAULTS, gate=GATE)
        paths[(n_obj, f'merge + filter gate {GATE}')] = lambda p=per_object, fr=frames, c=cpar: merge_objects(eng, p, fr, keep=(0,), components=c)
        for block in (8, 16):
            for radius in (16, 32):
                params = dict(motion.DEFAULTS, block=block, radius=radius)
                key = f'B{block} R{radius}'
                mv = eng.block_motion(rgb, **params)
                if n_obj == 1:                                       # the vectors do not depend on the labels: once
                    crop = rgb_np[:2] if radius == 16 else np.ascontiguousarray(rgb_np[:2, :, :128, :192])
                    t0 = time.perf_counter()
                    want = motion.vectors_host(crop, params)
                    if radius == 16:
                        host[key] = (time.perf_counter() - t0) * 1e3
                    got = mv[:2] if radius == 16 else eng.block_motion(torch.from_numpy(crop).cuda(), **params)
                    same[key] = (bool(np.array_equal(got.cpu().numpy(), want)), tuple(crop.shape[2:]),
                                 int((mv.cpu().numpy() != 0).any(axis=-1).sum()), int(mv[..., 0].numel()))
                    paths[(1, 'vectors ' + key)] = lambda r=rgb, p=params: eng.block_motion(r, **p)
                if radius == 16:
                    paths[(n_obj, f'warp B{block}')] = lambda x=labels, v=mv, b=block: eng.warp_labels(x, v, b)
                paths[(n_obj, f'merge + filter gate {GATE} + motion ' + key)] = \
                    lambda p=per_object, fr=frames, c=cpar, m=params: merge_objects(eng, p, fr, keep=(0,), components=c, motion=m)
    times = run_rounds(paths, a.rounds, a.reps)
    eng.close()
    after = parent_run(a.parent, a.rounds, a.reps) if a.parent else None
    for n_obj in (1, 3):
        lines.append(f'n_obj {n_obj}')
        for (n, path), t in times.items():
            if n == n_obj:
                lines.append(f'  {path:<44} {fmt(t)}')
        if a.parent:
            k = f'n_obj {n_obj} / merge + filter gate {GATE}'
            lines.append(f'  {"parent commit, the same path, run before":<44} {fmt(before[k])}')
            lines.append(f'  {"parent commit, the same path, run after":<44} {fmt(after[k])}')
    for key, (ok, shape, moving, total) in same.items():
        ms = f'{host[key]:9.1f} ms per frame' if key in host else '                     -'
        lines.append(f'  host twin {key:<8} {ms}    device == twin on frames 0..1 at {shape[0]} x {shape[1]}: {ok}; '
                     f'{moving} of {total} blocks of the 8 frames move')
    lines.append(json.dumps({'height': H, 'width': W, 'frames': FRAMES, 'rounds': a.rounds, 'reps': a.reps,
                             'ms_per_frame': {f'n_obj {n} / {p}': [round(v, 5) for v in t] for (n, p), t in times.items()},
                             'parent_ms_per_frame': {'before': before, 'after': after},
                             'host_ms_per_frame': {k: round(v, 1) for k, v in host.items()},
                             'device_equals_twin': all(v[0] for v in same.values())}))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
