"""Per-frame inference time with the object-centred zoom pass at 480 x 854 (batch 1), the four new launches on their own, the
off path against another checkout's `run_frames`, and the measured tolerances of the cut / put-back / blend kernels.

  python tools/zoom_time.py [--out profiles/zoom_time.txt] [--rounds 5] [--reps 20] [--parent DIR]

Timed, on one frame whose first pass is a synthetic blob (so that the box is valid, at zoom 3):
  plain        `Engine.infer`
  zoom         `Engine.infer` + `zoom.Refiner.refine`: eosvos_zoom_boxes -> eosvos_zoom_crop -> eosvos_infer_view ->
               eosvos_zoom_accumulate -> eosvos_zoom_blend
  zoom + flip  `tta.ViewSet.infer` (the flip pair) + the same with a plain and a mirrored zoomed view
  the launches eosvos_zoom_boxes (two launches), eosvos_zoom_crop, eosvos_zoom_accumulate, eosvos_zoom_blend, each alone
Each figure is the median [min .. max] over `rounds` interleaved rounds of `reps` calls ending in a device synchronise.  The
first pass handed to the refiner is a prescribed blob, not the synthetic network's output: the timing does not depend on what
the untrained weights happen to predict.

--parent DIR: a built checkout of the commit before this feature.  `run_frames(model, frames)` (zoom off) is timed in
subprocesses, this tree and DIR in turn, `rounds` times each: the off path should lie within the parent's run-to-run range.

Tolerances (cases of tests/test_gpu_zoom.py): largest error against the fp64 expression of the same expression in fp32 by torch
on the CPU, and of the kernel."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eosvos_amd import synthetic, tta, zoom  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.networks import DeepLabV3Plus  # noqa: E402

H, W = 480, 854
BN = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
Z = dict(zoom.DEFAULTS, max_zoom=3)                     # example values, untuned
FLIP = {'flip': True, 'scales': [1.0]}

OFF_CHILD = r'''
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
from eosvos_amd import synthetic
from eosvos_amd.helper_func import run_frames
from eosvos_amd.networks import DeepLabV3Plus
H, W, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
model = DeepLabV3Plus('resnet50', 1, batch_norm={'accum_stats': False, 'learn_weight': False, 'learn_bias': False}, max_batch=1)
model.load_state_dict(synthetic.synthetic_state('resnet50'))
x = synthetic.synthetic_frames(4, H, W)[0].cuda()
for _ in range(3):
    run_frames(model, x)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    run_frames(model, x)
torch.cuda.synchronize()
print(json.dumps({'ms_per_frame': 1e3 * (time.perf_counter() - t0) / (reps * x.shape[0])}))
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


def off_path(tree, reps):
    p = subprocess.run([sys.executable, '-c', OFF_CHILD, tree, str(H), str(W), str(reps)], cwd=tree, capture_output=True, text=True,
                       timeout=600)
    rows = [l for l in p.stdout.splitlines() if l.startswith('{')]
    if p.returncode != 0 or not rows:
        raise SystemExit(f'off-path run in {tree} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
    return json.loads(rows[-1])['ms_per_frame']


def _err(expr):
    r64 = expr(torch.float64)
    return r64, float((expr(torch.float32).double() - r64).abs().max())


def tolerances(lines):
    hw = (96, 160)
    boxes = [(1, 29, 49, 32, 54), (1, 0, 0, 48, 80)]
    eng = Engine('resnet50', *hw, max_batch=2)
    eng.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
    dev = torch.tensor(boxes, dtype=torch.int32, device='cuda')
    x = synthetic.synthetic_frames(2, *hw, seed=31)[0]
    out = []

    def row(what, e32, ek):
        out.append({'kernel': what, 'torch_fp32_error': e32, 'kernel_error': ek})
        lines.append(f'  {what:<34} torch fp32 {e32:.3e}   kernel {ek:.3e}   allowed (2 x torch fp32) {2 * e32:.3e}')
    r64, e32 = _err(lambda dt: zoom.crop_host(x, boxes, dt))
    row('eosvos_zoom_crop', e32, float((eng.zoom_crop(x.cuda(), dev).cpu().double() - r64).abs().max()))
    inside = torch.zeros(2, 1, *hw, dtype=torch.bool)
    for f, (_, y0, x0, bh, bw) in enumerate(boxes):
        inside[f, :, y0:y0 + bh, x0:x0 + bw] = True
    for mirror in (False, True):
        eng.infer_view(x.cuda(), mirror=mirror)
        logits = eng.debug_tensor('logits')[:2].cpu()
        r64, e32 = _err(lambda dt: zoom.put_back_host([(logits, mirror)], boxes, dt))
        pz = torch.zeros(2, 1, *hw, device='cuda')
        eng.zoom_accumulate(dev, pz, 1.0, mirror=mirror, first=True)
        row(f'eosvos_zoom_accumulate mirror {int(mirror)}', e32, float((pz.cpu().double() - r64)[inside].abs().max()))
    p0 = eng.infer(x.cuda())
    pz = torch.rand(2, 1, *hw, generator=torch.Generator().manual_seed(9)).cuda()
    for feather in (0, 8):
        r64, e32 = _err(lambda dt: zoom.blend_host(p0, pz, boxes, 0.7, feather, dt))
        got = eng.zoom_blend(dev, pz, p0.clone(), 0.7, feather)
        row(f'eosvos_zoom_blend feather {feather}', e32, float((got.cpu().double() - r64).abs().max()))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'zoom_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--parent', default=None, help='a built checkout of the commit before the zoom pass')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/zoom_time.py needs a GPU: nothing is measured without one')
    model = DeepLabV3Plus('resnet50', 1, batch_norm=BN, max_batch=1)
    model.load_state_dict(synthetic.synthetic_state('resnet50'))
    model.eval()
    eng = model._ensure_engine(H, W, 1)
    x = synthetic.synthetic_frames(1, H, W)[0].cuda()
    blob = torch.full((1, 1, H, W), 0.1, device='cuda')
    blob[:, :, 200:260, 400:470] = 0.9                              # a 60 x 70 object: the box is the max_zoom floor, 160 x 285
    box = zoom.boxes_host(blob, Z).tolist()
    plain, flip = zoom.Refiner(model, H, W, Z), zoom.Refiner(model, H, W, Z, FLIP)
    vs = tta.ViewSet(model, H, W, FLIP)
    vs.sync()
    boxes = eng.zoom_boxes(blob, Z)
    view, pz, p0 = torch.empty_like(x), torch.empty_like(blob), blob.clone()

    def zoomed(refiner, first_pass):
        first_pass()
        return refiner.refine(x, p0.copy_(blob))
    paths = {
        'plain': lambda: eng.infer(x),
        'zoom': lambda: zoomed(plain, lambda: eng.infer(x)),
        'flip, no zoom': lambda: vs.infer(x),
        'zoom + flip': lambda: zoomed(flip, lambda: vs.infer(x)),
        'eosvos_zoom_boxes alone': lambda: eng.zoom_boxes(blob, Z),
        'eosvos_zoom_crop alone': lambda: eng.zoom_crop(x, boxes, out=view),
        'eosvos_zoom_accumulate alone': lambda: eng.zoom_accumulate(boxes, pz, 1.0, first=True),
        'eosvos_zoom_blend alone': lambda: eng.zoom_blend(boxes, pz, p0, 0.5, 8),
    }
    for fn in paths.values():                                       # every path once before the timed windows
        for _ in range(3):
            fn()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn, a.reps))
    lines = [f'tools/zoom_time.py: batch 1 at {H} x {W}, {a.rounds} interleaved rounds of {a.reps} calls, ms per call: median [min .. max]',
             f'  zoom = {Z} (example values, untuned); first pass: a prescribed 60 x 70 blob, box {box[0]}']
    for k in paths:
        lines.append(f'  {k:<30} {fmt(times[k])}')
    off = None
    if a.parent:
        off = {'this tree': [], 'parent': []}
        for _ in range(a.rounds):
            off['this tree'].append(off_path(ROOT, a.reps))
            off['parent'].append(off_path(os.path.abspath(a.parent), a.reps))
        lines.append(f'off path, `run_frames(model, frames)` on 4 frames, one subprocess per figure, the trees in turn, ms per frame:')
        for k, t in off.items():
            lines.append(f'  {k:<30} {fmt(t)}')
    lines.append('tolerances (96 x 160, batch 2), max abs error against the fp64 expression:')
    tol = tolerances(lines)
    lines.append(json.dumps({'height': H, 'width': W, 'rounds': a.rounds, 'reps': a.reps, 'zoom': Z, 'box': box[0],
                             'ms_per_call': {k: [round(v, 4) for v in t] for k, t in times.items()},
                             'off_path_ms_per_frame': off and {k: [round(v, 4) for v in t] for k, t in off.items()},
                             'tolerances': tol}))
    model.close_engines()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
