"""Per-frame inference time with test-time augmentation at 480 x 854 (batch 1), and the measured tolerances of the view ->
accumulator kernel.

  python tools/tta_time.py [--out profiles/tta_time.txt] [--rounds 5] [--reps 20]

Timed, for no TTA, flip only and flip x {0.75, 1.0, 1.25}:
  device  `tta.ViewSet.infer`: per view eosvos_resize_frames (other sizes) -> eosvos_infer_view -> eosvos_tta_accumulate
  torch   the same views composed from `Engine.infer` and torch ops: F.interpolate / torch.flip of the frame, Engine.infer,
          torch.flip / F.interpolate of the probabilities, acc += p / n  (it resamples probabilities, not logits: one
          sigmoid-sized pass fewer than an exact restatement, so the comparison does not favour the device path)
Each figure is the median [min .. max] over `rounds` interleaved rounds of `reps` frames ending in a device synchronise.
The weights are synced into the view engines once, outside the timed window, as the evaluation loop does per round.

Tolerances (the cases of tests/test_gpu_tta.py): largest error against sigmoid(F.interpolate(logits.double())) of the same
expression in fp32 by torch on the CPU, and of the kernel."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eosvos_amd import synthetic, tta  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402
from eosvos_amd.networks import DeepLabV3Plus  # noqa: E402

H, W = 480, 854
CONFIGS = [('no TTA', None), ('flip', {'flip': True, 'scales': [1.0]}), ('flip x {0.75, 1.0, 1.25}', {'flip': True, 'scales': [0.75, 1.0, 1.25]})]
BN = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}


def torch_composition(model, view_set, x):
    acc = torch.zeros(x.shape[0], 1, H, W, device=x.device)
    for h, w, mirror, weight in view_set.views:
        eng = model.engine if (h, w) == (H, W) else view_set.engines[(h, w)]
        xs = x if (h, w) == (H, W) else F.interpolate(x, (h, w), mode='bilinear', align_corners=False)
        p = eng.infer(torch.flip(xs, [3]).contiguous() if mirror else xs)
        if mirror:
            p = torch.flip(p, [3])
        if (h, w) != (H, W):
            p = F.interpolate(p, (H, W), mode='bilinear', align_corners=False)
        acc += weight * p
    return acc


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def tolerances(lines):
    pairs = [((96, 160), (96, 160)), ((72, 120), (96, 160)), ((120, 200), (96, 160)), ((73, 122), (97, 163))]
    sd, lrs = synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')
    out = []
    for hw, HW in pairs:
        eng = Engine('resnet50', *hw, max_batch=2)
        eng.load_model_state(sd, lrs)
        x = synthetic.synthetic_frames(2, *hw, seed=21 + hw[0])[0].cuda()
        for mirror in (False, True):
            eng.infer_view(x, mirror=mirror)
            logits = eng.debug_tensor('logits')[:2].cpu()
            u = torch.flip(logits, [3]) if mirror else logits
            ex = lambda t: torch.sigmoid(F.interpolate(t, HW, mode='bilinear', align_corners=False))
            r64 = ex(u.double())
            e32 = float((ex(u).double() - r64).abs().max())
            acc = torch.empty(2, 1, *HW, device='cuda')
            eng.tta_accumulate(acc, 1.0, mirror=mirror, first=True)
            ek = float((acc.cpu().double() - r64).abs().max())
            out.append({'view': hw, 'frame': HW, 'mirror': mirror, 'torch_fp32_error': e32, 'kernel_error': ek})
            lines.append(f'  {hw[0]:>3} x {hw[1]:<3} -> {HW[0]:>3} x {HW[1]:<3} mirror {int(mirror)}   torch fp32 {e32:.3e}   kernel {ek:.3e}   '
                         f'allowed (2 x torch fp32) {2 * e32:.3e}')
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'tta_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/tta_time.py needs a GPU: nothing is measured without one')
    model = DeepLabV3Plus('resnet50', 1, batch_norm=BN, max_batch=1)
    model.load_state_dict(synthetic.synthetic_state('resnet50'))
    model.eval()
    eng = model._ensure_engine(H, W, 1)
    x = synthetic.synthetic_frames(1, H, W)[0].cuda()
    paths = {}
    for name, cfg in CONFIGS:
        if cfg is None:
            paths[(name, 'device')] = lambda: eng.infer(x)
            continue
        vs = tta.ViewSet(model, H, W, cfg)
        vs.sync()
        paths[(name, 'device')] = lambda vs=vs: vs.infer(x)
        paths[(name, 'torch')] = lambda vs=vs: torch_composition(model, vs, x)
    for fn in paths.values():                                       # every shape once before the timed windows
        for _ in range(3):
            fn()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn, a.reps))
    lines = [f'tools/tta_time.py: batch 1 at {H} x {W}, {a.rounds} interleaved rounds of {a.reps} frames, ms per frame: median [min .. max]']
    for name, cfg in CONFIGS:
        row = f'  {name:<26}'
        for path in ('device', 'torch'):
            if (name, path) in times:
                t = times[(name, path)]
                row += f'   {path} {statistics.median(t):7.3f} [{min(t):.3f} .. {max(t):.3f}]'
        if cfg is not None:
            row += f'   views {[(h, w, int(m)) for h, w, m, _ in tta.views(cfg, H, W)]}'
        lines.append(row)
    diff = float((paths[(CONFIGS[2][0], 'device')]() - paths[(CONFIGS[2][0], 'torch')]()).abs().max())
    lines.append(f'  largest difference between the two six-view results (logits resampled vs probabilities resampled): {diff:.3e}')
    lines.append('tolerances of eosvos_tta_accumulate (weight 1, first), max abs error against the fp64 expression:')
    tol = tolerances(lines)
    lines.append(json.dumps({'height': H, 'width': W, 'rounds': a.rounds, 'reps': a.reps,
                             'ms_per_frame': {f'{n} / {p}': [round(v, 4) for v in t] for (n, p), t in times.items()},
                             'tolerances': tol}))
    model.close_engines()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
