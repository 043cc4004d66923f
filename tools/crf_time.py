"""Time per frame of the local dense-CRF refinement (`eosvos_crf_labels`) at 480 x 854 with the default parameters, and the
measured tolerances of its kernels.

  python tools/crf_time.py [--out profiles/crf_time.txt] [--rounds 5] [--reps 10] [--variant-lib PATH --variant-name TEXT]

Timed, for n_obj 1 and 3, HIP events around `reps` calls on the engine's stream after a warm-up of every shape, `rounds`
interleaved rounds, median [min .. max] of the milliseconds per frame:
  device  `Engine.crf_labels` on 8 frames per call: one prepare launch + 5 iteration launches
  torch   `crf.refine_host` in fp32 on the same device tensors, one frame per call (it keeps (2r+1)^2 - 1 kernel planes per
          frame): what a user without the kernels would run
  T = 0   `Engine.crf_labels(iterations=0)`, i.e. the plain merge, for scale
A/B (--variant-lib): the same device measurement (2 frames per call) in child processes that load the library build under
test through EOSVOS_LIB, alternating with children on the tree's own build, and a hash of the results of both.

Tolerances (the cases of tests/test_gpu_crf.py): largest error of Q^T against `refine_host` in fp64, of `refine_host` in fp32
on the CPU and of the kernels."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from eosvos_amd import crf  # noqa: E402
from eosvos_amd.engine import Engine  # noqa: E402

H, W = 480, 854
FRAMES = 8
CASES = [(37, 53, 3, 2, 1), (48, 64, 2, 3, 2), (40, 70, 1, 5, 2), (33, 65, 5, 1, 3), (7, 9, 2, 5, 2), (2, 2, 1, 2, 2),
         (97, 163, 9, 4, 4)]


def scene(n_obj, n_frames):
    import crf_ref
    images, probs = crf_ref.scene(H, W, n_obj, seed=7 + n_obj, n_frames=n_frames)
    return images.cuda(), probs.cuda()


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


def child(a):
    """One process of the A/B: device time and result hashes with whatever library EOSVOS_LIB names."""
    eng = Engine('resnet50', 96, 160, max_batch=1)
    out = {}
    for n_obj in (1, 3):
        x, p = scene(n_obj, 2)
        fn = lambda: eng.crf_labels(x, p, return_q=True)
        for _ in range(3):
            lab, q = fn()
        out[f'n_obj {n_obj}'] = {'ms': [event_ms(fn, a.reps, 2) for _ in range(a.rounds)],
                                 'sha': hashlib.sha256(lab.cpu().numpy().tobytes() + q.cpu().numpy().tobytes()).hexdigest()[:16]}
    eng.close()
    print('AB ' + json.dumps(out))


def ab(a, lines):
    runs = {'tree': [], 'variant': []}
    for _ in range(2):                                              # alternating processes
        for name in runs:
            env = dict(os.environ)
            env.pop('EOSVOS_LIB', None)
            if name == 'variant':
                env['EOSVOS_LIB'] = os.path.abspath(a.variant_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--rounds', str(a.rounds), '--reps', str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=900)
            got = [l for l in p.stdout.splitlines() if l.startswith('AB ')]
            if p.returncode != 0 or not got:
                raise SystemExit(f'A/B child ({name}) failed: {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}')
            runs[name].append(json.loads(got[-1][3:]))
    lines.append(f'A/B, 2 frames per call, two alternating processes each, ms per frame; variant = {a.variant_name}')
    for key in runs['tree'][0]:
        row = f'  {key}'
        for name in runs:
            t = [v for r in runs[name] for v in r[key]['ms']]
            row += f'   {name} {fmt(t)} results {sorted({r[key]["sha"] for r in runs[name]})}'
        lines.append(row)
    return runs


def tolerances(eng, lines):
    import crf_ref
    out = []
    for h, w, n_obj, r, d in CASES:
        for T in (5, 1):
            images, probs = crf_ref.scene(h, w, n_obj, seed=100 + h + w + n_obj)
            params = dict(crf.DEFAULTS, iterations=T, radius=r, dilation=d)
            lab64, q64 = crf.refine_host(images, probs, params)
            e32 = float((crf.refine_host(images, probs, params, dtype=torch.float32)[1].double() - q64).abs().max())
            lab, q = eng.crf_labels(images.cuda(), probs.cuda(), return_q=True, **params)
            ek = float((q.cpu().double() - q64).abs().max())
            top = q64.topk(2, dim=1).values
            close = (top[:, 0] - top[:, 1]) < 8 * e32
            wrong = int((lab.cpu()[~close] != lab64[~close]).sum())
            out.append({'case': [h, w, n_obj, r, d, T], 'torch_fp32_error': e32, 'kernel_error': ek,
                        'undecided_fraction': float(close.double().mean()), 'labels_off': wrong})
            lines.append(f'  {h:>3} x {w:<3} n_obj {n_obj} r {r} d {d} T {T}   torch fp32 {e32:.3e}   kernel {ek:.3e}   allowed (4 x torch '
                         f'fp32) {4 * e32:.3e}   undecided in fp64 {float(close.double().mean()):.4%}   labels off {wrong}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join('profiles', 'crf_time.txt'))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--variant-lib')
    ap.add_argument('--variant-name', default='(unnamed)')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/crf_time.py needs a GPU: nothing is measured without one')
    if a.child:
        return child(a)
    lines = [f'tools/crf_time.py: eosvos_crf_labels at {H} x {W}, defaults {crf.DEFAULTS}',
             f'{a.rounds} interleaved rounds of {a.reps} calls between HIP events, ms per frame: median [min .. max]']
    runs = ab(a, lines) if a.variant_lib else None                  # before this process opens the GPU
    eng = Engine('resnet50', 96, 160, max_batch=1)
    paths = {}
    for n_obj in (1, 3):
        x, p = scene(n_obj, FRAMES)
        paths[(n_obj, 'device')] = (lambda x=x, p=p: eng.crf_labels(x, p), FRAMES, a.reps)
        paths[(n_obj, 'T = 0')] = (lambda x=x, p=p: eng.crf_labels(x, p, iterations=0), FRAMES, a.reps)
        paths[(n_obj, 'torch')] = (lambda x=x, p=p: crf.refine_host(x[:1], p[:1], crf.DEFAULTS, dtype=torch.float32), 1, 2)
    for fn, _, _ in paths.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, (fn, frames, reps) in paths.items():
            times[k].append(event_ms(fn, reps, frames))
    for n_obj in (1, 3):
        lines.append(f'  n_obj {n_obj}   ' + '   '.join(f'{path} {fmt(times[(n_obj, path)])}' for path in ('device', 'torch', 'T = 0')))
        x, p = scene(n_obj, 1)
        same = torch.equal(eng.crf_labels(x, p), crf.refine_host(x, p, crf.DEFAULTS, dtype=torch.float32)[0])
        lines.append(f'            labels of the two paths on one frame identical: {same}')
    lines.append('tolerances, max abs error of Q^T against refine_host in fp64 (the cases of tests/test_gpu_crf.py):')
    tol = tolerances(eng, lines)
    lines.append(json.dumps({'height': H, 'width': W, 'rounds': a.rounds, 'reps': a.reps,
                             'ms_per_frame': {f'n_obj {n} / {p}': [round(v, 5) for v in t] for (n, p), t in times.items()},
                             'ab': runs, 'variant': a.variant_name if runs else None, 'tolerances': tol}))
    eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
