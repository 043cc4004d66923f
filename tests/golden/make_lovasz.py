"""Fixture `lovasz.npz`: the UNMODIFIED reference's `lovasz_hinge` (networks/loss_lovasz.py:78-111) on seeded inputs.

    python tests/golden/make_lovasz.py --ref /path/to/reference/src

Loads the reference module by path (it needs torch and numpy only), evaluates loss and dL/dlogits through its autograd and
stores them beside the inputs, together with the reference's own distance to the fp64 stable-sort restatement
(tests/lovasz_ref.py) -- the reference forms its weights as differences of fp32 numbers near 1, and that noise is what a test
against this fixture may allow.  Cases: B = 3 at 48 x 80 with `per_image` True and False, and image 0 with an all-zero label.
The generator refuses inputs on which the reference and the restatement disagree by more than rounding (a tie between a
foreground and a background pixel that `torch.sort` happened to order the other way would be such a case).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lovasz_ref  # noqa: E402

B, H, W = 3, 48, 80
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-3          # a-priori bounds on reference vs restatement (fp32 cumsum / difference noise)


def load_reference(src):
    spec = importlib.util.spec_from_file_location('ref_loss_lovasz', os.path.join(src, 'networks', 'loss_lovasz.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference(mod, logits, labels, per_image):
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    loss = mod.lovasz_hinge(x, torch.from_numpy(labels.astype(np.float32)), per_image=per_image)
    (g,) = torch.autograd.grad(loss, x)
    return np.float32(loss.item()), g.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='the `src` directory of an e-OSVOS checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'lovasz.npz'))
    a = ap.parse_args()
    mod = load_reference(a.ref)
    rng = np.random.RandomState(20240)
    yy, xx = np.mgrid[0:H, 0:W]
    labels = np.stack([((yy - 24 - 3 * b) ** 2 / (12.0 + 2 * b) ** 2 + (xx - 40 + 5 * b) ** 2 / (20.0 - 3 * b) ** 2) <= 1.0
                       for b in range(B)]).astype(np.uint8)
    # a half-fitted state: the logits lean towards the label, about 40 % of the pixels are still inside the margin
    logits = ((2.0 * labels - 1.0) * 0.8 + 1.5 * rng.randn(B, H, W)).astype(np.float32)
    out = {'logits': logits, 'labels': labels}
    cases = [('per_image', logits, labels, True), ('flat', logits, labels, False),
             ('zero', logits[:1], np.zeros_like(labels[:1]), True)]
    for tag, x, t, per_image in cases:
        loss, grad = reference(mod, x, t, per_image)
        l64, g64 = lovasz_ref.lovasz_hinge_f64(x, t, per_image)
        dl = abs(float(loss) - l64)
        dg = float(np.abs(grad - g64).max() / np.abs(g64).max())
        assert dl <= LOSS_RTOL * max(1.0, abs(l64)), (tag, loss, l64)
        assert dg <= GRAD_RTOL, (tag, dg)
        assert np.array_equal(grad != 0, g64 != 0) or dg < 1e-6, tag
        out[f'{tag}_loss'] = np.float32(loss)
        out[f'{tag}_dlogits'] = grad.astype(np.float32)
        out[f'{tag}_ref_vs_f64_loss'] = np.float64(dl)
        out[f'{tag}_ref_vs_f64_grad'] = np.float64(dg)
        print(f'{tag}: loss {loss:.7f} (fp64 {l64:.9f}, diff {dl:.2e}); grad noise {dg:.2e} of max |grad| {np.abs(g64).max():.3e}')
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
