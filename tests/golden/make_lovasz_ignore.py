"""Fixture `lovasz_ignore.npz`: the UNMODIFIED reference's `lovasz_hinge(..., ignore=255)` (networks/loss_lovasz.py:78-126) on
seeded inputs with void pixels.

    python tests/golden/make_lovasz_ignore.py --ref /path/to/reference/src

Imports the reference module through `_refshim` (as make_golden.py does), evaluates loss and dL/dlogits through its autograd for
both `per_image` settings and stores them beside the inputs, together with the reference's own distance to the fp64
restatement (tests/loss_ignore_ref.py) -- the noise a test against this fixture may allow, as in `lovasz.npz`.  B = 3 at
40 x 64: image 0 carries a void band around the object's boundary plus scattered void pixels, image 1 is entirely void (it
adds 0 to the per-image mean, loss_lovasz.py:101-103), image 2 has no void pixel.  The generator refuses inputs on which the
reference and the restatement disagree by more than rounding.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import loss_ignore_ref  # noqa: E402

B, H, W, IGNORE = 3, 40, 64, 255
LOSS_RTOL, GRAD_RTOL = 1e-5, 1e-3          # a-priori bounds on reference vs restatement (fp32 cumsum / difference noise)


def reference(mod, logits, labels, per_image):
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    loss = mod.lovasz_hinge(x, torch.from_numpy(labels.astype(np.float32)), per_image=per_image, ignore=IGNORE)
    (g,) = torch.autograd.grad(loss, x)
    return np.float32(loss.item()), g.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='the `src` directory of an e-OSVOS checkout')
    ap.add_argument('--out', default=os.path.join(HERE, 'lovasz_ignore.npz'))
    a = ap.parse_args()
    import _refshim
    _refshim.install(a.ref)
    from networks import loss_lovasz as mod
    rng = np.random.RandomState(20255)
    yy, xx = np.mgrid[0:H, 0:W]
    r = [((yy - 20 - 2 * b) ** 2 / (10.0 + 2 * b) ** 2 + (xx - 32 + 4 * b) ** 2 / (16.0 - 2 * b) ** 2) for b in range(B)]
    labels = np.stack([v <= 1.0 for v in r]).astype(np.uint8)
    logits = ((2.0 * labels - 1.0) * 0.8 + 1.5 * rng.randn(B, H, W)).astype(np.float32)
    labels[0][(r[0] > 0.8) & (r[0] < 1.25)] = IGNORE           # a void band on the boundary
    labels[0][rng.rand(H, W) < 0.05] = IGNORE
    labels[1] = IGNORE
    out = {'logits': logits, 'labels': labels, 'ignore': np.float32(IGNORE)}
    for tag, per_image in (('per_image', True), ('flat', False)):
        loss, grad = reference(mod, logits, labels, per_image)
        l64, g64 = loss_ignore_ref.lovasz_hinge(logits, labels, IGNORE, per_image)
        dl = abs(float(loss) - l64)
        dg = float(np.abs(grad - g64).max() / np.abs(g64).max())
        assert dl <= LOSS_RTOL * max(1.0, abs(l64)), (tag, loss, l64)
        assert dg <= GRAD_RTOL, (tag, dg)
        assert not grad[labels == IGNORE].any() and not grad[1].any(), tag
        out[f'{tag}_loss'] = np.float32(loss)
        out[f'{tag}_dlogits'] = grad.astype(np.float32)
        out[f'{tag}_ref_vs_f64_loss'] = np.float64(dl)
        out[f'{tag}_ref_vs_f64_grad'] = np.float64(dg)
        print(f'{tag}: loss {loss:.7f} (fp64 {l64:.9f}, diff {dl:.2e}); grad noise {dg:.2e} of max |grad| {np.abs(g64).max():.3e}')
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
