"""The bits of every device loss, for comparing two builds of the library: one line per case with a hash of the loss and of
dL/dlogits.  Seeded, times nothing.  Per loss kind: plain, ignore without a void pixel, ignore with 30 % void; through
`Engine.loss_of` at n = 4097 and n = 1024 * 256 + 257 (a second trip of the partial grids' loop, ragged tail) and through
`Engine.loss` on a batch-3 forward at 96 x 160.  The kinds that need the frame's shape (`boundary.KINDS`): one 96 x 160 image
through `loss_of`, the batch through `loss`.  Two sums (SUMS) through `loss`, `loss_of` and `loss_grad_of`, each followed by
`last_loss_terms`.  The fused path: `set_loss` + one `finetune_step` per STEP_LOSSES entry, without and with a void label, as
`last_loss` and a hash of the parameters.  Run it once per build (EOSVOS_LIB selects the library) and diff the outputs.

    python tools/loss_bits.py [out.txt]
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eosvos_amd import boundary, synthetic  # noqa: E402
from eosvos_amd.engine import LOSS_KINDS, Engine  # noqa: E402

DEV, IGN = 'cuda:0', 255.0
SMALL, BIG = (96, 160), (296, 296)
SIZES = (4097, 1024 * 256 + 257)
SUMS = ('0.5*lovasz_hinge+boundary_f_4', '2*dice')
STEP_LOSSES = ('cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy_25', SUMS[0])


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def dlogits(e, n):
    return e.debug_tensor('dlogits').reshape(-1)[:n]


def variants(t, rng):
    """(tag, targets, ignore): plain, the void label without a void pixel, 30 % void."""
    t30 = t.copy()
    t30[rng.rand(t.size) < 0.3] = IGN
    return (('plain', t, None), ('ign0', t, IGN), ('ign30', t30, IGN))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('loss_bits: needs the GPU')
    out = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None
    sd, lrs = synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + '\n')

    engines = {}
    for hw in (SMALL, BIG):
        e = Engine('resnet50', *hw, max_batch=3, device=DEV)
        e.load_model_state(sd, lrs)
        x, y = synthetic.synthetic_frames(3, *hw, seed=11)
        e.forward(x.to(DEV), want_logits=False)
        engines[hw] = (e, y)
    big = engines[BIG][0]
    for n in SIZES:
        rng = np.random.RandomState(n)
        x = torch.from_numpy((3.0 * rng.randn(n)).astype(np.float32)).to(DEV)
        t = (rng.rand(n) < 0.3).astype(np.float32)
        for tag, tv, ign in variants(t, rng):
            td = torch.from_numpy(tv).to(DEV)
            for kind in LOSS_KINDS:
                loss = big.loss_of(kind, x, td, ignore=ign)
                emit(f'loss_of n={n:<7d} {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(dlogits(big, n))}')
    small, y = engines[SMALL]
    rng = np.random.RandomState(7)
    n = y.numel()
    one = SMALL[0] * SMALL[1]
    z0 = small.debug_tensor('logits').reshape(-1)[:one].clone()           # one image of the frame's shape for loss_of
    for tag, tv, ign in variants(y.numpy().reshape(-1).copy(), rng):
        masks = torch.from_numpy(tv).view(y.shape).to(DEV)
        m0 = masks.reshape(-1)[:one].contiguous()
        small.set_loss_boundary(0)
        for kind in (*LOSS_KINDS, *boundary.KINDS):
            loss = small.loss(kind, masks, ignore=ign)
            emit(f'loss 3 x 96 x 160    {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(dlogits(small, n))}')
        for kind in boundary.KINDS:
            loss = small.loss_of(kind, z0, m0, ignore=ign)
            emit(f'loss_of 96 x 160     {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(dlogits(small, one))}')
        for kind in SUMS:
            loss = small.loss(kind, masks, ignore=ign)
            emit(f'loss 3 x 96 x 160    {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(dlogits(small, n))} '
                 f'terms {small.last_loss_terms()!r}')
            loss = small.loss_of(kind, z0, m0, ignore=ign)
            emit(f'loss_of 96 x 160     {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(dlogits(small, one))} '
                 f'terms {small.last_loss_terms()!r}')
            loss, grad = small.loss_grad_of(kind, z0, m0, ignore=ign)
            emit(f'loss_grad_of 96x160  {kind:30s} {tag:6s} loss {digest(loss)} dlogits {digest(grad)} '
                 f'terms {small.last_loss_terms()!r}')
        if tag != 'ign0':
            x = synthetic.synthetic_frames(3, *SMALL, seed=11)[0].to(DEV)
            for kind in STEP_LOSSES:
                small.load_model_state(sd, lrs)
                small.set_loss(kind, ignore=ign)
                small.finetune_step(x, masks, sync_loss=False)
                emit(f'step 3 x 96 x 160    {kind:30s} {tag:6s} loss {digest(small.last_loss())} params {digest(small.get_params())}')
            small.set_loss('cross_entropy')
            small.load_model_state(sd, lrs)
            small.forward(x, want_logits=False)
    for e, _ in engines.values():
        e.close()
    if out:
        out.close()


if __name__ == '__main__':
    main()
