"""What the GPU tests of the device losses share (test_gpu_lovasz, test_gpu_bootstrap, test_gpu_boundary, test_gpu_loss_ignore,
test_gpu_loss_sum): moving arrays to the device, reading the engine's gradient buffer, writing its logits, void patterns
and masked frames.  A plain module like loss_ignore_ref.py; the fixtures stay in their files."""
import ctypes

import numpy as np
import torch

from eosvos_amd import _ffi, synthetic

DEV = 'cuda:0'
IGN = 255.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dlogits_dev(e, n):
    """The first n elements of dL/dlogits of the last evaluation, as a device tensor of its own."""
    return e.debug_tensor('dlogits').reshape(-1)[:n].clone()


def dlogits_of(e, n):
    """... as a numpy array."""
    return e.debug_tensor('dlogits').reshape(-1)[:n].cpu().numpy()


def _debug_pointer(e, name):
    ptr, dims = ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    _ffi.check(e.lib.eosvos_debug_tensor(e.h, name, ctypes.byref(ptr), dims))
    return ptr, dims[0] * dims[1] * dims[2] * dims[3]


def dlogits_raw(e, n):
    """The first n floats of the gradient buffer, also before any forward (debug_tensor reports one image then)."""
    ptr, _ = _debug_pointer(e, b'dlogits')
    out = torch.empty(n, device=DEV)
    e.synchronize()
    rc = ctypes.CDLL('libamdhip64.so').hipMemcpy(ctypes.c_void_p(out.data_ptr()), ptr, ctypes.c_size_t(n * 4), 3)
    assert rc == 0
    return out.cpu().numpy()


def poke_logits(e, logits):
    """Overwrite the engine's logits of the last forward with `logits` (a device tensor of lastB x H x W elements)."""
    ptr, numel = _debug_pointer(e, b'logits')
    assert logits.numel() == numel and logits.is_contiguous()
    e.synchronize()
    torch.cuda.synchronize()
    rc = ctypes.CDLL('libamdhip64.so').hipMemcpy(ptr, ctypes.c_void_p(logits.data_ptr()), ctypes.c_size_t(logits.numel() * 4), 3)
    assert rc == 0


def void_mask(n, pattern, rng):
    v = np.zeros(n, dtype=bool)
    if pattern == 'all':
        v[:] = True
    elif pattern == 'random30':
        v = rng.rand(n) < 0.3
    elif pattern == 'block':                    # one whole 256-element block and the first element of its neighbour
        start = 256 if n > 513 else 0
        v[start:start + 257] = True
    elif pattern == 'last_valid':
        v[:-1] = True
    return v


def masked_frames(seed, hw, void_share):
    """Batch 3 of synthetic frames at `hw` on the device: (images, masks, masks with `void_share` of the pixels void)."""
    x, y = synthetic.synthetic_frames(3, *hw, seed=seed)
    void = torch.from_numpy(np.random.RandomState(seed).rand(*y.shape) < void_share)
    ym = y.clone()
    ym[void] = IGN
    return x.to(DEV), y.to(DEV), ym.to(DEV)
