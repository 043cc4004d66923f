"""Local dense-CRF refinement of the merged label maps: the appearance-aware form of `evaluate.py:322-326` (threshold +
arg-max per pixel, which never looks at the frame) that the OSVOS family uses -- OSVOS' boundary snapping, OnAVOS' dense CRF,
DeepLab v1/v2.  The reference has no such step; this is an opt-in extension (`config.POSTPROCESS`), off by default.

    crf = {'iterations': 5, 'radius': 5, 'dilation': 2, 'w_appearance': 10.0, 'w_smooth': 3.0,
           'theta_alpha': 8.0, 'theta_beta': 0.05, 'theta_gamma': 3.0}              (`DEFAULTS`)

The model is the locally connected dense CRF (mean field with Gaussian position / colour kernels on a dilated (2r+1)^2
window, the "ConvCRF" restriction of Kraehenbuehl-Koltun); include/eosvos.h states it at `eosvos_crf_labels`, the kernels are
csrc/crf_kernels.hip, and `refine_host` below is its torch twin: the reference of the tests (in fp64) and the path of engines
without the entry point.  `None` and `iterations == 0` mean "off": callers then take today's merge, call for call (`active`).

The defaults are the customary pydensecrf ones (appearance weight 10 with sigmas 80 px / 13 of 255, smoothness weight 3 with
sigma 3 px) rescaled to this window and normalisation.  They are NOT tuned on data.
"""
import math
import numbers

import numpy as np
import torch

DEFAULTS = {'iterations': 5, 'radius': 5, 'dilation': 2, 'w_appearance': 10.0, 'w_smooth': 3.0,
            'theta_alpha': 8.0, 'theta_beta': 0.05, 'theta_gamma': 3.0}
_INTS = {'iterations': (0, 20), 'radius': (1, 7), 'dilation': (1, 4)}
MAX_REACH = 16                      # radius * dilation: the halo of the kernel's LDS tile
MAX_OBJECTS = 255
SCRATCH_CAP = 512 << 20             # bytes of engine scratch one `eosvos_crf_labels` call may take
FLOOR = float(np.float32(1e-5))     # the floor of the unary scores, as the fp32 value every path uses


def check(cfg):
    """The complete, validated parameter dictionary of `cfg` (missing keys take `DEFAULTS`); ValueError otherwise."""
    if not isinstance(cfg, dict) or set(cfg) - set(DEFAULTS):
        raise ValueError(f'crf={cfg!r}: a dictionary with keys from {sorted(DEFAULTS)}')
    out = dict(DEFAULTS, **cfg)
    for k, (lo, hi) in _INTS.items():
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= v <= hi:
            raise ValueError(f'crf.{k}={v!r}: an integer in [{lo}, {hi}]')
        out[k] = int(v)
    if out['radius'] * out['dilation'] > MAX_REACH:
        raise ValueError(f"crf: radius * dilation = {out['radius'] * out['dilation']} exceeds {MAX_REACH}")
    for k in ('w_appearance', 'w_smooth', 'theta_alpha', 'theta_beta', 'theta_gamma'):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f'crf.{k}={v!r}: a finite number')
        if (v < 0) if k.startswith('w_') else (v <= 0):
            raise ValueError(f"crf.{k}={v!r}: must be {'>= 0' if k.startswith('w_') else '> 0'}")
        out[k] = float(v)
    return out


def active(cfg):
    """Validated; False when `cfg` asks for the plain merge (None or iterations == 0)."""
    return cfg is not None and check(cfg)['iterations'] != 0


def frames_per_call(n_obj, height, width):
    """How many frames one `eosvos_crf_labels` call may take under the scratch cap (at least 1: a single frame over the cap
    is the library's to reject)."""
    per_frame = 3 * (n_obj + 1) * height * width * 4
    return max(1, min(SCRATCH_CAP // per_frame, 65535))


def _check_tensors(images, probs):
    if images.dim() != 4 or probs.dim() != 4 or images.shape[1] != 3 or images.shape[0] != probs.shape[0] or \
            images.shape[2:] != probs.shape[2:] or images.shape[2] < 1 or images.shape[3] < 1:
        raise ValueError(f'crf: images (N, 3, H, W) and probs (N, n_obj, H, W) expected, got {tuple(images.shape)} and '
                         f'{tuple(probs.shape)}')
    if not 1 <= probs.shape[1] <= MAX_OBJECTS:
        raise ValueError(f'crf: n_obj = {probs.shape[1]} outside [1, {MAX_OBJECTS}]')


def refine_host(images, probs, params=None, dtype=torch.float64):
    """The model of `eosvos_crf_labels` in torch, evaluated in `dtype` where the tensors are: images (N, 3, H, W), probs
    (N, n_obj, H, W) -> (labels (N, H, W) uint8, Q^T (N, n_obj + 1, H, W) in `dtype`).  The parameters enter as the fp32 values
    the C-ABI carries (theta_beta = 0.05 is not an fp32 number), so that every path evaluates one and the same model."""
    p = check(params if params is not None else {})
    _check_tensors(images, probs)
    f32 = lambda v: float(np.float32(v))
    T, r, d = p['iterations'], p['radius'], p['dilation']
    w_a, w_s = f32(p['w_appearance']), f32(p['w_smooth'])
    ia, ib, ig = (1.0 / (2.0 * f32(p[k]) ** 2) for k in ('theta_alpha', 'theta_beta', 'theta_gamma'))
    img, raw = images.to(dtype), probs.to(dtype)
    n, n_obj, H, W = raw.shape
    pc = raw.clamp(0.0, 1.0)
    m = pc.max(dim=1, keepdim=True).values
    s = torch.cat([1.0 - m, pc], dim=1).clamp_min(FLOOR)
    q = s / s.sum(dim=1, keepdim=True)
    if T == 0:                          # `merge_labels`' rule on the probabilities as given
        best, arg = raw[:, 0], torch.zeros_like(raw[:, 0], dtype=torch.int64)
        for o in range(1, n_obj):
            up = raw[:, o] > best
            best, arg = torch.where(up, raw[:, o], best), torch.where(up, torch.full_like(arg, o), arg)
        return torch.where(best < 0.5, torch.zeros_like(arg), arg + 1).to(torch.uint8), q
    unary = -torch.log(q)
    h = r * d
    pad = lambda t: torch.nn.functional.pad(t, (h, h, h, h))
    img_p, inside = pad(img), pad(torch.ones(1, 1, H, W, dtype=dtype, device=img.device))
    win = lambda t, dy, dx: t[:, :, h + dy * d:h + dy * d + H, h + dx * d:h + dx * d + W]
    offsets = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
    # what does not depend on Q: the kernels of every offset and the two position-only normalisers
    k_a, k_s = [], []
    n_a, n_s = torch.zeros(1, 1, H, W, dtype=dtype, device=img.device), torch.zeros(1, 1, H, W, dtype=dtype, device=img.device)
    for dy, dx in offsets:
        d2 = float((dy * d) ** 2 + (dx * d) ** 2)
        pa = torch.exp(torch.tensor(-d2 * ia, dtype=dtype, device=img.device))
        ps = torch.exp(torch.tensor(-d2 * ig, dtype=dtype, device=img.device))
        col = ((img - win(img_p, dy, dx)) ** 2).sum(dim=1, keepdim=True)
        k_a.append(torch.exp(-d2 * ia - col * ib))
        k_s.append(ps)
        n_a = n_a + pa * win(inside, dy, dx)
        n_s = n_s + ps * win(inside, dy, dx)
    zero = torch.zeros((), dtype=dtype, device=img.device)
    for _ in range(T):
        q_p = pad(q)
        acc_a, acc_s = torch.zeros_like(q), torch.zeros_like(q)
        for (dy, dx), ka, ks in zip(offsets, k_a, k_s):
            qn = win(q_p, dy, dx)       # 0 outside the frame
            acc_a = acc_a + ka * qn
            acc_s = acc_s + ks * qn
        msg = w_a * torch.where(n_a > 0, acc_a / n_a, zero) + w_s * torch.where(n_s > 0, acc_s / n_s, zero)
        q = torch.softmax(msg - unary, dim=1)
    best, arg = q[:, 1], torch.ones_like(q[:, 1], dtype=torch.int64)
    for l in range(2, n_obj + 1):
        up = q[:, l] > best
        best, arg = torch.where(up, q[:, l], best), torch.where(up, torch.full_like(arg, l), arg)
    return torch.where(q[:, 0] > best, torch.zeros_like(arg), arg).to(torch.uint8), q


def labels(engine, images, probs, params, return_q=False):
    """Refined label maps of `images` / `probs` on `engine`: its `crf_labels` (the device kernels) where it has the entry
    point, else `refine_host` in fp32 (stand-in engines of host tests)."""
    if hasattr(engine, 'crf_labels'):
        return engine.crf_labels(images, probs, return_q=return_q, **check(params))
    lab, q = refine_host(images, probs, params, dtype=torch.float32)
    return (lab, q) if return_q else lab
