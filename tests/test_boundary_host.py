"""Host-side checks of the soft boundary-F loss (no GPU): the spelled names and the keyword rules, the ids at every layer,
and the torch twin (`eosvos_amd.boundary.loss_host`): its autograd gradient against the closed form of include/eosvos.h /
DESIGN 2.5, written here as plain loops over pixels and windows, the exact cases, and the tie rule."""
import os
import re

import numpy as np
import pytest
import torch

from eosvos_amd import boundary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = 255.0
N, C = 'boundary_f', 'cross_entropy_and_boundary_f'
EPS = 1e-7


# ---- names ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,want', [(N, (N, None)), (N + '_1', (N, 1)), (N + '_8', (N, 8)), (N + '_16', (N, 16)),
                                       (C, (C, None)), (C + '_2', (C, 2)), (C + '_16', (C, 16)),
                                       ('dice', ('dice', None)), ('cross_entropy_and_dice', ('cross_entropy_and_dice', None)),
                                       ('boundary', ('boundary', None)), ('lovasz', ('lovasz', None))])
def test_parse_accepts(name, want):
    assert boundary.parse(name) == want


@pytest.mark.parametrize('name', [N + '_0', N + '_17', N + '_08', N + '_2.5', N + '_', N + '8', N + '_-5', N + '_1e1',
                                  C + '_0', C + '_17', C + '_03', C + 'x', N + '_8_8'])
def test_parse_rejects_under_the_prefix(name):
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError):
        boundary.parse(name)
    with pytest.raises(NotImplementedError):
        resolve_loss(name)
    with pytest.raises(NotImplementedError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_the_kinds_are_declared_at_every_layer():
    from eosvos_amd import _ffi
    from eosvos_amd.engine import LOSS_KINDS, resolve_loss, resolve_radius
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_BOUNDARY_F\s+8\b', header)
    assert re.search(r'#define\s+EOSVOS_LOSS_BCE_AND_BOUNDARY_F\s+9\b', header)
    assert not re.search(r'#define\s+EOSVOS_LOSS_\w+\s+7\b', header)          # kind 7 stays unassigned
    assert re.search(r'int\s+eosvos_set_loss_boundary\(eosvos_engine\*\s*e,\s*int\s+radius\)', header)
    assert 'eosvos_set_loss_boundary' in _ffi._SIGNATURES and 'eosvos_boundary_f' in _ffi._SIGNATURES
    assert boundary.KINDS == {N: 8, C: 9}
    assert LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                          'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, 'bootstrapped_cross_entropy': 6}      # has not grown
    assert resolve_loss(N) == (8, None) and resolve_loss(N + '_8') == (8, None) and resolve_loss(C + '_16', radius=16) == (9, None)
    assert resolve_radius(N) is None and resolve_radius(N + '_8') == 8 and resolve_radius(C, 3) == 3
    assert resolve_radius(C + '_3', 3) == 3 and resolve_radius('dice') is None
    assert resolve_loss('dice') == (1, None) and resolve_loss('bootstrapped_cross_entropy_10')[0] == 6
    engine_cpp = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'engine.cpp')).read()
    assert 'EOSVOS_LOSS_BOUNDARY_F' in engine_cpp and 'launch_boundary_f' in engine_cpp


def test_the_keyword_rules():
    from eosvos_amd.engine import resolve_loss, resolve_radius
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(ValueError):                         # suffix and keyword disagree
        resolve_radius(N + '_8', 4)
    with pytest.raises(ValueError):
        compute_loss(C + '_2', z, z, {'radius': 3})
    for bad in (0, 17, -1, 2.5, float('nan'), True):        # out of 1 .. 16, or not whole
        with pytest.raises(ValueError):
            resolve_loss(N, radius=bad)
        with pytest.raises(ValueError):
            compute_loss(N, z, z, {'radius': bad})
    for other in ('dice', 'cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy'):      # the keyword belongs to these kinds alone
        with pytest.raises(ValueError):
            resolve_loss(other, radius=8)
        with pytest.raises(ValueError):
            compute_loss(other, z, z, {'radius': 8})
    with pytest.raises(ValueError):                         # ... and the bootstrap keyword not to them
        resolve_loss(N, fraction=0.25)
    for name in ('lovasz', 'bootstrapped', 'boundary'):     # still unknown
        with pytest.raises(KeyError):
            resolve_loss(name)
        with pytest.raises(NotImplementedError):
            compute_loss(name, z, z)
    for name, kw in ((N, None), (N + '_8', {'radius': 8}), (C, {'radius': 2}), (C + '_16', None)):
        with pytest.raises(RuntimeError):                   # known spellings, but logits that no engine produced
            compute_loss(name, z, z, kw)


def test_radius_helpers():
    from eosvos_amd import data
    assert boundary.default_radius(480, 854) == 8 == min(16, data.davis_bound_pix(0.008, 480, 854))
    assert boundary.default_radius(720, 1280) == 12 and boundary.default_radius(1080, 1920) == 16
    assert boundary.default_radius(96, 160) == data.davis_bound_pix(0.008, 96, 160) == 2
    assert boundary.default_radius(1, 1) == 1
    assert [boundary.check_radius(r) for r in (1, 8, 16, 4.0)] == [1, 8, 16, 4]
    for bad in (0, 17, -3, 1.5, 'x', None, float('inf')):
        with pytest.raises((ValueError, OverflowError)):
            boundary.check_radius(bad)


# ---- the closed form, as plain loops ---------------------------------------------------------------------------------------
def closed_form(z, y, r, ign=None):
    """(loss, dL/dz) of (B, H, W) float64 arrays by the definition: loops over pixels and windows, first maximum in row-major
    order."""
    B, H, W = z.shape
    grad = np.zeros_like(z)
    total = 0.0
    for b in range(B):
        valid = np.ones((H, W), bool) if ign is None else y[b] != ign
        if not valid.any():
            continue
        e = np.exp(-np.abs(z[b]))
        q = np.where(z[b] >= 0, e / (1 + e), 1 / (1 + e))
        sig = np.where(z[b] >= 0, 1 / (1 + e), e / (1 + e))
        h = 1 - y[b]

        def window_max(a, i, j, rad):
            best, arg = -np.inf, None
            for yy in range(max(0, i - rad), min(H, i + rad + 1)):
                for xx in range(max(0, j - rad), min(W, j + rad + 1)):
                    if valid[yy, xx] and a[yy, xx] > best:
                        best, arg = a[yy, xx], (yy, xx)
            return best, arg

        pb, gb, pe, ge = (np.zeros((H, W)) for _ in range(4))
        a1, ar = {}, {}
        for i in range(H):
            for j in range(W):
                if valid[i, j]:
                    m, a1[i, j] = window_max(q, i, j, 1)
                    pb[i, j] = m - q[i, j]
                    gb[i, j] = window_max(h, i, j, 1)[0] - h[i, j]
        for i in range(H):
            for j in range(W):
                if valid[i, j]:
                    pe[i, j], ar[i, j] = window_max(pb, i, j, r)
                    ge[i, j] = window_max(gb, i, j, r)[0]
        Sp, Sg = pb[valid].sum() + EPS, gb[valid].sum() + EPS
        P, R = (pb * ge)[valid].sum() / Sp, (pe * gb)[valid].sum() / Sg
        total += 1 - 2 * P * R / (P + R + EPS)
        dP, dR = 2 * R * (R + EPS) / (P + R + EPS) ** 2, 2 * P * (P + EPS) / (P + R + EPS) ** 2
        routed = np.zeros((H, W))
        for (i, j), k in ar.items():
            routed[k] += gb[i, j]
        Gpb = np.where(valid, -(dP * (ge - P) / Sp + dR / Sg * routed), 0.0)
        Gq = -Gpb.copy()
        for (i, j), k in a1.items():
            Gq[k] += Gpb[i, j]
        grad[b] = np.where(valid, -sig * q * Gq / B, 0.0)
    return total / B, grad


def generic(B, H, W, seed, void=False):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    y = ((((yy - (H - 1) / 2) / max(H / 3.0, 1)) ** 2 + ((xx - (W - 1) / 2) / max(W / 3.0, 1)) ** 2) <= 1).double()
    y = y[None].repeat(B, 1, 1)
    z = 2 * torch.randn(B, H, W, generator=g, dtype=torch.float64) + 4 * (2 * y - 1) * torch.rand(B, H, W, generator=g, dtype=torch.float64)
    z = z.float().double()                                   # the twin takes fp32 logits
    if void:
        y.view(-1)[::7] = IGN
        y[:, H // 3:H // 3 + 2, W // 2 - 1:W // 2 + 2] = IGN
    return z, y


@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('B,H,W,r', [(1, 1, 1, 1), (1, 5, 7, 1), (2, 9, 13, 2), (1, 6, 11, 16), (3, 12, 10, 3)])
def test_autograd_of_the_twin_equals_the_closed_form(B, H, W, r, void):
    z, y = generic(B, H, W, seed=H * W + r, void=void)
    ign = IGN if void else None
    loss, grad, per = boundary.loss_host(z, y, r, ignore=ign)
    ref_loss, ref_grad = closed_form(z.numpy(), y.numpy(), r, ign)
    assert loss.dtype == torch.float64 and grad.shape == z.shape and per.shape == (B,)
    assert abs(float(loss) - ref_loss) <= 1e-14
    assert np.abs(grad.numpy() - ref_grad).max() <= 1e-15
    if void:
        assert not grad[y == IGN].any()
    if H * W > 1:
        assert float(grad.abs().max()) > 0


def test_fp32_and_fp64_come_from_one_source_and_the_combined_kind_adds_the_bce_mean():
    z, y = generic(2, 9, 13, seed=5, void=True)
    l64, g64, _ = boundary.loss_host(z, y, 2, ignore=IGN)
    l32, g32, p32 = boundary.loss_host(z, y, 2, ignore=IGN, dtype=torch.float32)
    assert l32.dtype == g32.dtype == p32.dtype == torch.float32
    assert abs(float(l32) - float(l64)) <= 1e-5 and float((g32.double() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    lc, gc, per = boundary.loss_host(z, y, 2, ignore=IGN, combined=True)
    valid = y != IGN
    zz, yv = z[valid], y[valid]
    bce = torch.clamp(zz, min=0) - zz * yv + torch.log1p(torch.exp(-zz.abs()))
    assert abs(float(lc) - float(l64) - float(bce.mean())) <= 1e-14 and torch.equal(per.mean(), l64)
    gb = torch.zeros_like(z)
    gb[valid] = (torch.sigmoid(zz) - yv) / int(valid.sum())
    assert float((gc - g64 - gb).abs().max()) <= 1e-15 and not gc[~valid].any()


# ---- the exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('case', ['empty_target', 'full_target', 'constant_logits'])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_degenerate_inputs_give_exactly_one_and_zero_gradient(case, void, dtype):
    z, y = generic(2, 9, 13, seed=3)
    if case == 'empty_target':
        y = torch.zeros_like(y)
    elif case == 'full_target':
        y = torch.ones_like(y)
    else:
        z = torch.full_like(z, 0.75)
    if void:
        y.view(-1)[::7] = IGN
    loss, grad, per = boundary.loss_host(z, y, 2, ignore=IGN if void else None, dtype=dtype)
    assert float(loss) == 1.0 and (per == 1).all() and not grad.any() and bool(torch.isfinite(grad).all())


def test_all_void_and_nan():
    z, y = generic(3, 6, 8, seed=9)
    y[1] = IGN
    loss, grad, per = boundary.loss_host(z, y, 2, ignore=IGN)
    assert float(per[1]) == 0.0 and not grad[1].any() and float(per[0]) > 0 and float(per[2]) > 0
    assert float(loss) == pytest.approx(float(per[0] + per[2]) / 3, rel=1e-15)
    lo, gr, _ = boundary.loss_host(z[1:2], y[1:2], 2, ignore=IGN)
    assert float(lo) == 0.0 and not gr.any()
    z2 = z.clone()
    z2[0, 2, 3] = float('nan')
    assert torch.isnan(boundary.loss_host(z2, y, 2, ignore=IGN)[0])
    y[0, 2, 3] = IGN                                         # the same logit under a void pixel never reaches the result
    clean = z.clone()
    clean[0, 2, 3] = 0.0
    a, b = boundary.loss_host(z2, y, 2, ignore=IGN), boundary.loss_host(clean, y, 2, ignore=IGN)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[1]).all())


# ---- the tie rule ----------------------------------------------------------------------------------------------------------
def test_the_tie_rule_decides_where_the_gradient_goes():
    """5 x 7, logits from three levels: q has plateaus, so both arg-max maps meet exact ties.  The first maximum in row-major
    order must take the gradient; taking the last instead gives a different gradient, so this case tells the two apart."""
    lv = {0: -3.0, 1: -0.5, 2: 1.25}
    pat = [[0, 0, 0, 1, 1, 2, 2],
           [0, 0, 1, 1, 1, 2, 2],
           [0, 1, 1, 1, 2, 2, 2],
           [0, 0, 1, 1, 1, 2, 2],
           [0, 0, 0, 1, 1, 2, 2]]
    z = torch.tensor([[lv[v] for v in row] for row in pat], dtype=torch.float64)[None]
    y = torch.tensor([[1.0 if v == 0 else 0.0 for v in row] for row in pat], dtype=torch.float64)[None]
    loss, grad, _ = boundary.loss_host(z, y, 1)
    ref_loss, ref_grad = closed_form(z.numpy(), y.numpy(), 1)
    assert abs(float(loss) - ref_loss) <= 1e-15 and np.abs(grad.numpy() - ref_grad).max() <= 1e-16
    # the mirrored problem, mirrored back, is "last maximum in the row wins": it must differ, or the case decides nothing
    _, flipped = closed_form(z.numpy()[:, :, ::-1].copy(), y.numpy()[:, :, ::-1].copy(), 1)
    assert np.abs(flipped[:, :, ::-1] - ref_grad).max() > 1e-3 * np.abs(ref_grad).max()
