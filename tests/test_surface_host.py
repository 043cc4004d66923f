"""Host-side checks of the distance-weighted surface loss (no GPU): the spelled names and the keyword rules, the ids at every
layer, and the numpy twins of `eosvos_amd.surface` against the definition written as all-pairs loops (tests/surface_ref.py):
the capped distances bit for bit, the loss and the gradient in fp64, the gradient against central differences."""
import os
import re

import numpy as np
import pytest
import torch

import surface_ref as ref
from eosvos_amd import loss_names, loss_sum, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = ref.IGN
N = 'surface'
SHAPES = [(1, 1, 1), (1, 9, 3), (9, 1, 3), (5, 7, 1), (17, 33, 4), (20, 70, 200)]      # (H, W, cap); the last cap is beyond the frame


# ---- names ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,want', [(N, (N, None)), (N + '_1', (N, 1)), (N + '_64', (N, 64)), (N + '_4095', (N, 4095)),
                                       ('dice', ('dice', None)), ('boundary_f_8', ('boundary_f_8', None)), ('surf', ('surf', None))])
def test_parse_accepts(name, want):
    assert surface.parse(name) == want


@pytest.mark.parametrize('name', [N + '_0', N + '_08', N + '_4096', N + 's', N + '_', N + '8', N + '_2.5', N + '_-5', N + '_8_8'])
def test_parse_rejects_under_the_prefix(name):
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError):
        surface.parse(name)
    with pytest.raises(NotImplementedError):
        resolve_loss(name)
    with pytest.raises(NotImplementedError):
        loss_sum.resolve('dice+' + name)
    with pytest.raises(NotImplementedError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_the_spellings_resolve():
    from eosvos_amd import engine
    assert loss_names.resolve_loss(N) == (10, None) and loss_names.resolve_loss(N + '_64') == (10, None)
    assert loss_names.resolve_cap(N) is None and loss_names.resolve_cap(N + '_64') == 64 and loss_names.resolve_cap(N, 8) == 8
    assert loss_names.resolve_cap(N + '_8', 8) == 8 and loss_names.resolve_cap('dice') is None
    kinds, weights, names, f, r = loss_sum.resolve('0.5*surface_8+dice')
    assert (kinds, weights, names, f, r) == ([10, 1], [0.5, 1.0], ['surface_8', 'dice'], None, None)
    assert loss_sum.resolve_cap('0.5*surface_8+dice') == 8 and loss_sum.resolve_cap('0.5*surface+dice', 12) == 12
    assert loss_sum.resolve_cap('dice+lovasz_hinge') is None and loss_sum.resolve_cap(N) is None
    # a boundary kind beside it is allowed: the radius and the cap are separate
    assert loss_sum.resolve('surface_32+boundary_f_4')[0] == [10, 8] and loss_sum.resolve('surface_32+boundary_f_4')[4] == 4
    assert loss_sum.resolve_cap('surface_32+boundary_f_4') == 32
    spec = engine._resolve('dice+0.5*surface_64', None, None, None)
    assert (spec.n, list(spec.kinds), list(spec.weights), spec.combine, spec.fraction, spec.radius, spec.cap) == \
        (2, [1, 10], [1.0, 0.5], True, None, None, 64)
    spec = engine._resolve(N, None, None, 7)
    assert (spec.n, list(spec.kinds), spec.combine, spec.cap) == (1, [10], False, 7)
    assert engine._resolve('dice', None, None).cap is None


def test_the_keyword_rules():
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    for other in ('dice', 'cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy', 'boundary_f_4'):
        with pytest.raises(ValueError):                     # the keyword belongs to this kind alone
            resolve_loss(other, cap=8)
        with pytest.raises(ValueError):
            loss_sum.resolve_cap(other + '+cross_entropy_and_dice', 8)
        with pytest.raises(ValueError):
            compute_loss(other, z, z, {'cap': 8})
    with pytest.raises(ValueError):                         # suffix and keyword disagree
        loss_names.resolve_cap(N + '_8', 4)
    with pytest.raises(ValueError):
        loss_sum.resolve_cap('dice+surface_8', 4)
    with pytest.raises(ValueError):
        compute_loss('dice+surface_8', z, z, {'cap': 4})
    with pytest.raises(ValueError):                         # the kind twice
        loss_sum.resolve('surface+surface_8')
    with pytest.raises(ValueError):
        loss_sum.resolve_cap('surface+surface_8')
    for bad in (0, 4096, -1, 2.5, float('nan'), float('inf'), True, 'x', None):
        with pytest.raises(ValueError):
            surface.check_cap(bad)
    for bad in (0, 4096, -1, 2.5, True):
        with pytest.raises(ValueError):
            resolve_loss(N, cap=bad)
    assert [surface.check_cap(c) for c in (1, 64, 4095, 4.0)] == [1, 64, 4095, 4]
    with pytest.raises(ValueError):                         # the other families' keywords do not belong to it
        resolve_loss(N, fraction=0.25)
    with pytest.raises(ValueError):
        resolve_loss(N, radius=4)
    with pytest.raises(ValueError):
        loss_sum.resolve('surface+dice', radius=4)
    for name, kw in ((N, None), (N + '_8', {'cap': 8}), ('dice+0.5*surface', {'cap': 2})):
        with pytest.raises(RuntimeError):                   # known spellings, but logits that no engine produced
            compute_loss(name, z, z, kw)


def test_the_pinned_tables_are_unchanged():
    assert loss_names.LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                                     'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, 'bootstrapped_cross_entropy': 6}
    assert loss_names.BOUNDARY_KINDS == {'boundary_f': 8, 'cross_entropy_and_boundary_f': 9}
    assert loss_names.SURFACE_KINDS == surface.KINDS == {N: 10} and loss_names.MAX_CAP == 4095
    assert loss_sum.MAX_TERMS == 4


def test_the_kind_is_declared_at_every_layer():
    from eosvos_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_SURFACE\s+10\b', header)
    assert not re.search(r'#define\s+EOSVOS_LOSS_\w+\s+7\b', header)          # kind 7 stays unassigned
    assert re.search(r'int\s+eosvos_set_loss_surface\(eosvos_engine\*\s*e,\s*int\s+cap\)', header)
    for name, n_args in (('eosvos_set_loss_surface', 2), ('eosvos_surface_loss', 10), ('eosvos_surface_weights', 9)):
        assert name + '(' in header and name in _ffi.exported_symbols() and len(_ffi._SIGNATURES[name][1]) == n_args
    makefile = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'Makefile')).read()
    assert 'surface_kernels.o' in makefile
    engine_cpp = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'engine.cpp')).read()
    assert 'EOSVOS_LOSS_SURFACE' in engine_cpp and 'launch_surface' in engine_cpp
    for name in ('eosvos_set_loss_surface', 'eosvos_surface_loss', 'eosvos_surface_weights'):
        assert re.search(r'\bint\s+' + name + r'\(', engine_cpp), name


def test_the_default_cap():
    assert surface.default_cap(480, 854) == 120 and surface.default_cap(112, 176) == 28
    assert surface.default_cap(1, 1) == 1 and surface.default_cap(3, 900) == 1 and surface.default_cap(4096 * 8, 4096 * 8) == 4095


# ---- the capped distances, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('kind', ref.TARGETS)
@pytest.mark.parametrize('H,W,cap', SHAPES)
def test_distance_host_equals_the_all_pairs_loops(H, W, cap, kind, void):
    y = ref.target(kind, H, W, void)
    ign = IGN if ref.uses_void(kind, void) else None
    want = ref.distance_loops(y, cap, ign)
    got = surface.distance_host(y, cap, ign)
    assert got.dtype == np.int32 and got.shape == (H, W)
    assert np.array_equal(got, want)
    assert np.array_equal(surface.distance_host(np.stack([y, y]), cap, ign), np.stack([want, want]))
    if ign is not None:
        assert not got[y == IGN].any()
    valid = np.ones_like(y, dtype=bool) if ign is None else y != IGN
    assert (got[valid] >= 1).all() and (got <= cap * cap + 1).all()
    w = surface.weights_host(got, cap)
    assert w.dtype == np.float32 and (w[valid] > 0).all() and (w <= 1).all() and not w[~valid].any()
    lf = np.float32(cap)                                    # rule 2, spelled out
    assert np.array_equal(w, np.where(got > cap * cap, lf, np.sqrt(got.astype(np.float32))) / lf)
    assert np.abs(surface.weights_host(got, cap, np.float64) - ref.weights_loops(got, cap)).max() <= 2e-16


def test_the_degenerate_targets_by_hand():
    H, W, cap = 5, 7, 3
    for kind in ('empty', 'full'):                          # no pixel of the other class: the cap everywhere, w = 1
        c = surface.distance_host(ref.target(kind, H, W, False), cap)
        assert (c == cap * cap + 1).all() and (surface.weights_host(c, cap) == 1).all()
    c = surface.distance_host(ref.target('all_void', H, W, False), cap, IGN)
    assert not c.any()
    c = surface.distance_host(ref.target('corner', H, W, False), 200)
    assert c[0, 0] == 1 and c[0, 1] == 1 and c[4, 6] == 16 + 36 and c[2, 3] == 4 + 9
    c = surface.distance_host(ref.target('checkerboard', H, W, False), cap)
    assert (c == 1).all()
    y = ref.target('void_band', 5, 9, False)                 # F in columns 0 .. 2, void in 3 .. 5, B in 6 .. 8
    c = surface.distance_host(y, 200, IGN)
    assert c[2].tolist() == [36, 25, 16, 0, 0, 0, 16, 25, 36]


# ---- the loss and the gradient ---------------------------------------------------------------------------------------------
def logits_for(y, seed):
    rng = np.random.RandomState(seed)
    sign = np.where(y >= 0.5, 1.0, -1.0)
    return (2 * rng.randn(*y.shape) + 3 * sign * rng.rand(*y.shape)).astype(np.float32)


@pytest.mark.parametrize('void', [False, True])
@pytest.mark.parametrize('kind', ref.TARGETS)
def test_loss_host_equals_the_loops(kind, void):
    H, W, cap = 9, 13, 4
    y = np.stack([ref.target(kind, H, W, void), ref.target('blob', H, W, void), ref.target('all_void', H, W, False)])
    ign = IGN
    z = logits_for(y, 3)
    z[y == IGN] = np.nan                                     # a void logit never reaches the result
    want_l, want_g = ref.loss_loops(np.where(y == IGN, 0, z).astype(np.float64), y, cap, ign)
    loss, grad = surface.loss_host(z, y, cap, ign)
    assert grad.dtype == np.float64 and grad.shape == z.shape
    assert abs(float(loss) - want_l) <= 1e-14                # ~100 terms of <= 1 each, two summation orders, two forms of p
    assert np.abs(grad - want_g).max() <= 1e-16
    void_px = y == IGN
    assert not grad[void_px].any() and not np.signbit(grad[void_px]).any() and not grad[2].any()
    l32, g32 = surface.loss_host(z, y, cap, ign, dtype=np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32
    assert abs(float(l32) - want_l) <= 1e-6 and np.abs(g32 - want_g).max() <= 1e-7
    one_l, one_g = surface.loss_host(z[1], y[1], cap, ign)   # (H, W) is one image
    assert one_g.shape == (H, W) and abs(float(one_l) - ref.loss_loops(np.where(y[1:2] == IGN, 0, z[1:2]).astype(np.float64), y[1:2], cap, ign)[0]) <= 1e-15


def test_an_empty_target_gives_the_mean_foreground_probability_and_an_all_void_batch_zero():
    y = np.zeros((2, 6, 8), dtype=np.float32)
    z = logits_for(y + 1, 5)
    loss, grad = surface.loss_host(z, y, 3)
    p = 1 / (1 + np.exp(-z.astype(np.float64)))
    assert abs(float(loss) - p.mean()) <= 1e-14
    assert np.abs(grad - p * (1 - p) / z.size).max() <= 1e-17
    loss, grad = surface.loss_host(z, np.full_like(y, IGN), 3, IGN)
    assert float(loss) == 0.0 and not grad.any()
    perfect = np.where(ref.target('blob', 6, 8, False) >= 0.5, 80.0, -80.0).astype(np.float32)
    loss, grad = surface.loss_host(perfect, ref.target('blob', 6, 8, False), 3)
    assert 0 <= float(loss) <= 1e-30 and np.abs(grad).max() <= 1e-30


@pytest.mark.parametrize('void', [False, True])
def test_the_gradient_matches_central_differences(void):
    H, W, cap = 6, 8, 3
    y = np.stack([ref.target('blob', H, W, void), ref.target('void_band', H, W, False)])
    ign = IGN
    z = logits_for(y, 11).astype(np.float64)
    _, grad = surface.loss_host(z, y, cap, ign)
    h = 1e-5
    for idx in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        fd = (float(surface.loss_host(zp, y, cap, ign)[0]) - float(surface.loss_host(zm, y, cap, ign)[0])) / (2 * h)
        assert abs(fd - grad[idx]) <= 1e-9, (idx, fd, grad[idx])          # h^2 |f'''| / 6 <= 1e-10 / 6 / 96; rounding 1e-16 / h
    assert np.abs(grad).max() > 1e-4


def test_torch_tensors_are_taken_too():
    y = ref.target('blob', 6, 8, True)
    z = logits_for(y, 2)
    a = surface.loss_host(z, y, 3, IGN)
    b = surface.loss_host(torch.from_numpy(z), torch.from_numpy(y), 3, IGN)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(surface.distance_host(torch.from_numpy(y), 3, IGN), surface.distance_host(y, 3, IGN))
