"""Host-side checks of the image-aware pairwise loss `potts` (no GPU): the numpy twin of `eosvos_amd.potts` against the
definition written as per-pixel, per-neighbour loops (tests/potts_ref.py) and against central differences of itself, the
closed cases, the spelled names and keyword rules, and the ids and symbols at every layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import potts_ref as ref
from eosvos_amd import loss_names, loss_sum, potts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 'potts'
SHAPES = [(5, 7), (9, 4), (1, 6)]
WINDOWS = [(1, 1), (2, 2), (3, 2)]                          # (3, 2): a window of 13 x 13 pixels, wider than every frame above


def rel(a, b):
    """The largest difference relative to the largest reference magnitude (0 for two all-zero arrays)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / scale if scale else float(np.abs(a - b).max())


# ---- the twin against the loops --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r,d', WINDOWS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_loss_host_equals_the_loops(H, W, r, d):
    z, img = ref.case(2, H, W, seed=H * W + r)
    E, Z, loss, grad = ref.loops(z, img, r, d, 2.5, 0.15)
    l64, g64 = potts.loss_host(z, img, r, d, 2.5, 0.15, np.float64)
    assert l64.dtype == np.float64 and g64.dtype == np.float64 and g64.shape == z.shape
    assert (Z > 0).all() and loss > 0
    assert abs(float(l64) - loss) <= 1e-12 * loss
    assert rel(g64, grad) <= 1e-12
    one = potts.loss_host(z[1], img[1], r, d, 2.5, 0.15)                         # (H, W) and (3, H, W); fp64 by default
    assert one[1].shape == (H, W) and abs(float(one[0]) - E[1] / Z[1]) <= 1e-12 * E[1] / Z[1]
    l32, g32 = potts.loss_host(z, img, r, d, 2.5, 0.15, np.float32)
    assert l32.dtype == np.float32 and g32.dtype == np.float32
    assert abs(float(l32) - loss) <= 1e-4 * loss and rel(g32, grad) <= 1e-4      # (the same rule, in single precision)


def test_the_default_sigma_xy_is_the_halo():
    z, img = ref.case(1, 5, 7, seed=1)
    a = potts.loss_host(z, img, 2, 2)
    b = potts.loss_host(z, img, 2, 2, 4.0, 0.1)
    assert potts.default_sigma_xy(3, 2) == 6.0 and float(a[0]) == float(b[0]) and np.array_equal(a[1], b[1])
    assert (potts.DEFAULT_WINDOW, potts.DEFAULT_DILATION, potts.DEFAULT_SIGMA_RGB) == (3, 2, 0.1)


@pytest.mark.parametrize('r,d', WINDOWS)
def test_the_gradient_matches_central_differences(r, d):
    z, img = ref.case(2, 5, 7, seed=11)
    z = (z / 4).astype(np.float64)
    _, g = potts.loss_host(z, img, r, d, 2.5, 0.15)
    h = 1e-6
    num = np.zeros_like(g)
    for i in range(z.size):
        zp, zm = z.copy(), z.copy()
        zp.reshape(-1)[i] += h
        zm.reshape(-1)[i] -= h
        num.reshape(-1)[i] = (float(potts.loss_host(zp, img, r, d, 2.5, 0.15)[0]) - float(potts.loss_host(zm, img, r, d, 2.5, 0.15)[0])) / (2 * h)
    assert rel(g, num) <= 1e-7                              # O(h^2) truncation + rounding of the quotient, on |g| ~ 1e-2


# ---- closed cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [40.0, -40.0])
def test_constant_saturated_logits_give_zero(value):
    _, img = ref.case(2, 9, 4, seed=3)
    z = np.full((2, 9, 4), value)
    loss, grad = potts.loss_host(z, img, 2, 2, 4.0, 0.1)
    assert abs(float(loss)) <= 1e-15 and float(np.abs(grad).max()) <= 1e-15      # p within 4e-18 of 0 or 1
    assert float(ref.loops(z, img, 2, 2, 4.0, 0.1)[2]) <= 1e-15


def test_a_one_pixel_image_gives_zero_and_no_gradient():
    for dtype in (np.float64, np.float32):
        loss, grad = potts.loss_host(np.array([[0.7]]), np.full((3, 1, 1), 0.4), 3, 2, 6.0, 0.1, dtype)
        assert float(loss) == 0.0 and grad.shape == (1, 1) and float(grad[0, 0]) == 0.0
    assert ref.loops(np.full((1, 1, 1), 0.7), np.full((1, 3, 1, 1), 0.4), 3, 2, 6.0, 0.1)[2] == 0.0


def test_a_half_plane_step_on_a_constant_image():
    H, W = 6, 8
    z = np.where(np.arange(W)[None, :] < 4, 30.0, -30.0) * np.ones((1, H, 1))
    img = np.full((1, 3, H, W), 0.3)
    _, _, want, gwant = ref.loops(z, img, 2, 1, 2.0, 0.1)
    loss, grad = potts.loss_host(z, img, 2, 1, 2.0, 0.1)
    assert want > 0.05                                      # the pairs across the step, over all pairs
    assert abs(float(loss) - want) <= 1e-12 * want and rel(grad, gwant) <= 1e-12
    flat = potts.loss_host(np.full((1, H, W), 30.0), img, 2, 1, 2.0, 0.1)[0]
    assert float(flat) < 1e-12 < float(loss)


def test_an_offset_of_the_frame_changes_nothing_beyond_the_rounding_of_the_differences():
    z, img = ref.case(2, 5, 7, seed=5)
    img = np.round(img.astype(np.float64) * 256) / 256       # multiples of 2^-8: with an offset of 3 the differences stay exact
    a = potts.loss_host(z, img, 2, 2, 4.0, 0.1)
    b = potts.loss_host(z, img + 3.0, 2, 2, 4.0, 0.1)
    assert float(a[0]) == float(b[0]) and np.array_equal(a[1], b[1])
    c = potts.loss_host(z, img + 0.1, 2, 2, 4.0, 0.1)       # an offset that rounds the differences: 1 ulp of 1.1 each, times 1 / sigma^2
    assert abs(float(c[0]) - float(a[0])) <= 1e-12 * float(a[0]) and rel(c[1], a[1]) <= 1e-12


def test_a_nan_logit_makes_the_loss_nan_and_torch_tensors_are_taken():
    z, img = ref.case(1, 5, 7, seed=6)
    good = potts.loss_host(torch.from_numpy(z), torch.from_numpy(img), 1, 1, 1.0, 0.1)
    assert np.isfinite(float(good[0]))
    z[0, 2, 3] = np.nan
    assert np.isnan(float(potts.loss_host(z, img, 1, 1, 1.0, 0.1)[0]))
    with pytest.raises(ValueError):
        potts.loss_host(z, img[:, :2], 1, 1, 1.0, 0.1)
    for bad in ((0, 1, 1.0, 0.1), (8, 1, 1.0, 0.1), (5, 4, 1.0, 0.1), (2, 5, 1.0, 0.1), (2, 2, 0.0, 0.1), (2, 2, 1.0, -1.0),
                (2, 2, float('nan'), 0.1), (2, 2, 1.0, float('inf'))):
        with pytest.raises(ValueError):
            potts.loss_host(z, img, *bad)


# ---- names ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,want', [(N, (N, None, None)), (N + '_1', (N, 1, None)), (N + '_7', (N, 7, None)),
                                       (N + '_3x2', (N, 3, 2)), (N + '_4x4', (N, 4, 4)), (N + '_7x2', (N, 7, 2)),
                                       ('dice', ('dice', None, None)), ('surface_8', ('surface_8', None, None)),
                                       ('pott', ('pott', None, None))])
def test_parse_accepts(name, want):
    assert potts.parse(name) == want


@pytest.mark.parametrize('name', [N + '_0', N + '_03', N + '_8', N + '_5x4', N + '_3x', N + '_3x0', N + '_3x02', N + '_3x5',
                                  N + 's', N + '_', N + '3', N + '_x2', N + '_3X2', N + '_3x2x1', N + '_2.5', N + '_-3', N + '_3x2\n'])
def test_parse_rejects_under_the_prefix(name):
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError):
        potts.parse(name)
    with pytest.raises(NotImplementedError) as err:
        resolve_loss(name)
    assert str(err.value) == f"loss_func='{name}'"
    with pytest.raises(NotImplementedError):
        loss_sum.resolve('cross_entropy+' + name)
    with pytest.raises(NotImplementedError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_the_spellings_resolve():
    from eosvos_amd import engine
    for name in (N, N + '_3', N + '_3x2'):
        assert loss_names.resolve_loss(name) == (12, None)
    assert loss_names.resolve_window(N) == (None, None) and loss_names.resolve_window(N + '_5') == (5, None)
    assert loss_names.resolve_window(N + '_3x2') == (3, 2) and loss_names.resolve_window(N, 4) == (4, None)
    assert loss_names.resolve_window(N + '_4', 4) == (4, None) and loss_names.resolve_window('dice') is None
    assert loss_sum.parse('cross_entropy+0.1*potts_3x2') == [(1.0, 'cross_entropy'), (float(np.float32(0.1)), 'potts_3x2')]
    kinds, weights, names, f, r = loss_sum.resolve('cross_entropy+0.1*potts_3x2')
    assert (kinds, names, f, r) == ([0, 12], ['cross_entropy', 'potts_3x2'], None, None)
    assert loss_sum.resolve_window('cross_entropy+0.1*potts_3x2') == (3, 2)
    assert loss_sum.resolve_window('cross_entropy+0.1*potts', 2) == (2, None) and loss_sum.resolve_window('dice+surface') is None
    assert loss_sum.resolve('potts+surface_32+boundary_f_4')[0] == [12, 10, 8]   # beside the frame-shape kinds
    spec = engine._resolve('cross_entropy+0.1*potts_3x2', None, None, None, None)
    assert (spec.n, list(spec.kinds), spec.combine, spec.fraction, spec.radius, spec.cap, spec.window) == \
        (2, [0, 12], True, None, None, None, (3, 2))
    spec = engine._resolve(N, None, None, None, 5)
    assert (spec.n, list(spec.kinds), spec.combine, spec.window) == (1, [12], False, (5, None))
    assert engine._resolve('dice', None, None).window is None and engine._resolve('surface_8', None, None).cap == 8


def test_the_keyword_rules():
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    for other in ('dice', 'cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy', 'boundary_f_4', 'surface_8'):
        with pytest.raises(ValueError):                     # the keyword belongs to this kind alone
            resolve_loss(other, window=2)
        with pytest.raises(ValueError):
            loss_sum.resolve_window(other + '+cross_entropy_and_dice', 2)
        with pytest.raises(ValueError):
            compute_loss(other, z, z, {'window': 2})
    with pytest.raises(ValueError):                         # the other families' keywords do not belong to it
        resolve_loss(N, fraction=0.25)
    with pytest.raises(ValueError):
        resolve_loss(N, radius=4)
    with pytest.raises(ValueError):
        resolve_loss(N, cap=8)
    with pytest.raises(ValueError):
        loss_sum.resolve('potts+dice', radius=4)
    with pytest.raises(ValueError):
        loss_sum.resolve('potts+dice', fraction=0.5)
    with pytest.raises(ValueError):
        loss_sum.resolve_cap('potts+dice', 8)
    with pytest.raises(ValueError):
        compute_loss('potts+dice', z, z, {'cap': 8})
    with pytest.raises(ValueError):                         # suffix and keyword disagree, or leave the limits together
        loss_names.resolve_window(N + '_3', 2)
    with pytest.raises(ValueError):
        loss_sum.resolve_window('dice+potts_3x2', 2)
    with pytest.raises(ValueError):
        loss_names.resolve_window(N + '_3x4', 5)
    with pytest.raises(ValueError):
        compute_loss('dice+potts_3', z, z, {'window': 2})
    for two in ('potts+potts', 'potts+0.5*potts_3', 'potts_2+dice+potts_3x2'):   # they would share the engine's one window
        with pytest.raises(ValueError):
            loss_sum.resolve(two)
        with pytest.raises(ValueError):
            loss_sum.resolve_window(two)
        with pytest.raises(ValueError):
            compute_loss(two, z, z)
    for bad in (0, 8, -1, 2.5, float('nan'), float('inf'), True, 'x', None):
        with pytest.raises(ValueError):
            potts.check_window(bad)
    for bad in (0, 8, -1, 2.5, True):
        with pytest.raises(ValueError):
            resolve_loss(N, window=bad)
    for r, d in ((5, 4), (7, 3), (3, 5), (3, 0), (3, 1.5)):
        with pytest.raises(ValueError):
            potts.check_window(r, d)
    assert potts.check_window(7) == 7 and potts.check_window(4.0, 4) == (4, 4) and potts.check_window(7, 2) == (7, 2)
    for bad in (0, -0.1, float('nan'), float('inf'), 1e-60, 1e60, True, 'x', None):      # (1e-60, 1e60: 0 and inf as fp32)
        with pytest.raises(ValueError):
            potts.check_sigma('sigma_rgb', bad)
    assert potts.check_sigma('sigma_rgb', 0.1) == float(np.float32(0.1)) and potts.check_sigma('sigma_xy', 6) == 6.0
    for name, kw in ((N, None), (N + '_3x2', {'window': 3}), ('cross_entropy+0.1*potts', {'window': 2})):
        with pytest.raises(RuntimeError):                   # known spellings, but logits that no engine produced
            compute_loss(name, z, z, kw)


def test_the_tables():
    assert loss_names.POTTS_KINDS == potts.KINDS == {N: 12}
    assert loss_names.LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                                     'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, 'bootstrapped_cross_entropy': 6}
    assert loss_names.BOUNDARY_KINDS == {'boundary_f': 8, 'cross_entropy_and_boundary_f': 9}
    assert loss_names.SURFACE_KINDS == {'surface': 10}
    assert (loss_names.MAX_WINDOW, loss_names.MAX_DILATION, loss_names.MAX_HALO) == (7, 4, 16)
    assert loss_sum.MAX_TERMS == 4


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_the_kind_is_declared_at_every_layer():
    from eosvos_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_POTTS\s+12\b', header)
    assert not re.search(r'#define\s+EOSVOS_LOSS_\w+\s+(7|11)\b', header)     # kinds 7 and 11 stay unassigned
    assert 'void pixels receive' in header and 'UNTUNED' in header
    for name, n_args in (('eosvos_set_loss_potts', 5), ('eosvos_potts_loss', 12)):
        decl = re.search(r'\bint\s+' + name + r'\(([^)]*)\)\s*;', header)
        assert decl and len(decl.group(1).split(',')) == n_args, name
        assert name in _ffi.exported_symbols() and len(_ffi._SIGNATURES[name][1]) == n_args
    makefile = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'Makefile')).read()
    assert 'potts_kernels.o' in makefile
    engine_cpp = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'engine.cpp')).read()
    assert 'EOSVOS_LOSS_POTTS' in engine_cpp and 'launch_potts' in engine_cpp
    for name in ('eosvos_set_loss_potts', 'eosvos_potts_loss'):
        assert re.search(r'\bint\s+' + name + r'\(', engine_cpp), name


def test_the_entry_points_refuse_a_null_engine():
    from eosvos_amd import _ffi
    lib = _ffi.load()
    # null engines are refused on the host, before anything touches a device
    assert lib.eosvos_set_loss_potts(None, 3, 2, ctypes.c_float(6.0), ctypes.c_float(0.1)) != 0
    assert b'null' in lib.eosvos_last_error()
    assert lib.eosvos_potts_loss(None, None, None, 1, 4, 4, 3, 2, ctypes.c_float(6.0), ctypes.c_float(0.1), None, None) != 0
    assert b'null' in lib.eosvos_last_error()


def test_the_spelling_survives_the_command_line_beside_the_void_band():
    from eosvos_amd import config
    spelled = 'cross_entropy+0.1*potts_3x2'
    found, bands = [], []

    def walk(x):
        if isinstance(x, dict):
            for k, v in x.items():
                if k == 'loss_func':
                    found.append(v)
                if k == 'min_prop':
                    bands.append(v)
                walk(v)
    walk(config.parse_cli(['with', f'loss_func={spelled}', 'eval_online_adapt.min_prop=[0.3,0.7]']))
    assert found and all(v == spelled for v in found), found
    assert [0.3, 0.7] in [list(b) if isinstance(b, (list, tuple)) else b for b in bands], bands
    assert loss_sum.resolve(spelled)[0] == [0, 12] and loss_sum.resolve_window(spelled) == (3, 2)
