"""Host-side checks of the topology-aware centreline loss `cldice` (no GPU): the spelled names and the keyword rules, the ids at
every layer, and the numpy twins of `eosvos_amd.cldice` against the rule written as per-pixel loops (tests/cldice_ref.py) bit
for bit in float64 and float32, against torch autograd of the published implementation in float64, and on the topology
property that is the loss's purpose."""
import os
import re

import numpy as np
import pytest
import torch

import cldice_ref as ref
from eosvos_amd import cldice, loss_names, loss_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = ref.IGN
N = 'cldice'
_CACHE = {}


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a)), np.atleast_1d(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def case(images, H, W, depth):
    """The shared inputs of a case and its float64 twin, computed once."""
    key = (images, H, W, depth)
    if key not in _CACHE:
        z, y = ref.case(images, H, W, seed=H + W)
        _CACHE[key] = (z, y, cldice.loss_host(z, y, depth))
    return _CACHE[key]


# ---- names ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,want', [(N, (N, None)), (N + '_1', (N, 1)), (N + '_5', (N, 5)), (N + '_16', (N, 16)),
                                       ('dice', ('dice', None)), ('surface_8', ('surface_8', None)), ('cldic', ('cldic', None))])
def test_parse_accepts(name, want):
    assert cldice.parse(name) == want


@pytest.mark.parametrize('name', [N + '_0', N + '_17', N + '_05', N + '_x', N + 's', N + '_', N + '5', N + '_2.5', N + '_-5', N + '_5_5'])
def test_parse_rejects_under_the_prefix(name):
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError):
        cldice.parse(name)
    with pytest.raises(NotImplementedError):
        resolve_loss(name)
    with pytest.raises(NotImplementedError):
        loss_sum.resolve('dice+' + name)
    with pytest.raises(NotImplementedError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_the_spellings_resolve():
    from eosvos_amd import engine
    assert loss_names.resolve_loss(N) == (13, None) and loss_names.resolve_loss(N + '_5') == (13, None)
    assert loss_names.resolve_depth(N) is None and loss_names.resolve_depth(N + '_5') == 5 and loss_names.resolve_depth(N, 8) == 8
    assert loss_names.resolve_depth(N + '_8', 8) == 8 and loss_names.resolve_depth('dice') is None
    kinds, weights, names, f, r = loss_sum.resolve('dice+0.5*cldice_5')
    assert (kinds, weights, names, f, r) == ([1, 13], [1.0, 0.5], ['dice', 'cldice_5'], None, None)
    assert loss_sum.resolve_depth('dice+0.5*cldice_5') == 5 and loss_sum.resolve_depth('0.5*cldice+dice', 12) == 12
    assert loss_sum.resolve_depth('dice+lovasz_hinge') is None and loss_sum.resolve_depth(N) is None
    # the other frame-shape kinds beside it are allowed: radius, cap and depth are separate
    assert loss_sum.resolve('cldice_3+boundary_f_4+surface_9')[0] == [13, 8, 10]
    assert loss_sum.resolve_depth('cldice_3+boundary_f_4+surface_9') == 3
    spec = engine._resolve('dice+0.5*cldice_5', None, None)
    assert (spec.n, list(spec.kinds), list(spec.weights), spec.combine, spec.fraction, spec.radius, spec.cap, spec.depth) == \
        (2, [1, 13], [1.0, 0.5], True, None, None, None, 5)
    spec = engine._resolve(N, None, None, None, None, 7)
    assert (spec.n, list(spec.kinds), spec.combine, spec.depth) == (1, [13], False, 7)
    assert engine._resolve('dice', None, None).depth is None


def test_the_keyword_rules():
    from eosvos_amd.engine import resolve_loss
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    for other in ('dice', 'cross_entropy', 'lovasz_hinge', 'bootstrapped_cross_entropy', 'boundary_f_4', 'surface', 'potts'):
        with pytest.raises(ValueError):                     # the keyword belongs to this kind alone
            resolve_loss(other, depth=3)
        with pytest.raises(ValueError):
            loss_sum.resolve_depth(other + '+cross_entropy_and_dice', 3)
        with pytest.raises(ValueError):
            compute_loss(other, z, z, {'depth': 3})
    with pytest.raises(ValueError):                         # suffix and keyword disagree
        loss_names.resolve_depth(N + '_8', 4)
    with pytest.raises(ValueError):
        loss_sum.resolve_depth('dice+cldice_8', 4)
    with pytest.raises(ValueError):
        compute_loss('dice+cldice_8', z, z, {'depth': 4})
    with pytest.raises(ValueError):                         # the kind twice
        loss_sum.resolve('cldice+cldice_8')
    with pytest.raises(ValueError):
        loss_sum.resolve_depth('cldice+cldice_8')
    for bad in (0, 17, -1, 2.5, float('nan'), float('inf'), True, False, 'x', None):
        with pytest.raises(ValueError):
            cldice.check_depth(bad)
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError):
            resolve_loss(N, depth=bad)
    assert [cldice.check_depth(c) for c in (1, 5, 16, 4.0)] == [1, 5, 16, 4]
    with pytest.raises(ValueError):                         # the other families' keywords do not belong to it
        resolve_loss(N, fraction=0.25)
    with pytest.raises(ValueError):
        resolve_loss(N, radius=4)
    with pytest.raises(ValueError):
        resolve_loss(N, cap=4)
    with pytest.raises(ValueError):
        resolve_loss(N, window=2)
    for name, kw in ((N, None), (N + '_8', {'depth': 8}), ('dice+0.5*cldice', {'depth': 2})):
        with pytest.raises(RuntimeError):                   # known spellings, but logits that no engine produced
            compute_loss(name, z, z, kw)


def test_the_tables():
    assert loss_names.LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                                     'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, 'bootstrapped_cross_entropy': 6}
    assert loss_names.BOUNDARY_KINDS == {'boundary_f': 8, 'cross_entropy_and_boundary_f': 9}
    assert loss_names.SURFACE_KINDS == {'surface': 10} and loss_names.POTTS_KINDS == {'potts': 12}
    assert loss_names.CLDICE_KINDS == cldice.KINDS == {N: 13} and loss_names.MAX_DEPTH == cldice.MAX_DEPTH == 16
    assert loss_sum.MAX_TERMS == 4


def test_the_kind_is_declared_at_every_layer():
    from eosvos_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_CLDICE\s+13\b', header)
    for unassigned in (7, 11, 14):
        assert not re.search(r'#define\s+EOSVOS_LOSS_\w+\s+%d\b' % unassigned, header)
    assert re.search(r'int\s+eosvos_set_loss_cldice\(eosvos_engine\*\s*e,\s*int\s+depth\)', header)
    for name, n_args in (('eosvos_set_loss_cldice', 2), ('eosvos_cldice_loss', 10), ('eosvos_soft_skeleton', 9)):
        declared = re.search(r'\bint\s+' + name + r'\(([^)]*)\)', header)
        assert declared and len(declared.group(1).split(',')) == n_args, name
        assert name in _ffi.exported_symbols() and len(_ffi._SIGNATURES[name][1]) == n_args, name
    makefile = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'Makefile')).read()
    assert 'cldice_kernels.o' in makefile
    engine_cpp = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'engine.cpp')).read()
    assert 'EOSVOS_LOSS_CLDICE' in engine_cpp and 'launch_cldice' in engine_cpp


def test_the_entry_points_refuse_a_null_engine():
    from eosvos_amd import _ffi
    lib = _ffi.load()
    # null engines are refused on the host, before anything touches a device
    assert lib.eosvos_set_loss_cldice(None, 3) != 0 and b'null' in lib.eosvos_last_error()
    assert lib.eosvos_cldice_loss(None, None, None, 1, 4, 4, 3, None, None, None) != 0 and b'null' in lib.eosvos_last_error()
    assert lib.eosvos_soft_skeleton(None, None, None, 1, 4, 4, 3, None, None) != 0 and b'null' in lib.eosvos_last_error()


def test_the_spelling_survives_the_command_line():
    from eosvos_amd import config
    spelled = 'dice+0.5*cldice_5'
    found = []

    def walk(x):
        if isinstance(x, dict):
            for k, v in x.items():
                if k == 'loss_func':
                    found.append(v)
                walk(v)
    walk(config.parse_cli(['with', f'loss_func={spelled}']))
    assert found and all(v == spelled for v in found), found
    assert loss_sum.resolve(spelled)[0] == [1, 13] and loss_sum.resolve_depth(spelled) == 5


def test_the_default_depth():
    assert cldice.default_depth(480, 854) == 5 and cldice.default_depth(112, 176) == 1 and cldice.default_depth(9, 9) == 1
    assert cldice.default_depth(4096, 4096) == 16 and cldice.default_depth(240, 427) == 3


# ---- the twins against the loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_the_twins_equal_the_loops_bit_for_bit(images, H, W, depth, dtype):
    z, y, _ = case(images, H, W, depth)
    lt, gt = cldice.loss_host(z, y, depth, dtype=dtype)
    ll, gl = ref.loss_loops(z, y, depth, dtype=dtype)
    assert lt.dtype == gt.dtype == np.dtype(dtype) and gt.shape == z.shape
    assert same_bits(lt, ll)
    assert np.array_equal(gt, gl) and np.isfinite(gt).all()
    p = cldice.sigmoid_host(z.astype(dtype), dtype)[0]
    for maps in (p, y):
        st = cldice.skeleton_host(maps, depth, dtype=dtype)
        assert st.dtype == np.dtype(dtype) and np.array_equal(st, ref.skeleton_loops(maps, depth, dtype=dtype))
        assert st.min() >= 0 and st.max() <= 1
    assert H == 1 or cldice.skeleton_host(y, depth).max() > 0      # (the one-row bar of 7 pixels outlasts 2 erosions: S(y) = 0)


@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_a_tenth_of_the_pixels_void(images, H, W, depth, dtype):
    z, y, _ = case(images, H, W, depth)
    yv = ref.speckle(y, seed=H)
    lt, gt = cldice.loss_host(z, yv, depth, ignore=IGN, dtype=dtype)
    ll, gl = ref.loss_loops(z, yv, depth, ignore=IGN, dtype=dtype)
    assert same_bits(lt, ll) and np.array_equal(gt, gl)
    void = yv == IGN
    assert same_bits(gt[void], np.zeros_like(gt[void]))          # exactly +0
    st = cldice.skeleton_host(y, depth, ignore=IGN, masks=yv, dtype=dtype)
    assert np.array_equal(st, ref.skeleton_loops(y, depth, valid=~void, dtype=dtype)) and not st[void].any()


# ---- the float64 twin against the published implementation ---------------------------------------------------------------
@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
def test_the_twin_matches_torch_autograd_of_the_published_form(images, H, W, depth):
    z, y, (l64, g64) = case(images, H, W, depth)
    lp, gp = ref.published(z, y, depth)
    dl, dg = abs(float(l64) - lp), float(np.abs(g64 - gp).max())
    print(f'PARITY published B={images} {H}x{W} k={depth}: loss {float(l64):.15g} diff {dl:.3e}, gradient diff {dg:.3e}')
    assert dl <= 1e-12 and dg <= 1e-12


@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
def test_the_product_form_equals_the_published_recurrence(images, H, W, depth):
    z, y, _ = case(images, H, W, depth)
    p = cldice.sigmoid_host(z.astype(np.float64), np.float64)[0]
    valid = np.ones(p.shape, dtype=bool)
    for maps in (p, y.astype(np.float64)):
        s, ds, _ = cldice._chain(maps, valid, depth)
        skel = ds[0]
        for d in ds[1:]:
            t = d - skel * d
            skel = skel + np.where(t > 0, t, 0.0)
        assert float(np.abs(skel - s).max()) <= 1e-14


@pytest.mark.parametrize('images,H,W,depth', ref.CASES)
def test_a_void_ring_changes_nothing_inside(images, H, W, depth):
    z, y, (l64, g64) = case(images, H, W, depth)
    zz, yy, inner = ref.void_ring(z, y)
    lr, gr = cldice.loss_host(zz, yy, depth, ignore=IGN)
    assert abs(float(lr) - float(l64)) <= 1e-15
    assert float(np.abs(gr[inner] - g64.reshape(-1)).max()) <= 1e-15
    ring = gr[~inner]
    assert same_bits(ring, np.zeros_like(ring))                  # exactly +0


# ---- what the loss is for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 3, 5])
def test_a_cut_costs_far_more_than_a_shave(depth):
    y, cut, shave = ref.bar_and_blob()
    assert (y - cut).sum() == (y - shave).sum() == 4
    l_cut = float(cldice.loss_host(np.where(cut > 0, 8.0, -8.0), y, depth)[0])
    l_shave = float(cldice.loss_host(np.where(shave > 0, 8.0, -8.0), y, depth)[0])
    print(f'PARITY topology k={depth}: cut {l_cut:.6g} shave {l_shave:.6g} factor {l_cut / l_shave:.1f}')
    assert l_shave > 0 and l_cut > 10 * l_shave


def test_the_edge_cases():
    z, y, _ = case(2, 19, 37, 3)
    for target in (np.zeros_like(y), np.ones_like(y)):                      # an empty and a full target: no special case
        l, g = cldice.loss_host(z, target, 3)
        assert np.isfinite(l) and np.isfinite(g).all() and 0 <= l <= 1
    l, g = cldice.loss_host(z, np.full_like(y, IGN), 3, ignore=IGN)         # no valid pixel
    assert l == 0 and not g.any()
    one = y.copy()
    one[1] = IGN                                                            # ... in one image of two: it adds 0 to the mean
    l1, g1 = cldice.loss_host(z, one, 3, ignore=IGN)
    l0, g0 = cldice.loss_host(z[:1], y[:1], 3)
    assert abs(float(l1) - float(l0) / 2) <= 1e-15 and not g1[1].any() and float(np.abs(g1[0] - g0[0] / 2).max()) <= 1e-15
    for v in (40.0, -40.0):
        for dtype in (np.float64, np.float32):
            l, g = cldice.loss_host(np.full_like(z, v), y, 3, dtype=dtype)
            assert np.isfinite(l) and np.isfinite(g).all()
    bad = z.copy()
    bad[0, 3, 5] = np.nan
    assert np.isnan(cldice.loss_host(bad, y, 3)[0]) and np.isnan(cldice.loss_host(bad, y, 3, dtype=np.float32)[0])
    void = y.copy()
    void[0, 3, 5] = IGN                                                     # ... but a void pixel's logit never reaches the result
    l, g = cldice.loss_host(bad, void, 3, ignore=IGN)
    assert np.isfinite(l) and np.isfinite(g).all()


def test_torch_tensors_and_single_maps_are_taken_too():
    z, y, (l64, g64) = case(1, 7, 7, 1)
    l, g = cldice.loss_host(torch.from_numpy(z[0]), torch.from_numpy(y[0]), 1)
    assert g.shape == (7, 7) and l == l64 and np.array_equal(g, g64[0])
    with pytest.raises(ValueError):
        cldice.loss_host(z, y[:, :3], 1)
    with pytest.raises(ValueError):
        cldice.skeleton_host(y, 0)
