"""Host-side checks of the Lovasz hinge kinds (no GPU): the fp64 stable-sort restatement the device kernels are held to
reproduces the reference fixture within the reference's own stored noise, and the two kinds are declared at every layer."""
import os
import re

import numpy as np
import pytest

import lovasz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'lovasz.npz'))


@pytest.mark.parametrize('tag,per_image', [('per_image', True), ('flat', False), ('zero', True)])
def test_restatement_reproduces_the_reference_fixture(fixture, tag, per_image):
    g = fixture
    x, t = g['logits'], g['labels']
    if tag == 'zero':
        x, t = x[:1], np.zeros_like(t[:1])
    loss, grad = lovasz_ref.lovasz_hinge_f64(x, t, per_image)
    ref_loss, ref_grad = float(g[f'{tag}_loss']), g[f'{tag}_dlogits'].astype(np.float64)
    # the stored distances were measured against this very restatement; fp32 storage of the reference's values adds 2^-24
    assert abs(loss - ref_loss) <= float(g[f'{tag}_ref_vs_f64_loss']) + 1e-7 * abs(ref_loss)
    assert np.abs(grad - ref_grad).max() <= (float(g[f'{tag}_ref_vs_f64_grad']) + 1e-7) * np.abs(grad).max()
    assert np.array_equal(grad != 0, ref_grad != 0) or tag != 'zero'


def test_all_background_image_is_the_largest_error(fixture):
    x = fixture['logits'][0]
    loss, grad = lovasz_ref.lovasz_flat_f64(x, np.zeros_like(x))
    assert loss == pytest.approx(float(np.float32(1) + x.max()), rel=1e-7)          # e = 1 + x on background
    assert np.count_nonzero(grad) == 1 and grad.reshape(-1)[np.argmax(x)] == 1.0


def test_ties_rank_by_pixel_index():
    # four equal errors, labels 1 0 0 1 in index order: G = 2, U = 2 3 4 4, I = 1 1 1 0 -> w = 1/2, 1/6, 1/12, 1/4
    x = np.array([0.5, -0.5, -0.5, 0.5], dtype=np.float32)
    t = np.array([1, 0, 0, 1])
    loss, grad = lovasz_ref.lovasz_flat_f64(x, t)
    np.testing.assert_allclose(grad, [-1 / 2, 1 / 6, 1 / 12, -1 / 4], rtol=1e-15)
    assert loss == pytest.approx(0.5 * (1 / 2 + 1 / 6 + 1 / 12 + 1 / 4), rel=1e-15)


def test_torch_form_matches_the_restatement(fixture):
    import torch
    x = torch.from_numpy(fixture['logits']).clone().requires_grad_(True)
    t = torch.from_numpy(fixture['labels'].astype(np.float32))
    for per_image in (True, False):
        loss = lovasz_ref.lovasz_hinge_torch(x, t, per_image)
        (g,) = torch.autograd.grad(loss, x)
        l64, g64 = lovasz_ref.lovasz_hinge_f64(fixture['logits'], fixture['labels'], per_image)
        assert abs(float(loss.detach()) - l64) <= 2e-7 * l64
        assert np.abs(g.numpy() - g64).max() <= 2e-7 * np.abs(g64).max()


def test_both_kinds_are_declared_at_every_layer():
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_LOVASZ_HINGE\s+4\b', header)
    assert re.search(r'#define\s+EOSVOS_LOSS_LOVASZ_HINGE_FLAT\s+5\b', header)
    assert 'loss_lovasz.py:78-111' in header
    from eosvos_amd.engine import LOSS_KINDS
    assert LOSS_KINDS['lovasz_hinge'] == 4 and LOSS_KINDS['lovasz_hinge_flat'] == 5
    assert 'lovasz' not in LOSS_KINDS                       # the reference's behaviour for unknown names stays
    assert {k: v for k, v in LOSS_KINDS.items() if v < 4} == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2,
                                                              'class_balanced_cross_entropy': 3}


def test_compute_loss_still_refuses_unknown_names():
    import torch
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError):
        compute_loss('lovasz', torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError):                       # a known name, but logits that no engine produced
        compute_loss('lovasz_hinge', torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
