"""Host-side checks of the bootstrapped cross-entropy (no GPU): the spelled names, k, the numpy twin
(`eosvos_amd.bootstrap.loss_host`) against the plain loops of tests/bootstrap_ref.py bit for bit in everything the selection
decides (k, tau, G, T, the fp32 weights), and fraction 1.0 against the plain BCE mean."""
import os
import re

import numpy as np
import pytest

import bootstrap_ref as R
from eosvos_amd import bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = 255.0
P = 'bootstrapped_cross_entropy'


@pytest.mark.parametrize('name,want', [(P, None), (P + '_1', 0.01), (P + '_25', 0.25), (P + '_100', 1.0)])
def test_parse_accepts(name, want):
    assert bootstrap.parse(name) == (P, want)


@pytest.mark.parametrize('name', [P + '_0', P + '_101', P + '_05', P + '_2.5', P + '_', P + '25', P + '_-5', P + '_1e1'])
def test_parse_rejects_under_the_prefix(name):
    with pytest.raises(NotImplementedError):
        bootstrap.parse(name)


@pytest.mark.parametrize('name', ['bootstrapped', 'lovasz'])
def test_other_unknown_names_stay_unknown(name):
    import torch
    from eosvos_amd.engine import LOSS_KINDS, resolve_loss
    from eosvos_amd.helper_func import compute_loss
    assert bootstrap.parse(name) == (name, None) and name not in LOSS_KINDS
    with pytest.raises(KeyError):
        resolve_loss(name)
    with pytest.raises(NotImplementedError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_the_kind_is_declared_at_every_layer():
    from eosvos_amd import _ffi
    from eosvos_amd.engine import LOSS_KINDS, resolve_loss
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_BOOTSTRAPPED_BCE\s+6\b', header)
    assert re.search(r'int\s+eosvos_set_loss_bootstrap\(eosvos_engine\*\s*e,\s*float\s+fraction\)', header)
    assert LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                          'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, P: 6}
    assert 'eosvos_set_loss_bootstrap' in open(_ffi.__file__).read()
    assert resolve_loss(P) == (6, None) and resolve_loss(P + '_10') == (6, pytest.approx(0.1))
    assert resolve_loss(P, 0.5) == (6, 0.5) and resolve_loss(P + '_50', 0.5) == (6, 0.5)
    assert resolve_loss('dice') == (1, None)


def test_compute_loss_names_and_keyword():
    import torch
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(NotImplementedError):
        compute_loss('lovasz', z, z)
    with pytest.raises(NotImplementedError):
        compute_loss(P + '_0', z, z)
    with pytest.raises(ValueError):                         # suffix and keyword disagree
        compute_loss(P + '_10', z, z, {'fraction': 0.25})
    with pytest.raises(ValueError):                         # out of (0, 1]
        compute_loss(P, z, z, {'fraction': 0.0})
    with pytest.raises(ValueError):                         # the keyword belongs to this kind alone
        compute_loss('dice', z, z, {'fraction': 0.25})
    for kw in (None, {'fraction': 0.1}, {'fraction': 0.25}):    # known spellings, but logits that no engine produced
        with pytest.raises(RuntimeError):
            compute_loss(P + ('_25' if kw and kw['fraction'] == 0.25 else ''), z, z, kw)


def test_k_of():
    assert bootstrap.k_of(1, 0.25) == 1 and bootstrap.k_of(1, 1.0) == 1 and bootstrap.k_of(0, 0.25) == 0
    for n in (1, 7, 32767, 32768, 10 ** 6):
        assert bootstrap.k_of(n, 1.0) == n
    assert bootstrap.k_of(32767, 1 / 65536) == 1            # (32767 + 32768) >> 16 = 0 -> the floor of 1
    assert bootstrap.k_of(32768, 1 / 65536) == 1            # the first n that rounds up to 1 by itself
    assert bootstrap.k_of(98303, 1 / 65536) == 1 and bootstrap.k_of(98304, 1 / 65536) == 2      # n q + 32768 crossing 2 * 2^16
    assert bootstrap.k_of(6, 0.25) == 2 and bootstrap.k_of(5, 0.25) == 1                        # 6/4 = 1.5 rounds up, 5/4 down
    assert bootstrap.q_of(0.25) == 16384 and bootstrap.q_of(1.0) == 65536 and bootstrap.q_of(1e-9) == 1
    assert bootstrap.q_of(0.1) == 6554                      # fp32 0.1 * 65536 = 6553.6
    assert bootstrap.k_of(2 ** 31 - 1, 1.0) == 2 ** 31 - 1  # 64-bit product
    for n in (1, 2, 255, 4097, 409920):
        for f in (1 / 65536, 0.1, 0.25, 0.5, 1.0):
            assert bootstrap.k_of(n, f) == R.k_of(n, f)
    for bad in (0.0, -0.25, 1.0001, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            bootstrap.k_of(10, bad)


def void_of(n, pattern, rng):
    v = np.zeros(n, dtype=bool)
    if pattern == 'all':
        v[:] = True
    elif pattern == 'random':
        v = rng.rand(n) < 0.3
    elif pattern == 'last_valid':
        v[:-1] = True
    return v


def keys_case(name, n, rng):
    """Logits whose keys (targets 0: key = logit) form the named pattern."""
    if name == 'random':
        return (3 * rng.randn(n)).astype(np.float32)
    if name == 'all_equal':
        return np.full(n, 0.75, dtype=np.float32)
    if name == 'ties_straddle':                            # few distinct values: the threshold falls inside a run of ties
        return rng.randint(0, 4, n).astype(np.float32) - 1.5
    if name == 'last_bit':                                 # 1 + i * 2^-23
        return (np.float32(1) + (np.arange(n) % 64).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    if name == 'signs_and_zeros':
        return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0, -1e-30, 1e-30], dtype=np.float32), n)
    if name == 'denormals':
        return (rng.randint(-5, 6, n).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    raise KeyError(name)


@pytest.mark.parametrize('pattern', ['none', 'all', 'random', 'last_valid'])
@pytest.mark.parametrize('fraction', [1 / 65536, 0.1, 0.25, 1.0])
@pytest.mark.parametrize('name', ['random', 'all_equal', 'ties_straddle', 'last_bit', 'signs_and_zeros', 'denormals'])
def test_twin_equals_the_plain_loops(name, fraction, pattern):
    n = 257
    rng = np.random.RandomState(len(name) + int(fraction * 1000) + len(pattern))
    x = keys_case(name, n, rng)
    t = (rng.rand(n) < 0.4).astype(np.float32) if name in ('random', 'signs_and_zeros') else np.zeros(n, dtype=np.float32)
    void = void_of(n, pattern, rng)
    t[void] = IGN
    ign = None if pattern == 'none' else IGN
    ref = R.one_set(x, t, fraction, ign)
    loss, grad, w, ks = bootstrap.loss_host(x, t, fraction, ignore=ign)
    assert ks == [ref['k']]
    valid = ~void if ign is not None else np.ones(n, dtype=bool)
    tau, G, T, r, w2 = bootstrap.select(bootstrap.keys_of(x, t), valid, ref['k'])
    assert (tau, G, T, r) == (ref['tau'], ref['G'], ref['T'], ref['r'])
    assert np.array_equal(w.view(np.uint32), ref['weights'].view(np.uint32)) and np.array_equal(w, w2)
    if ref['k']:
        assert 1 <= r <= T and abs(float(w.astype(np.float64).sum()) - ref['k']) <= 1e-4 * ref['k']
    assert loss == pytest.approx(ref['loss'], rel=1e-12, abs=1e-300)
    np.testing.assert_allclose(grad, ref['grad'], rtol=1e-12, atol=0)
    assert not grad[w == 0].any() and not np.signbit(grad[w == 0]).any()
    if pattern == 'all':
        assert loss == 0 and ks == [0] and not w.any()


def test_the_words_order_like_the_floats():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-45, 1e-40, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.inf,
                  np.nan], dtype=np.float32)
    u = bootstrap.orderable(v)
    assert [int(a) for a in u] == [R.word(a) for a in v]
    assert u[3] == u[4] and int(u[-1]) == 0xFFFFFFFF
    assert all(int(a) < int(b) for a, b in zip(np.delete(u, 3)[:-1], np.delete(u, 3)[1:]))


def test_a_nan_logit_on_a_valid_pixel_is_selected():
    x = np.array([0.1, np.nan, -2.0, 0.3] * 8, dtype=np.float32)
    t = np.zeros(32, dtype=np.float32)
    loss, _, w, _ = bootstrap.loss_host(x, t, 0.25)
    assert np.isnan(loss) and (w[1::4] == 1).all()
    t[1::4] = IGN
    loss, grad, w, _ = bootstrap.loss_host(x, t, 0.25, ignore=IGN)
    assert np.isfinite(loss) and np.isfinite(grad).all() and not w[1::4].any()


def test_fraction_one_is_the_bce_mean():
    rng = np.random.RandomState(3)
    x = (3 * rng.randn(3, 500)).astype(np.float32)
    t = (rng.rand(3, 500) < 0.3).astype(np.float32)
    loss, grad, w, ks = bootstrap.loss_host(x, t, 1.0)
    x64, t64 = x.astype(np.float64), t.astype(np.float64)
    bce = np.maximum(x64, 0) - x64 * t64 + np.log1p(np.exp(-np.abs(x64)))
    assert ks == [500] * 3 and (w == 1).all()
    assert loss == pytest.approx(bce.mean(), rel=1e-13)
    np.testing.assert_allclose(grad, (1 / (1 + np.exp(-x64)) - t64) / 1500, rtol=1e-12, atol=1e-18)


def test_batch_is_the_mean_of_the_sets_with_an_all_void_image():
    rng = np.random.RandomState(4)
    x = (3 * rng.randn(3, 300)).astype(np.float32)
    t = (rng.rand(3, 300) < 0.3).astype(np.float32)
    t[1] = IGN
    t[0, :100] = IGN
    loss, grad, w, ks = bootstrap.loss_host(x, t, 0.25, ignore=IGN)
    assert ks == [50, 0, 75]
    per = [R.one_set(x[s], t[s], 0.25, IGN) for s in range(3)]
    assert loss == pytest.approx(sum(p['loss'] for p in per) / 3, rel=1e-12)
    np.testing.assert_allclose(grad, np.stack([p['grad'] for p in per]) / 3, rtol=1e-12, atol=0)
    assert not grad[1].any() and not w[1].any()
