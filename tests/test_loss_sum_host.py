"""Host-side checks of the weighted loss sums (no GPU): the grammar of `eosvos_amd.loss_sum.parse`, what is refused and how,
the keyword rules, the numpy twin `combine_host` against the two-rounding rule of include/eosvos.h written out here (and
against a fused multiply-add, which it must NOT equal), and the declarations at every layer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from eosvos_amd import loss_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W03 = float(np.float32(0.3))


# ---- the spelling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,want', [
    ('lovasz_hinge+boundary_f', [(1.0, 'lovasz_hinge'), (1.0, 'boundary_f')]),
    ('0.5*lovasz_hinge+boundary_f_4', [(0.5, 'lovasz_hinge'), (1.0, 'boundary_f_4')]),
    ('cross_entropy+0.3*dice', [(1.0, 'cross_entropy'), (W03, 'dice')]),
    ('2*dice', [(2.0, 'dice')]),
    ('dice', [(1.0, 'dice')]),
    ('0.25*bootstrapped_cross_entropy_10+3*class_balanced_cross_entropy+lovasz_hinge_flat+10.5*cross_entropy_and_boundary_f_16',
     [(0.25, 'bootstrapped_cross_entropy_10'), (3.0, 'class_balanced_cross_entropy'), (1.0, 'lovasz_hinge_flat'),
      (10.5, 'cross_entropy_and_boundary_f_16')])])
def test_parse_accepts(name, want):
    assert loss_sum.parse(name) == want
    assert loss_sum.is_sum(name) == ('+' in name or '*' in name)


def test_the_weight_is_the_fp32_nearest_to_the_literal():
    for lit in ('0.3', '0.1', '0.7', '1.1', '123.456', '0.000001', '16777217', '0.30000001192092896'):
        (w, _), = loss_sum.parse(lit + '*dice')
        assert w == float(np.float32(w)) and w > 0                          # an fp32 value
        from fractions import Fraction
        exact, f = Fraction(lit), np.float32(w)
        for other in (np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))):
            assert abs(Fraction(float(f)) - exact) <= abs(Fraction(float(other)) - exact), lit


MALFORMED = ['', '+', 'dice+', '+dice', 'dice++cross_entropy',                               # an empty term
             '*dice', 'cross_entropy+*dice', 'dice*', 'dice*2',                              # '*' without a weight / a name
             '0*dice', '0.0*dice', '0.000*dice+cross_entropy',                               # a weight of 0
             '1e1*dice', '1E1*dice', '-1*dice', '+1*dice', '.5*dice', '1.*dice', '1.5.2*dice', '0x2*dice', 'inf*dice',
             'nan*dice', '2*3*dice', '1' + '0' * 40 + '*dice', '0.' + '0' * 60 + '1*dice',      # no fp32 > 0 and finite
             'cross_entropy+dice+lovasz_hinge+boundary_f+bootstrapped_cross_entropy',           # a fifth term
             'dice + cross_entropy', ' dice+cross_entropy', 'dice+cross_entropy ', '0.5 *dice', '0.5*\tdice', 'dice+\ncross_entropy',
             'lovasz+dice', 'dice+boundary', '2*bootstrapped', 'dice+unknown', '0.5*7',       # an unknown term name
             'dice+boundary_f_17', 'boundary_f_0+dice', 'dice+boundary_f_2.5', 'dice+cross_entropy_and_boundary_f_03',
             '2*bootstrapped_cross_entropy_0', 'dice+bootstrapped_cross_entropy_101', 'dice+bootstrapped_cross_entropy_1e1']


@pytest.mark.parametrize('name', MALFORMED)
def test_malformed_is_not_implemented_everywhere(name):
    from eosvos_amd.helper_func import compute_loss
    with pytest.raises(NotImplementedError) as err:
        loss_sum.parse(name)
    assert str(err.value) == f"loss_func='{name}'"
    with pytest.raises(NotImplementedError):
        loss_sum.resolve(name)
    if loss_sum.is_sum(name):                     # (a name without '+' or '*' is not a sum: it goes where it goes today)
        with pytest.raises(NotImplementedError):
            compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_parse_refuses_what_is_no_string():
    for name in (None, 3, 2.5, ['dice'], b'dice+cross_entropy'):
        with pytest.raises(NotImplementedError):
            loss_sum.parse(name)
        assert not loss_sum.is_sum(name)


@pytest.mark.parametrize('name', ['dice+dice', '2*dice+0.5*dice', 'lovasz_hinge+dice+lovasz_hinge',
                                  'boundary_f_2+boundary_f_3', 'bootstrapped_cross_entropy_10+bootstrapped_cross_entropy_20',
                                  'boundary_f+cross_entropy_and_boundary_f', 'cross_entropy_and_boundary_f_2+dice+boundary_f_2'])
def test_duplicates_and_both_boundary_kinds_are_value_errors(name):
    from eosvos_amd.helper_func import compute_loss
    assert loss_sum.parse(name)                          # the grammar is fine
    with pytest.raises(ValueError):
        loss_sum.resolve(name)
    with pytest.raises(ValueError):
        compute_loss(name, torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_resolve():
    kinds, weights, names, f, r = loss_sum.resolve('0.5*lovasz_hinge+boundary_f_4')
    assert (kinds, weights, names, f, r) == ([4, 8], [0.5, 1.0], ['lovasz_hinge', 'boundary_f_4'], None, 4)
    kinds, weights, names, f, r = loss_sum.resolve('class_balanced_cross_entropy+0.3*bootstrapped_cross_entropy_25+lovasz_hinge_flat')
    assert (kinds, weights, f, r) == ([3, 6, 5], [1.0, W03, 1.0], 0.25, None)
    assert loss_sum.resolve('2*dice') == ([1], [2.0], ['dice'], None, None)
    assert loss_sum.resolve('dice') == ([1], [1.0], ['dice'], None, None)
    kinds = loss_sum.resolve('0.7*cross_entropy_and_dice+0.3*dice+0.6*lovasz_hinge+0.9*cross_entropy_and_boundary_f_3')[0]
    assert kinds == [2, 1, 4, 9]


def test_the_keyword_rules():
    from eosvos_amd.helper_func import compute_loss
    z = torch.zeros(1, 1, 4, 4)
    # the keyword goes to the one term of its family
    assert loss_sum.resolve('dice+boundary_f', radius=3)[3:] == (None, 3)
    assert loss_sum.resolve('dice+boundary_f_3', radius=3)[3:] == (None, 3)
    assert loss_sum.resolve('0.5*bootstrapped_cross_entropy+dice', fraction=0.5)[3:] == (0.5, None)
    assert loss_sum.resolve('bootstrapped_cross_entropy_50+cross_entropy_and_boundary_f', 0.5, 2)[3:] == (0.5, 2)
    for name, kw in (('dice+cross_entropy', {'radius': 3}), ('lovasz_hinge+0.3*bootstrapped_cross_entropy', {'radius': 3}),
                     ('dice+boundary_f', {'fraction': 0.5}), ('2*dice', {'fraction': 0.5}), ('2*dice', {'radius': 2})):
        with pytest.raises(ValueError):                      # no term of that family
            loss_sum.resolve(name, **kw)
        with pytest.raises(ValueError):
            compute_loss(name, z, z, kw)
    for name, kw in (('dice+boundary_f_3', {'radius': 2}), ('0.5*cross_entropy_and_boundary_f_16+dice', {'radius': 8}),
                     ('dice+bootstrapped_cross_entropy_10', {'fraction': 0.5})):
        with pytest.raises(ValueError):                      # the suffix disagrees
            loss_sum.resolve(name, **kw)
        with pytest.raises(ValueError):
            compute_loss(name, z, z, kw)
    for kw in ({'radius': 0}, {'radius': 17}, {'radius': 2.5}, {'fraction': 0.0}, {'fraction': 1.5}):
        with pytest.raises(ValueError):                      # out of range, as for a single kind
            loss_sum.resolve('dice+boundary_f+bootstrapped_cross_entropy', **kw)
    # per_image: False turns a lovasz_hinge term into the flat kind
    assert loss_sum.resolve('0.5*lovasz_hinge+dice', per_image=False)[:3] == ([5, 1], [0.5, 1.0], ['lovasz_hinge_flat', 'dice'])
    assert loss_sum.flat_spelling('0.5*lovasz_hinge+dice+2*lovasz_hinge_flat') == '0.5*lovasz_hinge_flat+dice+2*lovasz_hinge_flat'
    with pytest.raises(ValueError):                          # ... which may then be there twice
        loss_sum.resolve('lovasz_hinge+lovasz_hinge_flat', per_image=False)
    with pytest.raises(NotImplementedError):                 # as today for the single kind
        compute_loss('dice+0.5*class_balanced_cross_entropy', z, z, {'size_average': False})
    for name, kw in (('0.5*lovasz_hinge+boundary_f_4', None), ('dice+boundary_f', {'radius': 3}), ('2*dice', None),
                     ('dice+0.5*class_balanced_cross_entropy', {'ignore': 255})):
        with pytest.raises(RuntimeError):                    # known spellings, but logits that no engine produced
            compute_loss(name, z, z, kw)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
def test_combine_host_is_the_two_rounding_rule_and_not_a_fused_multiply_add():
    rng = np.random.RandomState(0)
    g = [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]
    v = [np.float32(0.71), np.float32(1.37), np.float32(0.11)]
    w = [1.0, 0.3, 0.7]
    loss, grad = loss_sum.combine_host(v, g, w)
    w32 = [np.float32(x) for x in w]
    # every product rounded to fp32, then every sum rounded to fp32: through float64, where both are exact before the rounding
    want = (np.float64(w32[0]) * g[0].astype(np.float64)).astype(np.float32)
    for i in (1, 2):
        prod = (np.float64(w32[i]) * g[i].astype(np.float64)).astype(np.float32)
        want = (want.astype(np.float64) + prod.astype(np.float64)).astype(np.float32)
    assert grad.dtype == np.float32 and np.array_equal(grad.view(np.uint32), want.view(np.uint32))
    want_loss = np.float32(np.float32(np.float32(w32[0] * v[0]) + np.float32(w32[1] * v[1])) + np.float32(w32[2] * v[2]))
    assert loss.dtype == np.float32 and loss.view(np.uint32) == want_loss.view(np.uint32)
    # two terms against the contracted form a + w * b with one rounding (exact in float64: 24 + 24 bits, exponents close)
    _, two = loss_sum.combine_host(v[:2], g[:2], w[:2])
    fma = (g[0].astype(np.float64) + np.float64(w32[1]) * g[1].astype(np.float64)).astype(np.float32)
    differs = int((two.view(np.uint32) != fma.view(np.uint32)).sum())
    assert differs >= 1, 'a weight of 0.3 must tell a contracted kernel from the rule'
    # ... which powers of two cannot
    _, pow2 = loss_sum.combine_host(v[:2], g[:2], [1.0, 0.5])
    assert np.array_equal(pow2, (g[0].astype(np.float64) + 0.5 * g[1].astype(np.float64)).astype(np.float32))


def test_combine_host_edge_values():
    z = np.zeros(4, np.float32)
    _, grad = loss_sum.combine_host([0.0, 0.0], [z, z], [0.3, 0.7])
    assert np.array_equal(grad.view(np.uint32), np.zeros(4, np.uint32))           # void pixels keep +0
    loss, _ = loss_sum.combine_host([1.0, float('nan'), 2.0], None, [1.0, 0.3, 2.0])
    assert np.isnan(loss)
    loss, grad = loss_sum.combine_host([3.0], [np.float32([1.5, -2.0])], [2.0])
    assert float(loss) == 6.0 and grad.tolist() == [3.0, -4.0]
    loss, grad = loss_sum.combine_host([0.3], [np.float32([0.1])], [1.0])           # one term of weight 1: the term's bits
    assert loss == np.float32(0.3) and grad[0] == np.float32(0.1)


# ---- what has not changed ------------------------------------------------------------------------------------------------
def test_plain_names_resolve_as_before():
    from eosvos_amd import bootstrap, boundary
    from eosvos_amd.engine import LOSS_KINDS, resolve_loss
    assert LOSS_KINDS == {'cross_entropy': 0, 'dice': 1, 'cross_entropy_and_dice': 2, 'class_balanced_cross_entropy': 3,
                          'lovasz_hinge': 4, 'lovasz_hinge_flat': 5, 'bootstrapped_cross_entropy': 6}      # seven entries
    assert boundary.KINDS == {'boundary_f': 8, 'cross_entropy_and_boundary_f': 9}
    with pytest.raises(KeyError):
        resolve_loss('lovasz')
    with pytest.raises(KeyError):
        resolve_loss('dice+cross_entropy')                   # the single-name resolver does not learn sums
    assert resolve_loss('dice') == (1, None) and resolve_loss('boundary_f_8') == (8, None)
    assert bootstrap.parse('dice+bootstrapped_cross_entropy_10') == ('dice+bootstrapped_cross_entropy_10', None)
    assert not loss_sum.is_sum('cross_entropy_and_dice') and not loss_sum.is_sum('bootstrapped_cross_entropy_10')


def test_declared_at_every_layer():
    from eosvos_amd import _ffi
    header = open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert re.search(r'#define\s+EOSVOS_LOSS_MAX_TERMS\s+4\b', header) and loss_sum.MAX_TERMS == 4
    assert not re.search(r'#define\s+EOSVOS_LOSS_\w+\s+7\b', header)          # kind 7 stays unassigned
    for name in ('eosvos_set_loss_sum', 'eosvos_loss_sum', 'eosvos_loss_sum_tensors', 'eosvos_last_loss_terms'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _ffi._SIGNATURES, name
    assert len(_ffi._SIGNATURES['eosvos_loss_sum_tensors'][1]) == 11 and len(_ffi._SIGNATURES['eosvos_loss_sum'][1]) == 9
    kernels = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'misc_kernels.hip')).read()
    assert 'loss_sum_kernel' in kernels and 'launch_loss_sum' in kernels
    engine_cpp = open(os.path.join(ROOT, 'e-osvos_amd', 'csrc', 'engine.cpp')).read()
    assert 'launch_loss_sum' in engine_cpp and 'EOSVOS_LOSS_MAX_TERMS' in engine_cpp


def test_the_module_imports_without_torch():
    code = ('import sys; sys.modules["torch"] = None\n'
            'from eosvos_amd import loss_sum\n'
            'import numpy as np\n'
            'assert loss_sum.combine_host([1.0, 2.0], None, [1.0, 0.5])[0] == np.float32(2.0)\n'
            'assert loss_sum.is_sum("dice+cross_entropy")\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    subprocess.run([sys.executable, '-c', code], check=True, env=env, cwd=ROOT)


def test_the_sum_survives_the_command_line():
    from eosvos_amd import config
    spelled = '0.5*lovasz_hinge+boundary_f_4'
    found = []

    def walk(x):
        if isinstance(x, dict):
            for k, v in x.items():
                if k == 'loss_func':
                    found.append(v)
                walk(v)
    walk(config.parse_cli(['with', f'loss_func={spelled}']))
    assert found and all(v == spelled for v in found), found
