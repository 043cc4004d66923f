"""Op-level fp64 parity of the tiled convolutions under every work decomposition conv_plan (csrc/conv_kernels.hip) can choose,
at maps of a few thousand pixels: the op-level entries plan under the engine's workgroup budget (Engine.set_wg_budget), so a
64- or 128-workgroup budget brings the many-tile branches within reach of small shapes, and the plan log (Engine.plan_log /
plan_log_read) says which branch a launch took -- every case ASSERTS the plan it is named for, and that the fix-up pass ran
if and only if the plan shares a tile between workgroups.

Every case runs, in each matrix mode: the forward with the whole fused epilogue (norm scale + bias + residual + ReLU) through
Engine.test_conv_algo, and the weight and data gradients (norm scale, ReLU mask bytes of the input) through
Engine.test_conv_bwd_algo.  The data gradient is the K-major twin of the forward (M = B H W, N = Cin, K = Cout k^2).  Both
entries hand the kernels NaN-filled outputs, so an element no workgroup wrote fails the comparison; masked-out elements of the
data gradient must be exactly +0.  References: tests/conv_views_ref.py in fp64 (F.conv2d on the CPU for 3x3, one matrix
product for 1x1 -- on the device for the two 32 768-pixel cases).

Cases (forward geometry B x H x W, Cin -> Cout; the plan is the FORWARD launch's unless noted; numbers as logged on the MI355X,
see profiles/conv_plan_margins.txt):

  case  budget  conv                                  logged plan                                      reaches
  r01   64      2x32x64   256->256  1x1               64 tiles, q=1, per=0, 64 wg, no fix-up           whole tiles, exact rounds
  r02   64      2x33x64   256->256  1x1               66 tiles, q=2, 33 wg, no fix-up                  q+1 on fewer workgroups
  r03   64      1x45x64   64->304   3x3               69 tiles, q=2, 35 wg (2 x 35 = 70 > 69)          `tile >= tiles -> continue`; ragged M
                                                                                                       (22.5 row tiles); 48-wide last column tile
  r04   128     2x43x64   256->384  1x1               129 tiles, 8 K steps, q=2, per=0, 65 wg          tiny-K leftover: per < 2 -> whole tiles
  r05   128     2x43x64   4128->384 1x1               129 tiles, 129 K steps, q=1, per=2, 128 wg,      whole tiles PLUS a streamed leftover; an odd
                                                      fix-up (one tile, 65 contributors)               number of K steps; long fix-up chain
  r06   64      2x24x40   128->304  1x1               45 tiles, 4 K steps, per=ksteps, nwg=tiles       one whole tile per workgroup, ragged N
  r07   64      2x23x37   64->304   3x3               42 tiles, 18 K steps, per=12, 63 wg, fix-up      stream-K runs across tile borders (12 does not
                                                                                                       divide 18); parked 128+128+48 column tiles; M = 1702
  r08   64      2x13x21   1024->48  1x1               bn=64, 5 tiles, 32 K steps, per=4, 40 wg,        EOSVOS_MINK clamp; 64-wide kernel with N < 64
                                                      fix-up                                           through the fix-up pass
  r09   64      2x20x32   128->256  3x3               f16x3: 20 tiles, splitk=3, 60 wg, fix-up;        uniform split-K, chunk-major fix-up
                                                      others: stream-K per=12, 60 wg, fix-up
  r09b  64      2x20x32   128->304  3x3               f16x3: 30 tiles, splitk=2, 60 wg; others:        split-K with a ragged last column tile
                                                      stream-K per=17, 64 wg
  r10   64      2x33x33   512->128  3x3 stride 2      DATA GRADIENT (M = 2178, N = 512, K = 1152): tap  parity-major rows, four parity classes of different
                                                      table + tile order, 72 tiles; f16x3 / bf16x6:    sizes (odd map); whole tiles dealt out longest
                                                      q=2, 64 wg, no fix-up; f32: stream-K per=12,     first
                                                      63 wg over the compacted K, fix-up
  r11   64      2x13x21   256->256  3x3 d=12 pad 12   tap table, 10 tiles of 24...72 kept K steps,     compacted K space, binary search over the prefix,
                                                      stream-K per=8, 58 wg, fix-up, no split-K        fix-up with a tap table
  r12a  0       2x128x128 2048->512 1x1               f32: 1024 tiles, deep=1, 64 K steps, q=2,        3-workgroups-per-CU variant, K step 32
                                                      512 wg; other modes: q=2, 512 wg
  r12b  0       2x128x128 2032->512 1x1               f32: deep=2, 127 K steps of 16, q=2, 512 wg      3-workgroups-per-CU variant, K step 16, K % 32 != 0

Tolerances: the project's measured bound for the tiled paths, 2e-6 (tests/test_gpu_conv_algos.py, tests/test_gpu_conv_views.py),
wherever the reduction is within what those tables cover (K <= 2304 channels x taps; weight gradients: up to 77 040 pixels) --
and, no wider, for the data gradients of r03 / r07 / r09b, which reduce over 304 x 9 = 2736.
The forwards of r05 / r12a / r12b reduce over K = 4128 / 2048 / 2032: their bound is max(2e-6, 4 x the error of a plain fp32 torch
evaluation of the same op against the same fp64 reference) -- 4 for another summation order at equal precision; the bound comes
from the reference, never from the kernel under test.
"""
import contextlib

import pytest
import torch

import conv_views_ref as R
import test_gpu_conv_views as V
from eosvos_amd.engine import Engine
from test_gpu_conv_views import DEV, FAM, MODES, WFAM, matrix_mode

pytestmark = pytest.mark.gpu
TOL = V.TOL['auto']          # 2e-6

# name: (budget, (B, H, W, Cin, Cout, k, stride, dil, pad), expected plan fields of the forward launch per mode ('*': every mode),
#        expected plan fields of the data-gradient launch per mode or None)
CASES = {
    'r01': (64, (2, 32, 64, 256, 256, 1, 1, 1, 0),
            {'*': dict(bn=128, tiles=64, ksteps=8, dp_q=1, per=0, nwg=64, splitk=0, fixup=0)}, None),
    'r02': (64, (2, 33, 64, 256, 256, 1, 1, 1, 0),
            {'*': dict(bn=128, tiles=66, ksteps=8, dp_q=2, per=0, nwg=33, splitk=0, fixup=0)}, None),
    'r03': (64, (1, 45, 64, 64, 304, 3, 1, 1, 1),
            {'*': dict(bn=128, tiles=69, ksteps=18, dp_q=2, per=0, nwg=35, splitk=0, fixup=0)}, None),
    'r04': (128, (2, 43, 64, 256, 384, 1, 1, 1, 0),
            {'*': dict(bn=128, tiles=129, ksteps=8, dp_q=2, per=0, nwg=65, splitk=0, fixup=0)}, None),
    'r05': (128, (2, 43, 64, 4128, 384, 1, 1, 1, 0),
            {'*': dict(bn=128, tiles=129, ksteps=129, dp_q=1, per=2, nwg=128, splitk=0, fixup=1)}, None),
    'r06': (64, (2, 24, 40, 128, 304, 1, 1, 1, 0),
            {'*': dict(bn=128, tiles=45, ksteps=4, dp_q=0, per=4, nwg=45, splitk=0, fixup=0)}, None),
    'r07': (64, (2, 23, 37, 64, 304, 3, 1, 1, 1),
            {'*': dict(bn=128, tiles=42, ksteps=18, dp_q=0, per=12, nwg=63, splitk=0, fixup=1)}, None),
    'r08': (64, (2, 13, 21, 1024, 48, 1, 1, 1, 0),
            {'*': dict(bn=64, tiles=5, ksteps=32, dp_q=0, per=4, nwg=40, splitk=0, fixup=1)}, None),
    'r09': (64, (2, 20, 32, 128, 256, 3, 1, 1, 1),
            {'f16x3': dict(bn=128, tiles=20, ksteps=36, dp_q=0, per=0, nwg=60, splitk=3, fixup=1),
             '*': dict(bn=128, tiles=20, ksteps=36, dp_q=0, per=12, nwg=60, splitk=0, fixup=1)}, None),
    'r09b': (64, (2, 20, 32, 128, 304, 3, 1, 1, 1),
             {'f16x3': dict(bn=128, tiles=30, ksteps=36, dp_q=0, per=0, nwg=60, splitk=2, fixup=1),
              '*': dict(bn=128, tiles=30, ksteps=36, dp_q=0, per=17, nwg=64, splitk=0, fixup=1)}, None),
    'r10': (64, (2, 33, 33, 512, 128, 3, 2, 1, 1), None,
            {'f32': dict(bn=128, tiles=72, ksteps=36, tprefix=1, torder=1, dp_q=0, per=12, nwg=63, splitk=0, fixup=1),
             '*': dict(bn=128, tiles=72, ksteps=36, tprefix=1, torder=1, dp_q=2, per=0, nwg=64, splitk=0, fixup=0)}),
    'r11': (64, (2, 13, 21, 256, 256, 3, 1, 12, 12),
            {'*': dict(bn=128, tiles=10, ksteps=72, tprefix=1, dp_q=0, per=8, nwg=58, splitk=0, fixup=1)}, None),
    'r12a': (0, (2, 128, 128, 2048, 512, 1, 1, 1, 0),
             {'f32': dict(bn=128, tiles=1024, ksteps=64, deep=1, dp_q=2, per=0, nwg=512, splitk=0, fixup=0),
              '*': dict(bn=128, tiles=1024, ksteps=64, deep=0, dp_q=2, per=0, nwg=512, splitk=0, fixup=0)}, None),
    'r12b': (0, (2, 128, 128, 2032, 512, 1, 1, 1, 0),
             {'f32': dict(bn=128, tiles=1024, ksteps=127, deep=2, dp_q=2, per=0, nwg=512, splitk=0, fixup=0),
              '*': dict(bn=128, tiles=1024, ksteps=64, deep=0, dp_q=2, per=0, nwg=512, splitk=0, fixup=0)}, None),
}
LONG_K = ('r05', 'r12a', 'r12b')          # forwards whose bound comes from the fp32 evaluation (module docstring)
ON_DEVICE = ('r12a', 'r12b')              # operands and references made on the device

_CACHE = {}


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)
    yield e
    e.close()
    _CACHE.clear()          # the device-resident references of the 32 768-pixel cases


@contextlib.contextmanager
def budget(e, workgroups):
    assert e.set_wg_budget(workgroups) == workgroups
    try:
        yield
    finally:
        e.set_wg_budget(0)          # the module's engine runs under the default budget


@contextlib.contextmanager
def plans(e, label, out):
    """The plan records of the launches inside the block, appended to `out` and printed."""
    e.plan_log(True)
    try:
        yield
        recs = e.plan_log_read()
    finally:
        e.plan_log(False)
    for p in recs:
        print(f'PLAN {label}: ' + ' '.join(f'{k}={v}' for k, v in p.items() if k != 'kernel_id'))
    out.extend(recs)


def _planned_for(workgroups):
    return workgroups if workgroups else 512


def _check_plan(p, mode, workgroups, kmajor, label):
    """What holds for every plan: the kernel of the mode and gather side, the budget the caller set, no more workgroups than
    conv_ws_floats() has slabs for (the budget; 768 for the deep variants), every tile covered, and the fix-up pass exactly when
    a tile is shared."""
    assert p['kernel'].startswith(FAM[mode] + f"{p['bn']}, " + ('true' if kmajor else 'false')), (label, p)
    assert p['kmajor'] == int(kmajor) and p['budget'] == _planned_for(workgroups), (label, p)
    assert 0 < p['nwg'] <= (768 if p['deep'] else p['budget']), (label, p)
    assert p['deep'] == 0 or (mode == 'f32' and p['bn'] == 128), (label, p)
    whole = p['dp_q'] * p['nwg']
    if p['splitk']:
        assert p['splitk'] > 1 and p['nwg'] == p['tiles'] * p['splitk'] and (p['per'], p['dp_q'], p['fixup']) == (0, 0, 1), (label, p)
    elif p['per'] == 0:
        assert whole >= p['tiles'] and p['fixup'] == 0, (label, p)
    else:
        assert whole <= p['tiles'], (label, p)
        if not p['tprefix']:
            assert p['nwg'] * p['per'] >= (p['tiles'] - whole) * p['ksteps'], (label, p)
            assert p['fixup'] == int(whole < p['tiles'] and p['per'] % p['ksteps'] != 0), (label, p)
        else:
            assert p['fixup'] == 1, (label, p)


def _expect(p, table, mode, label):
    want = table.get(mode, table['*'])
    got = {k: p[k] for k in want}
    assert got == want, (label, mode, 'planned', got, 'the case is named for', want)


def _err(got, ref):
    """max |got - ref| / max |ref| on the device the reference lives on; NaN (an unwritten element) compares false."""
    d = got.to(ref.device).double() - ref
    return float(d.abs().max() / ref.abs().max())


def _data(name):
    """Operands (on the device), fp64 references (where they were made) and the forward's bound, once per case."""
    def make():
        _, (B, H, W, Ci, Co, k, s, d, pad), _, _ = CASES[name]
        dev = DEV if name in ON_DEVICE else 'cpu'
        gen = torch.Generator(device=dev).manual_seed(1000 + sorted(CASES).index(name))
        rn = lambda *shape: torch.randn(*shape, generator=gen, device=dev)
        Ho, Wo = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
        x = torch.relu(rn(B, H, W, Ci))          # a ReLU output: its mask bytes gate the data gradient
        w = rn(Co, Ci, k, k) / (Ci * k * k) ** 0.5
        a, b = torch.rand(Co, generator=gen, device=dev) + 0.5, rn(Co) * 0.1
        res, g = rn(B, Ho, Wo, Co), rn(B, Ho, Wo, Co)
        m8 = R.relu_bytes(x)
        tol_y = TOL
        if k == 1:
            y = R.fwd_ref_mm(x, w, a, b, res=res, relu=True)
            dx, dw = R.dgrad_ref_mm(g, w, a, m8=m8), R.wgrad_ref_mm(g, x, a)
            if name in LONG_K:
                e32 = _err(R.fwd_ref_mm(x, w, a, b, res=res, relu=True, dtype=torch.float32), y)
                tol_y = max(TOL, 4.0 * e32)
                print(f'BOUND fwd {name}: fp32 evaluation {e32:.2e} -> {tol_y:.2e}')
        else:
            y = R.fwd_ref(x, w, a, b, s, d, pad, res=res, relu=True)
            dx, dw = R.dgrad_ref(g, w, a, (H, W), s, d, pad, m8=m8), R.wgrad_ref(g, x, w.shape, a, s, d, pad)
        ops = {n: t.to(DEV) for n, t in dict(x=x, w=w, a=a, b=b, res=res, g=g).items()}
        return ops, dict(y=y, dx=dx, dw=dw), R.unpack_bits(m8).to(DEV), tol_y
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def _forward(e, name, mode, label):
    """(y, plan record) of the case's forward: scale + bias + residual + ReLU."""
    _, (B, H, W, Ci, Co, k, s, d, pad), _, _ = CASES[name]
    o, ref, _, tol_y = _data(name)
    recs = []
    with matrix_mode(mode), plans(e, f'fwd {label}', recs):
        y = e.test_conv_algo('auto', o['x'], o['w'], o['a'], o['b'], o['res'], True, s, d, pad)
    assert len(recs) == 1, recs
    err = _err(y, ref['y'])
    print(f'MARGIN fwd {label}: {err:.2e}')
    assert err <= tol_y, (label, err, tol_y)
    return y, recs[0]


def _backward(e, name, mode, label):
    """(dx, dw, plan records) of the case's weight and data gradients; asserts the weight-gradient family that ran."""
    _, (B, H, W, Ci, Co, k, s, d, pad), _, _ = CASES[name]
    o, ref, M, _ = _data(name)
    recs = []
    with matrix_mode(mode), V.symbols(e, [(WFAM[mode],)], f'bwd {label}'), plans(e, f'dgrad {label}', recs):
        dx, dw = e.test_conv_bwd_algo('auto', o['x'], o['w'], o['g'], s, d, pad, scale=o['a'], mask=o['x'])
    assert not bool(torch.isnan(dw).any()), f'{label}: a weight-gradient slab that is summed was not written'
    errs = _err(dx, ref['dx']), _err(dw, ref['dw'])
    print(f'MARGIN dgrad {label}: {errs[0]:.2e}')
    print(f'MARGIN wgrad {label}: {errs[1]:.2e}')
    assert errs[0] <= TOL and errs[1] <= TOL, (label, errs)
    assert bool((V._bits(dx)[~M] == 0).all()), f'{label}: a masked-out element is not exactly +0'
    return dx, dw, recs


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_plan_case_elementwise_vs_fp64(eng, name, mode):
    wb, _, fwd_plan, dgrad_plan = CASES[name]
    label = f'{name} wb={wb} {mode}'
    with budget(eng, wb):
        _, p = _forward(eng, name, mode, label)
        _, _, recs = _backward(eng, name, mode, label)
    _check_plan(p, mode, wb, False, label)
    if fwd_plan:
        _expect(p, fwd_plan, mode, label)
    assert 1 <= len(recs) <= 2, recs          # (two: 128-wide column tiles + the <= 64-column tail launch of a 304-channel gradient)
    for q in recs:
        _check_plan(q, mode, wb, True, label)
    if dgrad_plan:
        assert len(recs) == 1
        _expect(recs[0], dgrad_plan, mode, label)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('wb', [64, 0])
@pytest.mark.parametrize('name', ['r01', 'r07', 'r09'])
def test_weight_gradient_slabs_follow_the_budget(eng, name, mode, wb):
    """The scratch engine's slabs are sized for the budget the split count is picked under: dw against fp64 under a 64-workgroup
    budget and under the whole chip, the NaN pre-fill gone (every slab that is summed was written), on the mode's own family."""
    with budget(eng, wb):
        _, _, recs = _backward(eng, name, mode, f'{name} wb={wb} {mode} (wgrad)')
    assert all(q['budget'] == _planned_for(wb) for q in recs), recs


# the plans 0 and 256 workgroups give r09 coincide but for the budget itself (both end at EOSVOS_MINK = 3 K steps per workgroup)
DIFFERENT = {'r05': [(0, 64), (0, 256), (64, 256)], 'r09': [(0, 64), (64, 256)]}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['r05', 'r09'])
def test_budget_invariance(eng, name, mode):
    """The same conv under budgets 0, 64 and 256: every result within the bound of fp64, the plans really different, and the same
    budget twice bit-identical (the fix-up pass sums its contributors in workgroup order, not in arrival order)."""
    key = lambda p: (p['dp_q'], p['per'], p['nwg'], p['splitk'], p['fixup'])
    fwd, bwd = {}, {}
    for wb in (0, 64, 256):
        with budget(eng, wb):
            runs = [(_forward(eng, name, mode, f'{name} wb={wb} {mode} #{i}'), _backward(eng, name, mode, f'{name} wb={wb} {mode} #{i}'))
                    for i in range(2)]
        (y0, p0), (dx0, dw0, r0) = runs[0]
        (y1, p1), (dx1, dw1, r1) = runs[1]
        assert V._same_bits(y0, y1) and V._same_bits(dx0, dx1) and V._same_bits(dw0, dw1), f'{name} wb={wb} {mode}: two runs differ'
        assert p0 == p1 and r0 == r1
        _check_plan(p0, mode, wb, False, f'{name} wb={wb} {mode}')
        fwd[wb], bwd[wb] = p0, r0
    assert [fwd[wb]['budget'] for wb in (0, 64, 256)] == [512, 64, 256]
    for u, v in DIFFERENT[name]:
        assert key(fwd[u]) != key(fwd[v]), (name, mode, u, v, fwd[u], fwd[v])
    assert any(fwd[wb]['fixup'] for wb in fwd) and any(q['fixup'] for wb in bwd for q in bwd[wb])


# ---- both locations of the fused epilogue, every term, through the views entry ---------------------------------------------------
# fix-up kernel: r07's forward (stream-K) and its data gradient (N = 64: split-K in f16x3, stream-K otherwise); main kernel: r03's
# forward (q + 1 whole tiles) and r02's data gradient (q + 1 whole tiles; r03's own data gradient shares its 23 tiles)
EPILOGUE = {
    'fixup': dict(fwd=('r07', 1), dgrad=('r07', 1, 32)),
    'main': dict(fwd=('r03', 0), dgrad=('r02', 0, 128)),
}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('where', sorted(EPILOGUE))
def test_epilogue_location(eng, mode, where):
    """Forward into channels [128, 128 + Cout) of a 512-wide tensor with a residual of its own pitch, writing the ReLU mask bytes
    of that slice (byte for byte R.relu_bytes of the output) and, in f16x3, the slot = bits of the written maximum; and an
    accumulating data gradient masked from channel mask_c0 on -- each once where the main kernel applies the epilogue and once
    where the fix-up kernel does (test_gpu_conv_views._run_fwd / _run_dgrad make all of these assertions)."""
    name, fixup = EPILOGUE[where]['fwd']
    wb, (B, H, W, Ci, Co, k, s, d, pad), fwd_plan, _ = CASES[name]
    recs = []
    with budget(eng, wb), plans(eng, f'epilogue fwd {name} {mode}', recs):
        V._run_fwd(eng, mode, f'plans {name}', 'auto', (B, H, W, Ci, Co, k, d, pad), 512, 128,
                   [V.tiled(mode, False, 128)] + ([V.FIXUP] if fixup else []), res_ld=512)
    assert len(recs) == 1 and recs[0]['fixup'] == fixup, recs
    _check_plan(recs[0], mode, wb, False, name)
    _expect(recs[0], fwd_plan, mode, f'epilogue fwd {name}')
    name, fixup, c0 = EPILOGUE[where]['dgrad']
    wb, geom, _, _ = CASES[name]
    bn = 64 if geom[3] <= 64 else 128
    recs = []
    with budget(eng, wb), plans(eng, f'epilogue dgrad {name} {mode}', recs):
        V._run_dgrad(eng, mode, f'plans {name}', 'auto', geom, [V.tiled(mode, True, bn)] + ([V.FIXUP] if fixup else []), accum=True,
                     mask_c0=c0)
    assert len(recs) == 1 and recs[0]['fixup'] == fixup, recs
    _check_plan(recs[0], mode, wb, True, name)
    assert (recs[0]['per'] > 0 or recs[0]['splitk'] > 1) == bool(fixup), recs
