"""Op-level fp64 parity of the convolution launches in the FORMS the network's passes use (tests/test_gpu_conv_algos.py covers
the algorithms on dense tensors only): forwards into a channel slice of a wider tensor with the epilogue writing the ReLU
mask bytes of that slice, data gradients that accumulate / add a second tensor / mask from channel 256 on, gradient operands
that are slices of a wider tensor (f16x3: under the WHOLE tensor's absmax), weight gradients of sliced operands, and the
K-concatenated ASPP data gradient -- each through the production conv_fwd / conv_dgrad / conv_wgrad / aspp_dgrad
(Engine.test_conv_views, Engine.test_aspp_dgrad) against tests/conv_views_ref.py.

Every case also asserts: nothing outside the written view changed (fp32 buffer and mask-byte buffer, bit for bit); masked-out
gradient elements are exactly +0; the mask bytes a forward wrote are the bits of ITS OWN output; the f16x3 absmax slot of the
destination holds the bit pattern of max |written value|; and the kernel symbol the case is meant for really ran
(profile_read names at most a handful of symbols per case; its buffer holds 32).

What the symbol assertions cannot tell apart: the profiler's name table has no entries for the Winograd transforms, so a
Winograd case names only its plane GEMM (`conv_h3_kernel<...>`), which a direct launch would also satisfy -- those cases stay
on the Winograd path because the entry forces the algorithm (a shape that is not eligible is an error, never a silent direct
launch), not because of the symbol; and the table files the streaming kernel's 48-column form under
`conv1x1_stream_kernel<*, 64>`, so NC = 48 is told from the tiled kernel but not from NC = 64 (N = 48 has no 64-column form).

Tolerances are those of tests/test_gpu_conv_algos.py (same measure); measured maxima: profiles/conv_views_margins.txt.
"""
import contextlib
import struct

import pytest
import torch

import conv_views_ref as R
from eosvos_amd import engine as engine_mod
from eosvos_amd.engine import Engine

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = ['f16x3', 'bf16x6', 'f32']
TOL = {'direct': 3e-6, 'wino_f2': 6e-6, 'wino_f4': 2.5e-5, 'auto': 2e-6}          # tests/test_gpu_conv_algos.py
FAM = {'f16x3': 'conv_h3_kernel<', 'bf16x6': 'conv_x6_kernel<', 'f32': 'conv_igemm_kernel<'}
WFAM = {'f16x3': 'wgrad_h3_kernel<', 'bf16x6': 'wgrad_x6_kernel<', 'f32': 'wgrad_kernel<'}
FIXUP = ('conv_fixup_kernel',)


def tiled(mode, kmajor, bn=''):
    """Substrings of the tiled kernel's symbol: column-tile width (when the case pins it) and gather side."""
    return (FAM[mode] + str(bn), ', true' if kmajor else ', false')


@pytest.fixture(scope='module')
def eng():
    e = Engine('resnet50', 96, 160, max_batch=1, device=DEV)
    yield e
    e.close()


@contextlib.contextmanager
def matrix_mode(mode):
    prev = engine_mod.get_matrix_mode()
    engine_mod.set_matrix_mode(mode)
    try:
        yield
    finally:
        engine_mod.set_matrix_mode(prev)


@contextlib.contextmanager
def symbols(e, want, label):
    """Every entry of `want` (a tuple of substrings) must match one kernel symbol launched inside the block."""
    e.profile_launches(True)
    try:
        yield
        names = e.profile_read()
    finally:
        e.profile_launches(False)
    print(f'SYMBOLS {label}: {sorted(names)}')
    for w in want:
        assert any(all(s in n for s in w) for n in names), (label, w, sorted(names))


def _maxrel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _max_bits(t):
    """Bit pattern of max |t| over the finite elements."""
    t = t[torch.isfinite(t)]
    return struct.unpack('<I', struct.pack('<f', float(t.abs().max()) if t.numel() else 0.0))[0]


def _check_slot(mode, slot, written, label, must_be_valid=False):
    bits, valid = slot
    if mode != 'f16x3':
        assert (bits, valid) == (0, False), (label, slot)
        return
    assert bits == _max_bits(written), (label, hex(bits), hex(_max_bits(written)), valid)
    if must_be_valid:
        assert valid, label


def _outside(base, off, C):
    keep = torch.ones(base.shape[-1], dtype=torch.bool, device=base.device)
    keep[off:off + C] = False
    return base[..., keep]


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- (a) forwards into slices, with mask bytes ------------------------------------------------------------------------------
def _fwd_data(label, B, H, W, Ci, Co, k, d, pad, res):
    def make():
        g = torch.Generator().manual_seed(len(label) + B + H + W + Ci + Co)
        x = torch.relu(torch.randn(B, H, W, Ci, generator=g))
        w = torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5
        a, b = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
        r = torch.randn(B, H, W, Co, generator=g) if res else None
        refs = {relu: R.fwd_ref(x, w, a, b, 1, d, pad, res=r, relu=relu) for relu in (True, False)}
        return x, w, a, b, r, refs
    return _cached(('fwd', label), make)


def _run_fwd(e, mode, label, algo, geom, ldy, off, want, relu=True, res_ld=0, dense_valid=False):
    """y = the channels [off, off + Co) of an ldy-wide buffer prefilled with noise; mask bytes for the whole buffer, prefilled 0xA5."""
    B, H, W, Ci, Co, k, d, pad = geom
    x, w, a, b, r, refs = _fwd_data(label, B, H, W, Ci, Co, k, d, pad, res_ld > 0)
    g = torch.Generator().manual_seed(1)
    base = torch.randn(B, H, W, ldy, generator=g).to(DEV)
    base0 = base.clone()
    m8 = torch.full((B, H, W, ldy // 4), 0xA5, dtype=torch.uint8, device=DEV)
    yv = base[..., off:off + Co]
    res = None
    if r is not None:
        rbuf = torch.randn(B, H, W, res_ld, generator=g).to(DEV)
        res = rbuf[..., res_ld - Co:]
        res.copy_(r.to(DEV))
    with matrix_mode(mode), symbols(e, want, f'{label} {mode}'):
        out = e.test_conv_views(algo, w.to(DEV), 1, d, pad, (B, H, W), scale=a.to(DEV), bias=b.to(DEV), x=x.to(DEV),
                                y=(yv, base) if ldy != Co else yv, res=res, relu=relu, y_m8=m8)
    err = _maxrel(yv, refs[relu])
    print(f'MARGIN fwd {label} relu={int(relu)} {mode}: {err:.2e}')
    assert err <= TOL[algo], (label, mode, err)
    assert _same_bits(_outside(base, off, Co), _outside(base0, off, Co)), f'{label}: wrote outside the view'
    q0, q1 = off // 4, (off + Co) // 4
    if relu:
        assert torch.equal(m8[..., q0:q1], R.relu_bytes(yv)), f'{label}: mask bytes are not the bits of the output'
        assert int(m8[..., q0:q1].max()) < 16
    else:
        assert bool((m8[..., q0:q1] == 0xA5).all()), f'{label}: mask bytes written without a ReLU'
    assert bool((m8[..., :q0] == 0xA5).all()) and bool((m8[..., q1:] == 0xA5).all()), f'{label}: mask bytes outside the slice'
    _check_slot(mode, out['y_slot'], yv, f'{label} {mode}', must_be_valid=dense_valid)
    return out


DEC1 = (256, 48, 1, 1, 0)          # decoder.conv1: 1x1, 256 -> 48, into channels [256, 304) of dcat


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('B', [1, 2])
def test_dec1_forward_into_the_304_wide_concat(eng, mode, B):
    """25 x 41: 1025 pixels (a ragged last row tile).  f16x3 at batch 1: the streaming kernel's 48-column form; batch 2 (2050
    pixels, below its threshold) and the other modes: the tiled 64-wide kernel.  ldy = 304 != N, bytes at + 256 / 4, pitch 76."""
    want = [('conv1x1_stream_kernel<*, 64>',)] if (mode == 'f16x3' and B == 1) else [tiled(mode, False, 64)]
    _run_fwd(eng, mode, f'dec1 B{B}', 'auto', (B, 25, 41) + DEC1, 304, 256, want)
    if B == 2:
        _run_fwd(eng, mode, f'dec1 B{B}', 'auto', (B, 25, 41) + DEC1, 304, 256, want, relu=False)


@pytest.mark.parametrize('mode', MODES)
def test_aspp_branch_forward_into_the_1280_wide_concat(eng, mode):
    """3x3, d = 6, 512 -> 256 into slice 2 of cat at 21 x 38: 14 tiles share K = 4608 between workgroups, so the fix-up pass
    writes the output AND its mask bytes (pitch 320, at + 128)."""
    _run_fwd(eng, mode, 'aspp2', 'direct', (1, 21, 38, 512, 256, 3, 6, 6), 1280, 512, [tiled(mode, False, 128), FIXUP])


@pytest.mark.parametrize('algo', ['wino_f4', 'wino_f2'])
def test_winograd_output_transform_writes_the_mask_bytes(eng, algo):
    """Bytes from the F(4,3) / F(2,3) output transform.  The transform itself is not in the profiler's name table: the symbol
    names the plane GEMM only, the forced algorithm keeps the case on the Winograd path (see the module docstring)."""
    _run_fwd(eng, 'f16x3', algo, algo, (1, 33, 57, 64, 64, 3, 1, 1), 64, 0, [tiled('f16x3', False)])


def test_conv3x3_stream_kernel_writes_the_mask_bytes(eng):
    _run_fwd(eng, 'f16x3', 's3x3', 'auto', (1, 128, 129, 64, 64, 3, 1, 1), 64, 0, [('conv3x3_stream_kernel',)], dense_valid=True)


def test_residual_with_its_own_pitch(eng):
    """layer1 conv3's epilogue (norm, residual, ReLU) with the residual a slice of a 512-wide tensor: ldres != N."""
    _run_fwd(eng, 'f16x3', 'res512', 'auto', (1, 25, 41, 64, 256, 1, 1, 0), 256, 0, [('conv1x1_stream_kernel<*, 128>',)], res_ld=512,
             dense_valid=True)


def test_slot_after_all_slices_is_the_tensor_maximum(eng):
    """Both 48-channel slices of a 96-wide tensor written by two launches of ONE absmax phase (fwd_slices = 2: launch i reads
    channels [256 i, 256 i + 256) of a 512-wide x and writes [48 i, 48 i + 48) of y): the tensor's one slot, read after the last
    launch, holds the maximum of the whole tensor, each slice matches fp64 and carries its own bytes.  Neither launch covers
    the tensor, so the entry's slot is not marked trusted (the network marks such a tensor itself once all writers ran)."""
    B, H, W, Ci, Co = 1, 25, 41, 256, 48

    def make():
        g = torch.Generator().manual_seed(77)
        x = torch.relu(torch.randn(B, H, W, 2 * Ci, generator=g))
        x[..., Ci:] *= 3.0                      # the second slice holds the tensor's maximum ...
        w = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
        a, b = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
        return x, w, a, b, [R.fwd_ref(x[..., Ci * i:Ci * i + Ci], w, a, b, 1, 1, 0, relu=True) for i in range(2)]
    x, w, a, b, refs = _cached('two slices', make)
    xb = x.to(DEV)
    base = torch.randn(B, H, W, 2 * Co, generator=torch.Generator().manual_seed(1)).to(DEV)
    m8 = torch.full((B, H, W, 2 * Co // 4), 0xA5, dtype=torch.uint8, device=DEV)
    with matrix_mode('f16x3'), symbols(eng, [('conv1x1_stream_kernel<*, 64>',)], 'two slices'):
        out = eng.test_conv_views('auto', w.to(DEV), 1, 1, 0, (B, H, W), scale=a.to(DEV), bias=b.to(DEV), x=(xb[..., :Ci], xb),
                                  y=(base[..., :Co], base), relu=True, y_m8=m8, fwd_slices=2)
        assert eng.profile_read()['conv1x1_stream_kernel<*, 64>'][0] == 2
    for i in range(2):
        err = _maxrel(base[..., Co * i:Co * i + Co], refs[i])
        print(f'MARGIN fwd two slices {i} f16x3: {err:.2e}')
        assert err <= TOL['auto'], (i, err)
    assert torch.equal(m8, R.relu_bytes(base))
    assert _max_bits(base[..., Co:]) > _max_bits(base[..., :Co])          # ... so the first launch alone would leave less
    assert out['y_slot'] == (_max_bits(base), False), out['y_slot']
    assert out['x_slot'] == (_max_bits(xb), True), out['x_slot']


# ---- (b) data gradients -----------------------------------------------------------------------------------------------------
def _dgrad_data(label, B, H, W, Ci, Co, k, s, d, pad, g_ld, g_off, mask_c0, masked, accum, add, want_dw):
    def make():
        gen = torch.Generator().manual_seed(len(label) + B + H + W + Ci + Co + g_off)
        Ho, Wo = (H + 2 * pad - d * (k - 1) - 1) // s + 1, (W + 2 * pad - d * (k - 1) - 1) // s + 1
        gbase = torch.randn(B, Ho, Wo, g_ld, generator=gen)
        w = torch.randn(Co, Ci, k, k, generator=gen) / (Co * k * k) ** 0.5
        a = torch.rand(Co, generator=gen) + 0.5
        gv = gbase[..., g_off:g_off + Co]
        core = R.dgrad_ref(gv, w, a, (H, W), s, d, pad)
        sd = float(core.std())          # initial contents / added tensor of the gradient's own magnitude
        gx0 = torch.randn(B, H, W, Ci, generator=gen) * sd
        addt = torch.randn(B, H, W, Ci, generator=gen) * sd if add else None
        m8 = torch.randint(0, 16, (B, H, W, Ci // 4), generator=gen, dtype=torch.uint8) if masked else None
        if masked and (accum or add):
            # the largest value the launch ever holds sits where the mask clears it: an absmax taken before the mask shows
            m8[-1, H // 2, W // 2, -1] &= 0xE
            (gx0 if accum else addt)[-1, H // 2, W // 2, -4] = 64.0 * sd
        ref = R.dgrad_ref(gv, w, a, (H, W), s, d, pad, gx0=gx0 if accum else None, add=addt, m8=m8, mask_c0=mask_c0)
        x = torch.relu(torch.randn(B, H, W, Ci, generator=gen)) if want_dw else None
        dw = R.wgrad_ref(gv, x, w.shape, a, s, d, pad) if want_dw else None
        return gbase, w, a, gx0, addt, m8, ref, x, dw
    return _cached(('dgrad', label, accum), make)


def _run_dgrad(e, mode, label, algo, geom, want, accum=False, masked=True, mask_c0=0, add_ld=0, g_ld=0, g_off=0, others=1.0,
               want_dw=False):
    B, H, W, Ci, Co, k, s, d, pad = geom
    g_ld = g_ld or Co
    gbase, w, a, gx0, addt, m8, ref, x, dw_ref = _dgrad_data(label, B, H, W, Ci, Co, k, s, d, pad, g_ld, g_off, mask_c0, masked,
                                                             accum, add_ld > 0, want_dw)
    gb = gbase.to(DEV)
    if others != 1.0:                    # the other channels of the tensor set its absmax, not the slice
        gv0 = gb[..., g_off:g_off + Co].clone()
        gb *= others
        gb[..., g_off:g_off + Co] = gv0
    gv = gb[..., g_off:g_off + Co]
    gx = gx0.to(DEV).clone()
    add = None
    if addt is not None:
        abuf = torch.randn(B, H, W, add_ld, generator=torch.Generator().manual_seed(2)).to(DEV)
        add = abuf[..., add_ld - Ci:]
        add.copy_(addt.to(DEV))
    m8d = m8.to(DEV) if m8 is not None else None
    with matrix_mode(mode), symbols(e, want, f'{label} {mode}'):
        out = e.test_conv_views(algo, w.to(DEV), s, d, pad, (B, H, W), scale=a.to(DEV), g=(gv, gb) if g_ld != Co else gv, gx=gx,
                                add=add, accum=accum, mask_c0=mask_c0, gx_m8=m8d, x=x.to(DEV) if want_dw else None,
                                want_dw=want_dw)
    if g_ld != Co:      # the slice really ran under the absmax of its whole tensor (the entry's seeding cannot fail silently)
        assert out['g_slot'] == ((_max_bits(gb), True) if mode == 'f16x3' else (0, False)), (label, out['g_slot'], hex(_max_bits(gb)))
        if others != 1.0:
            assert _max_bits(gb) > _max_bits(gv)
    err = _maxrel(gx, ref)
    print(f'MARGIN dgrad {label} accum={int(accum)} others={others:g} {mode}: {err:.2e}')
    assert err <= TOL[algo], (label, mode, err)
    if m8 is not None:
        M = R.unpack_bits(m8d)
        M[..., :mask_c0] = True
        assert bool((_bits(gx)[~M] == 0).all()), f'{label}: a masked-out element is not exactly +0'
    written = gx
    if s == 2:                           # the coarse-grid form touches the even pixels only
        odd = torch.ones(H, W, dtype=torch.bool, device=DEV)
        odd[::2, ::2] = False
        if accum:
            assert _same_bits(gx[:, odd], gx0.to(DEV)[:, odd]), f'{label}: an untouched pixel lost its sum'
        else:
            assert bool((_bits(gx[:, odd]) == 0).all()), f'{label}: an untouched pixel is not zero'
        written = gx[:, ::2, ::2]
    _check_slot(mode, out['gx_slot'], written, f'{label} {mode}', must_be_valid=not algo.startswith('wino'))
    if want_dw:
        werr = _maxrel(out['dw'], dw_ref)
        print(f'MARGIN wgrad {label} {mode}: {werr:.2e}')
        assert werr <= TOL[algo], (label, mode, werr)
    return gx


C1 = (256, 64, 1, 1, 1, 0)          # a bottleneck's conv1 of layer1: the data gradient contracts K = 64 into N = 256


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [(1, 25, 41), (2, 13, 21)], ids=['stream', 'tiled'])
def test_accumulating_masked_data_gradient(eng, mode, shape):
    """conv1 after the downsample conv: g_xin = M * (g_xin + dgrad).  f16x3 at batch 1, 1025 pixels: the streaming kernel's
    read-modify-write; batch 2, 546 pixels: the tiled kernel's."""
    stream = mode == 'f16x3' and shape[0] == 1
    _run_dgrad(eng, mode, f'c1 {shape}', 'auto', shape + C1, [('conv1x1_stream_kernel<*, 128>',) if stream else tiled(mode, True, 128)], accum=True)


@pytest.mark.parametrize('add_ld', [256, 512], ids=['dense', 'pitch512'])
@pytest.mark.parametrize('shape', [(1, 25, 41), (2, 13, 21)], ids=['stream', 'tiled'])
def test_data_gradient_with_a_fused_add(eng, shape, add_ld):
    """identity block: g_xin = M * (dgrad + g_out), g_out dense or a slice of a 512-wide tensor (ldres != N, k-major path)."""
    want = [('conv1x1_stream_kernel<*, 128>',) if shape[0] == 1 else tiled('f16x3', True, 128)]
    _run_dgrad(eng, 'f16x3', f'c1add {shape} {add_ld}', 'auto', shape + C1, want, add_ld=add_ld)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('plan', ['b1_1025px', 'b2_546px', 'fixup'])
def test_added_tensor_goes_in_before_the_old_contents(eng, mode, plan):
    """A data gradient with BOTH a fused add and accumulate: g_xin = M * ((dgrad + g_out) + g_xin), in that order.  The two sums
    commute up to one rounding, which no tolerance sees, so the operands are small integers and powers of two: the contraction
    is exact in every matrix mode and the result must equal the two fp32 additions bit for bit.  `b1_1025px`: the streaming
    kernel in f16x3, the tiled kernel of the mode otherwise (as `b2_546px` in every mode); `fixup`: K = 512 under a
    64-workgroup budget is streamed, the order is then the fix-up pass's."""
    B, H, W = (1, 25, 41) if plan == 'b1_1025px' else (2, 13, 21)
    Ci, Co = 256, 512 if plan == 'fixup' else 64
    gen = torch.Generator().manual_seed(Co + B)
    g = torch.randint(-2, 3, (B, H, W, Co), generator=gen).float()
    w = torch.randint(-1, 2, (Co, Ci, 1, 1), generator=gen).float()
    a = 2.0 ** torch.randint(-1, 2, (Co,), generator=gen).float()
    core = R.dgrad_ref(g, w, a, (H, W), 1, 1, 0).float()
    assert bool((core * 2 == (core * 2).round()).all()) and float(core.abs().max()) < 2 ** 14      # multiples of 1/2: exact in every mode
    sd = float(core.std())
    addt, gx0 = torch.randn(B, H, W, Ci, generator=gen) * sd, torch.randn(B, H, W, Ci, generator=gen) * sd
    m8 = torch.randint(0, 16, (B, H, W, Ci // 4), generator=gen, dtype=torch.uint8)
    M = R.unpack_bits(m8)
    want = torch.where(M, (core + addt) + gx0, torch.zeros(()))
    swapped = torch.where(M, (core + gx0) + addt, torch.zeros(()))
    assert not _same_bits(want, swapped), 'the data cannot tell the two orders apart'
    stream = plan == 'b1_1025px' and mode == 'f16x3'
    syms = [('conv1x1_stream_kernel<*, 128>',) if stream else tiled(mode, True, 128)] + ([FIXUP] if plan == 'fixup' else [])
    gx = gx0.to(DEV).clone()
    if plan == 'fixup':
        eng.set_wg_budget(64)
    eng.plan_log(True)
    try:
        with matrix_mode(mode), symbols(eng, syms, f'both {plan} {mode}'):
            eng.test_conv_views('auto', w.to(DEV), 1, 1, 0, (B, H, W), scale=a.to(DEV), g=g.to(DEV), gx=gx, add=addt.to(DEV),
                                accum=True, gx_m8=m8.to(DEV))
        logged = eng.plan_log_read()
    finally:
        eng.plan_log(False)
        if plan == 'fixup':
            eng.set_wg_budget(0)          # the module's engine runs under the default budget
    if plan == 'fixup':      # the op-level entry plans under the engine's budget: 10 tiles x 16 K steps in runs of 4 (40 workgroups under 512 too)
        assert len(logged) == 1, logged
        assert {k: logged[0][k] for k in ('budget', 'fixup', 'per', 'nwg')} == dict(budget=64, fixup=1, per=4, nwg=40), logged
    assert _same_bits(gx.cpu(), want), f'{plan} {mode}: {int((_bits(gx.cpu()) != _bits(want)).sum())} elements differ'


@pytest.mark.parametrize('accum', [False, True], ids=['zero', 'accum'])
def test_stride2_coarse_grid_scatter(eng, accum):
    """The stride-2 1x1 downsample gradient runs on the coarse grid and scatters to the even pixels: the others are zero, or
    -- accumulating -- keep their contents bit for bit."""
    _run_dgrad(eng, 'f16x3', 'ds', 'auto', (1, 25, 41, 256, 512, 1, 2, 1, 0), [tiled('f16x3', True)], accum=accum, masked=False)


@pytest.mark.parametrize('accum', [False, True], ids=['write', 'accum'])
@pytest.mark.parametrize('algo,hw', [('wino_f4', (33, 57)), ('wino_f2', (9, 11)), ('direct', (13, 21))])
def test_partial_mask_from_channel_256_of_304(eng, algo, hw, accum):
    """decoder conv on dcat: the first 256 channels carry no ReLU (their 64 mask bytes per pixel hold random bits that the
    result must ignore), the 48-column tail launch re-bases mask_c0.  One call, as in the network: weight gradient (304 dense
    input channels) first, then the data gradient.  Winograd forms: the mask and the accumulate are applied by the data-gradient
    output transform, which the profiler does not name -- the symbols are the plane GEMM's two launches (see the module docstring)."""
    want = [tiled('f16x3', True, 128), tiled('f16x3', True, 64), (WFAM['f16x3'],)]          # 2 x 128 columns + the 48-column tail
    _run_dgrad(eng, 'f16x3', f'deca {algo}', algo, (1,) + hw + (304, 256, 3, 1, 1, 1), want, accum=accum, mask_c0=256, want_dw=True)


def test_gradient_operand_is_the_48_channel_slice_of_304(eng):
    """decoder.conv1's data gradient: g = channels [256, 304) of g_dcat, ldx = 304 != Kc = 48 on the gather side."""
    _run_dgrad(eng, 'f16x3', 'dec1 dgrad', 'auto', (1, 25, 41, 256, 48, 1, 1, 1, 0), [tiled('f16x3', True)], masked=False, g_ld=304, g_off=256)


@pytest.mark.parametrize('others', [1.0, 1024.0], ids=['plain', 'others_x1024'])
def test_gradient_operand_is_a_slice_of_1280(eng, others):
    """An ASPP branch's accumulating data gradient: g = slice 1 of g_cat (Kc = 256 of 1280, 3x3, d = 6).  `others_x1024`: the
    rest of the tensor is 2^10 larger, so the slice runs 2^-10 below the absmax of its tensor -- inside the 2^-16 range that
    keeps fp32 accuracy in the f16x3 mode (include/eosvos.h); same tolerance, error against the slice's own reference.  Tiles are
    shared between workgroups: the fix-up pass does the accumulate read."""
    _run_dgrad(eng, 'f16x3', 'aspp1 dgrad', 'direct', (1, 21, 38, 512, 256, 3, 1, 6, 6), [tiled('f16x3', True, 128), FIXUP], accum=True, masked=False,
               g_ld=1280, g_off=256, others=others)


# ---- (c) weight gradients of sliced operands --------------------------------------------------------------------------------
@pytest.mark.parametrize('label,algo,geom,g_ld,g_off', [
    ('dec1 wgrad', 'auto', (1, 25, 41, 256, 48, 1, 1, 1, 0), 304, 256),               # Cout 48 from g_dcat + 256
    ('aspp3 wgrad', 'direct', (1, 21, 38, 512, 256, 3, 1, 18, 18), 1280, 768),        # Cout 256 from slice 3 of g_cat, x 512 wide
], ids=['dec1', 'aspp3'])
def test_weight_gradient_of_a_sliced_gradient(eng, label, algo, geom, g_ld, g_off):
    B, H, W, Ci, Co, k, s, d, pad = geom

    def make():
        gen = torch.Generator().manual_seed(g_off)
        gbase = torch.randn(B, H, W, g_ld, generator=gen)
        x = torch.relu(torch.randn(B, H, W, Ci, generator=gen))
        a = torch.rand(Co, generator=gen) + 0.5
        return gbase, x, a, R.wgrad_ref(gbase[..., g_off:g_off + Co], x, (Co, Ci, k, k), a, s, d, pad)
    gbase, x, a, ref = _cached(('wgrad', label), make)
    gb = gbase.to(DEV)
    w = torch.zeros(Co, Ci, k, k, device=DEV)
    with matrix_mode('f16x3'), symbols(eng, [(WFAM['f16x3'],)], label):
        out = eng.test_conv_views(algo, w, s, d, pad, (B, H, W), scale=a.to(DEV), g=(gb[..., g_off:g_off + Co], gb), x=x.to(DEV), want_dw=True)
    assert out['g_slot'] == (_max_bits(gb), True), out['g_slot']
    err = _maxrel(out['dw'], ref)
    print(f'MARGIN wgrad {label} f16x3: {err:.2e}')
    assert err <= TOL[algo], (label, err)


# ---- (d) the K-concatenated ASPP data gradient on a loaded engine ------------------------------------------------------------
ASPP_KEYS = [(f'classifier.0.convs.{i}.0', f'classifier.0.convs.{i}.1') for i in range(4)]


def _state():
    from eosvos_amd import synthetic
    return _cached('state', lambda: (synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50')))


def _aspp_engine(name):
    """One of conv_views_ref.ASPP_ENGINES (the list the host test checks the tap coverage of) with the synthetic state."""
    H, W, max_batch = R.ASPP_ENGINES[name][:3]
    sd, lrs = _state()
    e = Engine('resnet50', H, W, max_batch=max_batch, device=DEV)
    e.load_model_state(sd, lrs)
    return e


@pytest.fixture(scope='module')
def aspp_eng():
    """21 x 38 map: 798 pixels, so at batch 2 the 128-pixel tile 6 holds the end of image 0 and the start of image 1."""
    e = _aspp_engine('main')
    yield e
    e.close()


@pytest.fixture(scope='module')
def aspp_eng_low():
    """21 x 18 map, batch 2: 756 pixels, below the work threshold from which the d = 6 branch runs F(2,3) in the bf16x6 mode (where
    the merged launch declines); tile 2 holds the end of image 0 and the start of image 1."""
    e = _aspp_engine('low')
    yield e
    e.close()


@pytest.fixture(scope='module')
def aspp_eng_small():
    """21 x 22 map, batch 1: bf16x6 merged with tiles that drop the d = 6 vertical taps (no tile of the 21 x 18 map can)."""
    e = _aspp_engine('small')
    yield e
    e.close()


MAIN, LOW, SMALL = R.aspp_map('main'), R.aspp_map('low'), R.aspp_map('small')


def _aspp_data(B, h, w):
    def make():
        sd, _ = _state()
        gen = torch.Generator().manual_seed(100 * B + w)
        g_cat = torch.randn(B, h, w, 1280, generator=gen).to(DEV)
        m8 = torch.randint(0, 16, (B, h, w, 512), generator=gen, dtype=torch.uint8).to(DEV)
        ws = [sd[c + '.weight'].to(DEV) for c, _ in ASPP_KEYS]
        scales = [(sd[n + '.weight'].double() / torch.sqrt(sd[n + '.running_var'].double() + 1e-5)).to(DEV) for _, n in ASPP_KEYS]
        zero = torch.zeros(B, h, w, 2048, dtype=torch.float64, device=DEV)
        parts = [R.dgrad_taps_ref(g_cat[..., 256 * i:256 * i + 256], ws[i], scales[i], (1, 6, 12, 18)[i]) for i in range(4)]
        core = parts[0] + parts[1] + parts[2] + parts[3]
        g0 = (torch.randn(B, h, w, 2048, generator=gen) * float(core.std())).to(DEV)          # the pooling branch's broadcast
        m8[-1, h // 2, w // 2, -1] &= 0xE          # the largest value of all sits where the mask clears it (absmax taken too early)
        g0[-1, h // 2, w // 2, -4] = 64.0 * float(core.std())
        ref = (core + g0.double()) * R.unpack_bits(m8)
        # largest magnitude any of the one-by-one form's four launches writes (the first three unmasked)
        acc, stage_max = g0.double(), 0.0
        for i in range(4):
            acc = acc + parts[i]
            stage_max = max(stage_max, float((acc if i < 3 else ref).abs().max()))
        return g_cat, m8, g0, ref, stage_max
    return _cached(('aspp', B, h, w), make)


def _run_aspp(e, mode, B, hw, tol, merged, want, force_fallback=False, g_cat_scale=None, label=''):
    g_cat, m8, g0, ref, _ = _aspp_data(B, *hw)
    if g_cat_scale is not None:
        g_cat = g_cat.clone()
        g_cat[..., 1024:] *= g_cat_scale
    g_l4 = g0.clone()
    with matrix_mode(mode), symbols(e, want, f'aspp {label} B{B} {hw} {mode}'):
        ran, slot = e.test_aspp_dgrad(g_cat, m8, g_l4, force_fallback=force_fallback)
        names = e.profile_read()
    assert ran == merged, (mode, B, ran)
    assert any('multi_kernel' in n for n in names) == merged, sorted(names)
    err = _maxrel(g_l4, ref)
    print(f'MARGIN aspp dgrad {label} B{B} {hw} {mode} merged={int(ran)}: {err:.2e}')
    assert err <= tol, (mode, B, err)
    assert bool((_bits(g_l4)[~R.unpack_bits(m8)] == 0).all()), 'a masked-out element is not exactly +0'
    if mode == 'f16x3' and merged:
        _check_slot(mode, slot, g_l4, f'aspp B{B} {mode}', must_be_valid=True)
    return g_l4, slot


def test_aspp_merged_f16x3_batch_2_then_1(aspp_eng):
    """conv_h3_multi_kernel; batch 2 first, then batch 1 on the same engine (the tables are cached per batch size)."""
    for B in (2, 1):
        _run_aspp(aspp_eng, 'f16x3', B, MAIN, TOL['direct'], True, [('conv_h3_multi_kernel',), FIXUP])


def test_aspp_forced_fallback_f16x3(aspp_eng):
    """Four accumulating conv_dgrad launches, the mask applied by the last.  All four commit into the slot of g_l4 -- the first
    three their unmasked partial sums --, so the slot is the largest magnitude any of them wrote: an upper bound of max |g_l4|
    (trusted: every launch covered the tensor), equal to it only when the last launch holds the maximum."""
    g_l4, slot = _run_aspp(aspp_eng, 'f16x3', 2, MAIN, TOL['direct'], False, [tiled('f16x3', True, 128)], force_fallback=True)
    stage_max = _aspp_data(2, *MAIN)[4]
    val = struct.unpack('<f', struct.pack('<I', slot[0]))[0]
    print(f'SLOT aspp fallback: slot {val:.6e} max|g_l4| {float(g_l4.abs().max()):.6e} largest partial sum (fp64) {stage_max:.6e}')
    assert slot[1] and slot[0] >= _max_bits(g_l4)
    assert abs(val - stage_max) <= 3e-6 * stage_max, (val, stage_max)


def test_aspp_f32_runs_the_fallback(aspp_eng):
    """No K-concatenated kernel in the fp32-MFMA mode; as in bf16x6 the d = 6 branch of this size runs F(2,3)."""
    _run_aspp(aspp_eng, 'f32', 2, MAIN, TOL['wino_f2'], False, [tiled('f32', True, 128)])


def test_aspp_merged_bf16x6_batch_2_then_1(aspp_eng_low):
    """conv_x6_multi_kernel; batch 2 first (a tile across the image boundary), then batch 1 on the same engine (the per-batch
    table cache), on the 21 x 18 map that keeps the d = 6 branch off the Winograd path at batch 2."""
    for B in (2, 1):
        _run_aspp(aspp_eng_low, 'bf16x6', B, LOW, TOL['direct'], True, [('conv_x6_multi_kernel',), FIXUP])


def test_aspp_bf16x6_other_sizes(aspp_eng, aspp_eng_small):
    """bf16x6 on the 21 x 22 map at batch 1 (merged; tiles that drop the d = 6 vertical taps), and on the 21 x 38 map at batch 2,
    above the Winograd work threshold: the d = 6 branch runs F(2,3) and the four gradients accumulate one by one -- as at full
    size in this mode."""
    _run_aspp(aspp_eng_small, 'bf16x6', 1, SMALL, TOL['direct'], True, [('conv_x6_multi_kernel',), FIXUP])
    _run_aspp(aspp_eng, 'bf16x6', 2, MAIN, TOL['wino_f2'], False, [tiled('bf16x6', True, 128)])


@pytest.mark.parametrize('mode', ['f16x3', 'bf16x6'])
def test_aspp_merged_scale_edges(aspp_eng, aspp_eng_low, mode):
    """The pooling slice of g_cat (not contracted, but part of the tensor whose absmax the launch runs under) is 2^10 larger, and
    branch 2 is re-parametrised exactly: weights x 2^-9, norm scale x 2^9.  The per-segment rescale of the accumulators is an
    exact power of two (kernels.h), so g_l4 matches fp64 to the same tolerance and is bit-identical to the run with the
    original parametrisation.  Batch 2 in both modes."""
    e, B, hw = (aspp_eng, 2, MAIN) if mode == 'f16x3' else (aspp_eng_low, 2, LOW)
    sd, lrs = _state()
    sd2 = {k: v.clone() for k, v in sd.items()}
    conv, bn = ASPP_KEYS[2]
    f = 2.0 ** -9
    sd2[conv + '.weight'] *= f
    sd2[bn + '.running_mean'] *= f
    sd2[bn + '.weight'] /= f
    want = [('conv_h3_multi_kernel' if mode == 'f16x3' else 'conv_x6_multi_kernel',), FIXUP]
    try:
        plain, _ = _run_aspp(e, mode, B, hw, TOL['direct'], True, want, g_cat_scale=1024.0, label='pool x1024')
        e.load_model_state(sd2, lrs)
        repar, _ = _run_aspp(e, mode, B, hw, TOL['direct'], True, want, g_cat_scale=1024.0, label='pool x1024, branch 2 x 2^-9')
    finally:
        e.load_model_state(sd, lrs)
    assert _same_bits(plain, repar), float((plain - repar).abs().max())
