"""CPU checks of tests/conv_views_ref.py: the composed forms the engine's backward pass launches (accumulating, adding and
partially masked data gradients; the K-concatenated ASPP gradient) against autograd through explicit torch.nn modules, the
mask-byte packing, and the tap-coverage condition the GPU test's ASPP map sizes must meet."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_views_ref as R

TOL = 1e-11          # both sides are fp64; they differ by the order of a few hundred additions


def _bn(c, g):
    m = nn.BatchNorm2d(c).double().eval()
    with torch.no_grad():
        m.weight.copy_(torch.rand(c, generator=g) + 0.5)
        m.bias.copy_(torch.randn(c, generator=g) * 0.1)
        m.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return m


def _fold(bn):
    return (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach()


def _conv(ci, co, k, g, stride=1, dil=1):
    m = nn.Conv2d(ci, co, k, stride, dil * (k // 2), dil, bias=False).double()
    with torch.no_grad():
        m.weight.copy_(torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5)
    return m


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def test_mask_bytes_round_trip_and_ignore_the_high_bits():
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 3, 5, 48, generator=g)
    y[y.abs() < 0.3] = 0.0                    # exact zeros and negative zero are not > 0
    y[0, 0, 0, 0] = -0.0
    b = R.relu_bytes(y)
    assert b.dtype == torch.uint8 and b.shape == (2, 3, 5, 12) and int(b.max()) < 16
    assert torch.equal(R.unpack_bits(b), y > 0)
    assert torch.equal(R.unpack_bits(b | 0xA0), y > 0)
    # byte q, bit j <-> channel 4q + j
    one = torch.zeros(1, 1, 1, 16)
    one[..., 9] = 1.0
    assert R.relu_bytes(one).flatten().tolist() == [0, 0, 2, 0]


def test_matrix_product_forms_of_the_1x1_references_are_the_conv_forms():
    """fwd_ref_mm / dgrad_ref_mm / wgrad_ref_mm (tests/test_gpu_conv_plans.py: long reductions) against the convolution forms."""
    g = torch.Generator().manual_seed(5)
    B, H, W, Ci, Co = 2, 5, 7, 24, 16
    x = torch.relu(torch.randn(B, H, W, Ci, generator=g))
    w = torch.randn(Co, Ci, 1, 1, generator=g)
    a, b = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g)
    res, gy = torch.randn(B, H, W, Co, generator=g), torch.randn(B, H, W, Co, generator=g)
    m8 = R.relu_bytes(x)
    for relu in (False, True):
        assert _rel(R.fwd_ref_mm(x, w, a, b, res=res, relu=relu), R.fwd_ref(x, w, a, b, 1, 1, 0, res=res, relu=relu)) < 1e-14
    ref = R.dgrad_ref(gy, w, a, (H, W), 1, 1, 0, m8=m8, mask_c0=8)
    got = R.dgrad_ref_mm(gy, w, a, m8=m8, mask_c0=8)
    assert _rel(got, ref) < 1e-14 and torch.equal(got == 0, ref == 0)
    assert _rel(R.wgrad_ref_mm(gy, x, a), R.wgrad_ref(gy, x, w.shape, a, 1, 1, 0)) < 1e-14
    f32 = R.fwd_ref_mm(x, w, a, b, res=res, relu=True, dtype=torch.float32)
    assert f32.dtype == torch.float32 and 0 < _rel(f32.double(), R.fwd_ref_mm(x, w, a, b, res=res, relu=True)) < 1e-5


@pytest.mark.parametrize('downsample', [False, True], ids=['identity', 'downsample'])
def test_bottleneck_input_gradient_is_the_engines_composition(downsample):
    """torchvision Bottleneck (stride on conv2).  Identity block: g_xin = M * (g_out + dgrad_conv1(a1 * g_t1)) -- the fused-add
    form; downsample block: dgrad_ds(a_d * g_out) first, then conv1's gradient ACCUMULATES into it and applies the mask."""
    g = torch.Generator().manual_seed(3 + downsample)
    cin, mid, cout, s = (16, 8, 32, 2) if downsample else (32, 8, 32, 1)
    B, H, W = 2, 7, 9
    c1, c2, c3 = _conv(cin, mid, 1, g), _conv(mid, mid, 3, g, stride=s), _conv(mid, cout, 1, g)
    b1, b2, b3 = _bn(mid, g), _bn(mid, g), _bn(cout, g)
    cd, bd = (_conv(cin, cout, 1, g, stride=s), _bn(cout, g)) if downsample else (None, None)
    z = torch.randn(B, cin, H, W, generator=g).double().requires_grad_(True)          # pre-ReLU output of the previous block
    xin = F.relu(z)
    t1 = b1(c1(xin)); t1.retain_grad()
    t2 = b2(c2(F.relu(t1)))
    skip = bd(cd(xin)) if downsample else xin
    out = b3(c3(F.relu(t2))) + skip; out.retain_grad()
    (F.relu(out) * torch.randn(out.shape, generator=g).double()).sum().backward()
    m8 = R.pack_bits(R.nhwc(z.detach()) > 0)
    g_t1, g_out = R.nhwc(t1.grad), R.nhwc(out.grad)
    if downsample:
        gx0 = R.dgrad_ref(g_out, cd.weight.detach(), _fold(bd), (H, W), s, 1, 0)
        # the coarse-grid form: only the even pixels of the finer grid receive a contribution
        assert float(gx0[:, 1::2].abs().max()) == 0.0 and float(gx0[:, :, 1::2].abs().max()) == 0.0
        gx = R.dgrad_ref(g_t1, c1.weight.detach(), _fold(b1), (H, W), 1, 1, 0, gx0=gx0, m8=m8)
    else:
        gx = R.dgrad_ref(g_t1, c1.weight.detach(), _fold(b1), (H, W), 1, 1, 0, add=g_out, m8=m8)
    assert _rel(gx, R.nhwc(z.grad)) < TOL
    assert bool((gx[~R.unpack_bits(m8)] == 0).all())
    # the weight gradient of conv1 in the same convention
    dw = R.wgrad_ref(g_t1, R.nhwc(xin.detach()), c1.weight.shape, _fold(b1), 1, 1, 0)
    assert _rel(dw, c1.weight.grad) < TOL


def test_aspp_input_gradient_is_the_sum_of_the_branch_gradients():
    """Four parallel dilated convs on relu(z), each with norm + ReLU, concatenated (1024 of the 1280 channels; the last 256
    belong to the pooling branch, whose gradient reaches z by another route: g_l4_0)."""
    g = torch.Generator().manual_seed(11)
    B, H, W, cin, dils = 2, 9, 11, 8, (1, 2, 3, 4)
    convs = [_conv(cin, 256, 1 if i == 0 else 3, g, dil=d) for i, d in enumerate(dils)]
    bns = [_bn(256, g) for _ in dils]
    z = torch.randn(B, cin, H, W, generator=g).double().requires_grad_(True)
    l4 = F.relu(z)
    pre = [bn(c(l4)) for c, bn in zip(convs, bns)]
    for p in pre:
        p.retain_grad()
    cat = torch.cat([F.relu(p) for p in pre], 1)
    q = torch.randn(B, cin, H, W, generator=g).double()
    ((cat * torch.randn(cat.shape, generator=g).double()).sum() + (l4 * q).sum()).backward()
    g_cat = torch.randn(B, H, W, 1280, generator=g).double()          # the pooling slice holds anything: it is not contracted
    for i, p in enumerate(pre):
        g_cat[..., 256 * i:256 * i + 256] = R.nhwc(p.grad)
    m8 = R.pack_bits(R.nhwc(z.detach()) > 0)
    ref = R.aspp_dgrad_ref(g_cat, [c.weight.detach() for c in convs], [_fold(b) for b in bns], R.nhwc(q), m8, dils=dils)
    assert _rel(ref, R.nhwc(z.grad)) < TOL


def test_partial_mask_of_the_decoder_concat():
    """dcat = concat(u, relu(z_low)): channels [0, 256) carry no ReLU, so the gradient of the 3x3 conv on dcat is masked from
    mask_c0 = 256 on only, whatever bits the first 64 bytes of a pixel hold."""
    g = torch.Generator().manual_seed(5)
    B, H, W = 1, 6, 7
    conv, bn = _conv(304, 16, 3, g), _bn(16, g)
    u = torch.randn(B, 256, H, W, generator=g).double().requires_grad_(True)
    z = torch.randn(B, 48, H, W, generator=g).double().requires_grad_(True)
    d1 = bn(conv(torch.cat([u, F.relu(z)], 1))); d1.retain_grad()
    (F.relu(d1) * torch.randn(d1.shape, generator=g).double()).sum().backward()
    m8 = R.pack_bits(torch.cat([torch.rand(B, H, W, 256, generator=g) > 0.5, R.nhwc(z.detach()) > 0], -1))
    gx = R.dgrad_ref(R.nhwc(d1.grad), conv.weight.detach(), _fold(bn), (H, W), 1, 1, 1, m8=m8, mask_c0=256)
    assert _rel(gx, R.nhwc(torch.cat([u.grad, z.grad], 1))) < TOL
    assert _rel(R.fwd_ref(R.nhwc(torch.cat([u, F.relu(z)], 1).detach()), conv.weight.detach(), _fold(bn),
                          (bn.bias - bn.running_mean * _fold(bn)).detach(), 1, 1, 1), R.nhwc(d1.detach())) < TOL


ASPP_CASES = [(name, B, d) for name, (_, _, _, batches, dils) in R.ASPP_ENGINES.items() for B in batches for d in dils]


@pytest.mark.parametrize('name,B,d', ASPP_CASES)
def test_aspp_map_sizes_exercise_the_per_tile_tap_lists(name, B, d):
    """For each engine of the GPU test's merged-ASPP cases (one list: conv_views_ref.ASPP_ENGINES), each batch it runs and each
    dilation it claims: every vertical off-centre tap is kept by some 128-pixel tile and dropped by another, so a tap list that
    is stale, shifted by a tile or shared between tiles changes the result."""
    h, w = R.aspp_map(name)
    assert h >= 21
    for tap, (keep, drop) in R.tap_coverage(B, h, w, d).items():
        assert keep and drop, (tap, keep, drop)
    if B > 1:
        assert (h * w) % 128 != 0          # one tile holds the end of image 0 and the start of image 1


def test_every_dilation_is_covered_by_some_engine_in_each_split_mode():
    """d = 6 cannot be dropped by any tile of the batch-2 bf16x6 map (see ASPP_ENGINES); the batch-1 `small` map covers it."""
    assert set(R.ASPP_ENGINES['main'][4]) == {6, 12, 18}                                      # f16x3
    assert set(R.ASPP_ENGINES['low'][4]) | set(R.ASPP_ENGINES['small'][4]) == {6, 12, 18}     # bf16x6
    h, w = R.aspp_map('low')
    assert all(not drop for keep, drop in R.tap_coverage(2, h, w, 6).values())               # the stated impossibility
    assert 2 * h * w < 764 <= R.aspp_map('main')[0] * R.aspp_map('main')[1]
