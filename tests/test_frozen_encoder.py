"""Frozen-encoder fine-tuning (`parent_model.train_encoder: False`, cfgs/meta.yaml:71) on the host: configuration,
requires_grad flags and the MetaOptimizer layout against the reference (fixture G24, tests/golden/make_g24.py), the
`freeze_encoder` counts over the trainable subset, and a world-2 gloo meta-training run whose all-reduce carries exactly
the subset.  The stand-in engine of tests/fake_engine.py is subclassed here to take the boundary."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BN = {'accum_stats': False, 'learn_weight': False, 'learn_bias': False}
ARCHS = [('DeepLabV3Plus', 'resnet50', 'resnet50'), ('DeepLabV3Plus', 'resnet101', 'resnet101'),
         ('DeepLabV3', 'resnet50', 'deeplabv3_resnet50')]


@pytest.fixture(scope='module')
def g24(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'g24_frozen_layout.json')))


def _model(arch, encoder):
    from eosvos_amd.networks import DeepLabV3, DeepLabV3Plus
    cls = DeepLabV3 if arch == 'DeepLabV3' else DeepLabV3Plus
    return cls(encoder, num_classes=1, batch_norm=BN, train_encoder=False)


def test_config_passes_train_encoder_through(monkeypatch):
    from eosvos_amd import config, helper_func, topology
    cfg = config.parse_cli(['with', 'DAVIS-2017', 'parent_model.train_encoder=False'])
    assert cfg['parent_model']['train_encoder'] is False
    seen = {}

    class Spy(helper_func.DeepLabV3Plus):
        def __init__(self, *a, **k):
            seen.update(k)
            super().__init__(*a, **k)
    monkeypatch.setattr(helper_func, 'DeepLabV3Plus', Spy)
    model, _ = helper_func.init_parent_model(**cfg['parent_model'])
    assert seen['train_encoder'] is False
    assert model._train_from == topology.trainable_from(model.encoder, False) == 43
    assert config.parse_cli(['with', 'DAVIS-2017'])['parent_model']['train_encoder'] is True


@pytest.mark.parametrize('arch,encoder,key', ARCHS)
def test_requires_grad_and_layout_match_the_reference(g24, arch, encoder, key):
    from eosvos_amd import topology
    from eosvos_amd.meta_optim import MetaOptimizer
    ref = g24[key]
    model = _model(arch, encoder)
    got = [[n, list(p.shape)] for n, p in model.named_parameters() if p.requires_grad]
    assert got == ref['trainable']
    assert len(model.state_dict()) == ref['n_state_keys']
    # the frozen tensors are a prefix of the engine's flat order; every conv before the boundary has one tensor
    names = [n for n, _ in topology.trainable(model.encoder)]
    nf = topology.frozen_tensors(model.encoder, False)
    assert [n for n, _ in ref['trainable']] == names[nf:]
    assert model._train_from == nf and topology.conv_infos(model.encoder)[nf].name + '.weight' == names[nf]
    for lvl in ('SINGLE', 'TENSOR', 'NEURON', 'PARAM'):
        for use_log in (False, True):
            mo = MetaOptimizer(model, init_lr=1e-3, learn_model_init=True, second_order_gradients=False,
                               lr_hierarchy_level=lvl, use_log_init_lr=use_log, max_lr=None)
            assert [[n, list(p.shape)] for n, p in mo.named_parameters()] == ref['meta_' + lvl], (lvl, use_log)
            assert [[k, list(v.shape)] for k, v in mo.state_dict().items()] == ref['meta_' + lvl]
            assert mo.meta_model.num_param_groups == len(ref['trainable'])
            if lvl == 'SINGLE':
                assert tuple(mo.state_lr.shape) == (len(ref['trainable']), 1)


def test_reference_counts():
    """The counts the issue quotes, from the layout (G24 pins the lists themselves)."""
    from eosvos_amd import topology
    for enc, tensors, scalars, frozen in (('resnet50', 21, 31777025, 43), ('resnet101', 21, 31777025, 94),
                                          ('deeplabv3_resnet50', 9, 16122113, 53)):
        tr = topology.trainable(enc)
        nf = topology.frozen_tensors(enc, False)
        assert nf == frozen and len(tr) - nf == tensors
        assert sum(math.prod(s) for _, s in tr[nf:]) == scalars


def test_full_checkpoint_does_not_load_into_a_frozen_encoder_optimizer():
    from eosvos_amd.meta_optim import MetaOptimizer
    from eosvos_amd.networks import DeepLabV3Plus
    kw = dict(init_lr=1e-3, learn_model_init=True, second_order_gradients=False, lr_hierarchy_level='NEURON',
              use_log_init_lr=False, max_lr=None)
    full = MetaOptimizer(DeepLabV3Plus('resnet50', 1, batch_norm=BN), **kw)
    frozen = MetaOptimizer(_model('DeepLabV3Plus', 'resnet50'), **kw)
    assert len(full.state_dict()) == 128 and len(frozen.state_dict()) == 42
    with pytest.raises(RuntimeError, match='Unexpected key'):
        frozen.load_state_dict(full.state_dict())
    with pytest.raises(KeyError):
        full.load_state_dict(frozen.state_dict())
    sd = {k: v * 0 + 2e-3 for k, v in frozen.state_dict().items()}
    frozen.load_state_dict(sd)
    assert float(frozen._lr_flat.max()) == pytest.approx(2e-3)


def _frozen_fake():
    sys.path.insert(0, HERE)
    from fake_engine import FakeEngine

    class FrozenFake(FakeEngine):
        """The stand-in with the boundary of `eosvos_set_trainable_from` (full-layout entries, as the engine's)."""
        train_from = 0

        def set_trainable_from(self, conv_idx):
            self.train_from = int(conv_idx)
    return FrozenFake


@pytest.mark.parametrize('encoder,expect_lr', [('resnet50', 3 * (512 + 512 + 2048) + 2048), ('deeplabv3_resnet50', 0)])
def test_freeze_encoder_counts_over_the_subset(encoder, expect_lr):
    from eosvos_amd import topology
    from eosvos_amd.meta_run import MetaTrainer
    eng = _frozen_fake()(encoder, 16, 24, 1)
    eng.set_trainable_from(topology.trainable_from(encoder, False))
    mt = MetaTrainer(eng, meta_batch_size=1, freeze_encoder=True)
    tr = topology.trainable(encoder)[eng.train_from:]
    assert mt.n_lr == sum(s[0] for _, s in tr) and mt.n_param == sum(math.prod(s) for _, s in tr)
    assert mt.state.numel() == mt.n_lr + mt.n_param
    assert mt._backbone_lr == expect_lr
    assert mt._backbone_param == sum(math.prod(s) for n, s in tr if n.startswith('backbone'))
    assert not mt.fused_outer
    assert list(mt.state_dict())[0] == 'log_init_lr_' + tr[0][0].replace('.', '-')


_WORKER = r'''
import os, sys
sys.path[:0] = [{root!r}, {tests!r}, os.path.join({tests!r}, 'mp_workers')]
import torch
import torch.distributed
import common
from fake_engine import FakeDeepLab, FakeEngine
from eosvos_amd import train_meta, topology

class FrozenFake(FakeEngine):
    train_from = 0
    def set_trainable_from(self, conv_idx):
        self.train_from = int(conv_idx)

class FrozenDeepLab(FakeDeepLab):
    def _ensure_engine(self, height, width, batch):
        e = self.engine
        if e is None or e.height != height or e.width != width or batch > e.max_batch:
            self.engine = FrozenFake(self.encoder, height, width, max(batch, self.max_batch))
            self.engine.set_trainable_from(self._train_from)
            self._dirty = True
        return super()._ensure_engine(height, width, batch)

def init(architecture='DeepLabV3Plus', encoder='resnet50', batch_norm=None, train_encoder=True, **_kw):
    return FrozenDeepLab(encoder, num_classes=1, batch_norm=batch_norm, train_encoder=train_encoder), {{}}

sizes = []
_all_reduce = torch.distributed.all_reduce
def all_reduce(t, *a, **k):
    sizes.append(t.numel())
    return _all_reduce(t, *a, **k)
torch.distributed.all_reduce = all_reduce
os.environ['EOSVOS_DIST_BACKEND'] = 'gloo'
train_meta.init_parent_model = init
out, save_dir = sys.argv[1], sys.argv[2]
mt = train_meta.main(['with', 'YouTube-VOS', 'meta_batch_size=2', 'num_epochs.train=2', 'vis_interval=1', f'save_dir={{save_dir}}',
                      'env_suffix=fz', 'parent_model.train_encoder=False'], height=common.H, width=common.W, num_frames=4,
                     num_meta_iters=2, data_root=os.path.join(save_dir, 'no_data'), device='cpu')
torch.save({{'sizes': sizes, 'n': mt.state.numel(), 'keys': list(mt.state_dict()), 'state': mt.state.clone()}},
           f'{{out}}.{{os.environ["RANK"]}}')
'''


def test_train_meta_two_ranks_all_reduces_the_subset(tmp_path):
    from eosvos_amd import topology
    script = tmp_path / 'worker.py'
    script.write_text(_WORKER.format(root=ROOT, tests=HERE))
    out = str(tmp_path / 'res')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29561', OMP_NUM_THREADS='2', WORLD_SIZE='2',
               LOCAL_WORLD_SIZE='2')
    procs = [subprocess.Popen([sys.executable, str(script), out, str(tmp_path / 'models')],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    res = [torch.load(f'{out}.{r}', weights_only=False) for r in range(2)]
    tr = topology.trainable('resnet50')[43:]
    n = sum(s[0] for _, s in tr) + sum(math.prod(s) for _, s in tr)
    assert n == 31777025 + sum(s[0] for _, s in tr)
    for r in res:
        assert r['n'] == n
        # one all-reduce of the meta-gradient per meta-iteration, of the subset's length
        assert [s for s in r['sizes'] if s > 1] == [n, n], r['sizes']
        assert len(r['keys']) == 42 and r['keys'][0] == 'log_init_lr_backbone-layer4-0-conv1-weight'
    assert torch.equal(res[0]['state'], res[1]['state'])


def test_trainable_from_symbol_is_exported():
    """The C-ABI entry of the boundary: declared in include/eosvos.h, bound by the ctypes layer, exported by the library."""
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, 'e-osvos_amd', 'libeosvos.so')):
        ge.build()
    from eosvos_amd import _ffi
    assert 'int eosvos_set_trainable_from(eosvos_engine* e, int conv_idx);' in open(os.path.join(ROOT, 'include', 'eosvos.h')).read()
    assert 'eosvos_set_trainable_from' in _ffi.exported_symbols()
    assert hasattr(_ffi.load(), 'eosvos_set_trainable_from')
