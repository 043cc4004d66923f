"""The N > 1 paths on CPU (gloo, world_size 2) with the stand-in engine of tests/fake_engine.py, so that the first real
multi-GPU run is not the first execution of this host code:
  * `train_meta.main` in meta-train mode: tasks sharded over the ranks, one all-reduce per meta-iteration, identical
    RAdam state on every rank, `last_meta_iter.model`, and the concurrent validation CHILD PROCESS
    (`eval_worker`, BASELINE configs[4]) reading the checkpoint snapshots;
  * `bench.py`'s control flow for both metrics under torch.distributed;
  * `evaluate_dataset` with the (sequence, object) work items dealt over the ranks == the single-process result.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
W = os.path.join(HERE, 'mp_workers')


def launch(script, args, world, port, timeout=900):
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), OMP_NUM_THREADS='2', WORLD_SIZE=str(world),
               LOCAL_WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, os.path.join(W, script)] + args, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)))
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=timeout) == 0


def test_train_meta_two_ranks_with_concurrent_eval_process(tmp_path):
    out, save_dir = str(tmp_path / 'res'), str(tmp_path / 'models')
    launch('train_meta_worker.py', [out, save_dir], 2, 29541)
    r0, r1 = (torch.load(f'{out}.{r}', weights_only=False) for r in (0, 1))
    assert r0['step'] == r1['step'] == 2
    assert torch.equal(r0['state'], r1['state'])                       # all-reduce + identical outer step, no broadcast
    run = os.path.join(save_dir, 'mp')
    ck = torch.load(os.path.join(run, 'last_meta_iter.model'), weights_only=False)
    assert ck['meta_iter'] == 2 and len(ck['meta_optim_state_dict']) == 128
    # the validation process evaluated at least the final snapshot and wrote the reference's files
    lines = [json.loads(l) for l in open(os.path.join(run, 'eval_log.jsonl'))]
    assert lines and lines[-1]['meta_iter'] == 2 and lines[-1]['dataset'] == 'val_davis17'
    assert os.path.exists(os.path.join(run, 'last_val_davis17_meta_iter.model'))
    # (best_* is only written when mean J improves on the best so far, evaluate.py:370; the stand-in network scores J = 0)
    assert (lines[-1]['mean_J'] > 0) == os.path.exists(os.path.join(run, 'best_val_davis17_meta_iter.model'))
    assert os.path.exists(os.path.join(run, 'best_eval_preds', 'DAVIS-2017', 'val_seqs', 'synthetic00', '00003.png'))
    # a single process computes the same update (sharding + sum == serial accumulation, up to fp32 summation order)
    out1 = str(tmp_path / 'res1')
    env = dict(os.environ, OMP_NUM_THREADS='2', WORLD_SIZE='1', RANK='0')
    env.pop('MASTER_ADDR', None)
    p = subprocess.Popen([sys.executable, os.path.join(W, 'train_meta_worker.py'), out1, str(tmp_path / 'models1')], env=env)
    assert p.wait(timeout=900) == 0
    s1 = torch.load(f'{out1}.0', weights_only=False)['state']
    assert torch.allclose(s1, r0['state'], rtol=1e-5, atol=1e-8)
    assert float((s1 - r0['state']).abs().max()) < 1e-6


@pytest.mark.parametrize('metric', ['meta', 'finetune'])
def test_bench_control_flow_two_ranks(tmp_path, metric):
    out = str(tmp_path / 'bench')
    launch('bench_worker.py', [out, metric], 2, 29543 if metric == 'meta' else 29545)
    line = json.loads(open(f'{out}.0').read().strip().splitlines()[-1])
    assert open(f'{out}.1').read().strip() == ''                        # rank 0 prints the ONE line
    assert line['n_gpus'] == 2 and line['steps'] == 2 and line['warmup'] == 1 and line['scaling'] == 'weak'
    assert line['metric'] == ('meta_tasks_per_sec' if metric == 'meta' else 'finetune_iters_per_sec')
    per_step = 2 * (4 if metric == 'meta' else 1)                      # ranks x tasks per rank (meta: 4 tasks in flight per GPU)
    assert line['value'] > 0 and abs(line['value'] - per_step * 2 / (line['ms_per_step'] * 2 / 1e3)) < 1e-6 * line['value']
    if metric == 'meta':
        assert line['config']['meta_batch_size'] == 8 and line['config']['tasks_per_rank'] == 4
    assert line['roofline']['kernel'] == 'stand_in_kernel' and line['cpu_baseline'] is None and line['vs_baseline'] is None
    assert line['dtype'].startswith('f32')
    if metric == 'finetune':
        assert line['extra']['meta_tasks_per_sec'] > 0
        # the shapes BASELINE names beside the headline survive in the top-level keys the driver stores
        c = line['configs']
        assert c['meta_tasks_per_sec_tpr1'] > 0 and c['meta_tasks_per_sec_tpr4'] == line['extra']['meta_tasks_per_sec']
        assert c['meta_tpr1_allreduce_ms'] >= 0 and c['c1_b1_ms'] > 0 and c['c3_round_ms'] > 0
    # the headline is ONE timed region of exactly --steps steps (no repeats, no longer region beside it)
    (dt,) = line['extra']['timed_region_samples_s']
    assert 'long_run' not in line and abs(line['ms_per_step'] - 1e3 * dt / 2) < 1e-9 * line['ms_per_step']


@pytest.mark.parametrize('metric', ['finetune', 'meta'])
def test_bench_dump_outputs_of_the_last_timed_step(tmp_path, monkeypatch, metric):
    """`--dump-outputs DIR` (stand-in engine, one process): float32 / float64 arrays of at most 64 MB in all, identical in two
    runs with the same arguments, and -- fine-tune metric -- the loss of the last timed step (warm-up + K steps from the
    loaded state), not of a step run after the timed region."""
    import contextlib
    import importlib.util
    import io

    import numpy as np
    from fake_engine import FakeEngine
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    spec = importlib.util.spec_from_file_location('bench_under_test3', os.path.join(os.path.dirname(HERE), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, 'H', 16)
    monkeypatch.setattr(bench, 'W', 24)
    runs = []
    for r in range(2):
        d = tmp_path / f'run{r}'
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            bench.main(['--steps', '3', '--warmup', '2', '--metric', metric, '--no-cpu-baseline', '--no-ab', '--no-meta',
                        '--dump-outputs', str(d)], engine_factory=FakeEngine, device='cpu', backend='gloo')
        assert json.loads(buf.getvalue().strip().splitlines()[-1])['steps'] == 3
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert all(f.endswith('.npy') for f in os.listdir(d))
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        runs.append(arrays)
    assert runs[0].keys() == runs[1].keys()
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
    if metric == 'finetune':
        assert set(runs[0]) == {'loss', 'logits', 'params_sample'} and runs[0]['logits'].shape == (3, 1, 16, 24)
        from eosvos_amd import synthetic
        e = FakeEngine('resnet50', 16, 24, max_batch=3)
        e.load_model_state(synthetic.synthetic_state('resnet50'), synthetic.synthetic_lrs('resnet50'))
        x, y = synthetic.synthetic_frames(3, 16, 24, seed=7)
        losses = [e.finetune_step(x, y) for _ in range(2 + 3)]
        assert float(runs[0]['loss'][0]) == np.float32(losses[-1])
        assert np.array_equal(runs[0]['params_sample'], bench.param_sample(e.get_params()).numpy())
    else:
        assert set(runs[0]) == {'meta_losses', 'state_sample'} and runs[0]['meta_losses'].shape == (4,)


@pytest.mark.parametrize('metric', ['finetune', 'meta'])
def test_bench_plain_run_measures_only_the_headline(monkeypatch, metric):
    """Without `--full` (stand-in engine, one process): the warm-up and the timed steps are all that run -- no profiled
    pass, no CPU baseline, no further engines or shapes -- and the line carries the headline fields only."""
    import contextlib
    import importlib.util
    import io

    from fake_engine import FakeEngine
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        monkeypatch.delenv(k, raising=False)
    spec = importlib.util.spec_from_file_location('bench_under_test4', os.path.join(os.path.dirname(HERE), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, 'H', 16)
    monkeypatch.setattr(bench, 'W', 24)

    def refuse(*args, **kwargs):
        raise AssertionError('a plain run must not measure the CPU baseline')
    monkeypatch.setattr(bench, 'cpu_baseline_finetune', refuse)
    monkeypatch.setattr(bench, 'cpu_baseline_meta', refuse)
    FakeEngine.instances.clear()
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        bench.main(['--steps', '3', '--warmup', '2', '--metric', metric], engine_factory=FakeEngine, device='cpu', backend='gloo')
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert line['metric'] == ('meta_tasks_per_sec' if metric == 'meta' else 'finetune_iters_per_sec')
    assert line['steps'] == 3 and line['warmup'] == 2 and line['higher_is_better'] is True and line['dtype'].startswith('f32')
    per_step = 4 if metric == 'meta' else 1                            # meta: 4 tasks in flight per GPU
    (dt,) = line['extra']['timed_region_samples_s']
    assert abs(line['ms_per_step'] - 1e3 * dt / 3) < 1e-9 * line['ms_per_step']
    assert abs(line['value'] - per_step * 3 / dt) < 1e-6 * line['value']
    assert not {'roofline', 'cpu_baseline', 'configs'} & set(line)
    assert set(line['extra']) <= {'matrix_mode', 'guard_log', 'guard_enabled', 'lib_version', 'timed_region_samples_s'}
    assert all(getattr(e, '_prof', None) is None for e in FakeEngine.instances)      # no profiled pass
    if metric == 'finetune':
        (e,) = FakeEngine.instances
        assert e.log.count('step') == 2 + 3                            # warm-up + timed steps, nothing after them
    else:
        assert len(FakeEngine.instances) == 4


def test_bench_gpus_flag_must_match_the_world_size(tmp_path):
    """`--gpus N` is the contract, not a hint: a rank started with another WORLD_SIZE refuses to run (and N > 1 without
    WORLD_SIZE self-launches N ranks, which needs N GPUs: here it must fail loudly, there being none)."""
    env = dict(os.environ, OMP_NUM_THREADS='2')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    root = os.path.dirname(HERE)
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1'], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and 'GPU(s) visible' in p.stderr and p.stdout.strip() == ''
    p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1'], env=dict(env, WORLD_SIZE='1', RANK='0'),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and 'WORLD_SIZE=1' in p.stderr and p.stdout.strip() == ''


def test_bench_self_launch_fails_when_a_rank_fails():
    """`bench.py --gpus N` starts its N ranks as fresh children (`python -m torch.distributed.run`); when one of them dies --
    here rank 1 of 2, before the first collective, while rank 0 waits in a barrier -- the launcher tears the others down and
    bench.py exits non-zero WITHOUT a result line (round-4 verdict, next #8)."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location('bench_under_test2', os.path.join(os.path.dirname(HERE), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = types.SimpleNamespace(gpus=2)
    with pytest.raises(SystemExit) as exc:
        bench.self_launch(a, ['--gpus', '2'], script=os.path.join(W, 'failing_rank_worker.py'), need_gpus=False)
    assert 'rank processes failed' in str(exc.value) and 'result line: False' in str(exc.value)


def test_bench_traffic_lookup_covers_every_leading_kernel_symbol(tmp_path, monkeypatch):
    """`roofline.traffic` comes from the committed PMC passes; three kernel symbols take a similar share of the step and which
    one leads flips between runs, so the artifact records all of them (`others`) and the lookup must find each -- and must
    answer None with a reason for another library version, batch or symbol."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(os.path.dirname(HERE), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    art = {'kernel': 'wgrad_h3_kernel<128, 128>', 'batch': 3, 'lib_version': 'v', 'traffic_bytes_per_launch': 1.0, 'note': 'n',
           'others': [{'kernel': 'conv_h3_kernel<128, true>', 'traffic_bytes_per_launch': 2.0},
                      {'kernel': 'conv_h3_kernel<128, false>', 'traffic_bytes_per_launch': 3.0}]}
    path = tmp_path / 'pmc.json'
    path.write_text(json.dumps(art))
    monkeypatch.setattr(bench, 'PMC_FILES', [str(tmp_path / 'missing.json'), str(path)])
    assert bench.pmc_traffic('wgrad_h3_kernel<128, 128>', 'v', 3) == (1.0, 'n')
    assert bench.pmc_traffic('conv_h3_kernel<128, true>', 'v', 3) == (2.0, 'n')
    assert bench.pmc_traffic('conv_h3_kernel<128, false>', 'v', 3) == (3.0, 'n')
    for args in (('conv_h3_kernel<64, true>', 'v', 3), ('wgrad_h3_kernel<128, 128>', 'w', 3), ('wgrad_h3_kernel<128, 128>', 'v', 1)):
        t, why = bench.pmc_traffic(*args)
        assert t is None and 'PMC artifact is for' in why
    # the committed artifact of this round is well-formed
    real = json.load(open(os.path.join(os.path.dirname(HERE), 'profiles', 'r04_pmc_dominant_kernel.json')))
    assert real['traffic_bytes_per_launch'] > 0 and all(o['traffic_bytes_per_launch'] > 0 for o in real.get('others', []))


def test_evaluation_sharded_over_ranks_equals_single_process(tmp_path):
    out2, out1 = str(tmp_path / 'e2'), str(tmp_path / 'e1')
    launch('eval_shard_worker.py', [out2, str(tmp_path / 's2')], 2, 29547)
    env = dict(os.environ, OMP_NUM_THREADS='2', WORLD_SIZE='1', RANK='0')
    assert subprocess.Popen([sys.executable, os.path.join(W, 'eval_shard_worker.py'), out1, str(tmp_path / 's1')],
                            env=env).wait(timeout=900) == 0
    a, b, one = (torch.load(p, weights_only=False) for p in (f'{out2}.0', f'{out2}.1', f'{out1}.0'))
    # three (sequence, object) items dealt round-robin: rank 0 takes items 0 and 2, rank 1 item 1
    assert a['items'] == [('bear', 0), ('cows', 0)] and b['items'] == [('bear', 1)]
    for seq in one['labels']:
        assert torch.equal(a['labels'][seq], one['labels'][seq]) and torch.equal(b['labels'][seq], one['labels'][seq])
    assert a['J_seq'] == one['J_seq']
    assert os.path.exists(os.path.join(str(tmp_path / 's2'), 'best_eval_preds', 'DAVIS-2017', 'val_seqs', 'bear', '00000.png'))


@pytest.mark.parametrize('mbs', [4, 8])
def test_meta_iteration_four_ranks_nan_task_and_short_tail(tmp_path, mbs):
    """world_size 4 (BASELINE configs[3] / [4] shapes): meta_batch_size 4 (one task per rank) and 8 (two per rank: the
    concurrent-engine path), one NaN task on one rank, one iteration in which some ranks have fewer (or no) tasks -- every
    rank takes part in every all-reduce and applies the same outer step (`src/util/meta_run.py:39,209-243`,
    `src/train_meta.py:361-373`); the result equals the single-process run of the same tasks."""
    out4, out1 = str(tmp_path / 'w4'), str(tmp_path / 'w1')
    launch('meta_ws_worker.py', [out4, str(mbs)], 4, 29551 + mbs)
    env = dict(os.environ, OMP_NUM_THREADS='2', WORLD_SIZE='1', RANK='0')
    env.pop('MASTER_ADDR', None)
    assert subprocess.Popen([sys.executable, os.path.join(W, 'meta_ws_worker.py'), out1, str(mbs)], env=env).wait(timeout=900) == 0
    res = [torch.load(f'{out4}.{r}', weights_only=False) for r in range(4)]
    one = torch.load(f'{out1}.0', weights_only=False)
    for r in res:
        assert r['step'] == 4 and r['collectives'] == 5                # 4 gradient all-reduces + the matrix-mode verdict of the first
        # meta-iteration (MetaTrainer._collective_mode_check): no rank skipped a collective, short task list or not
        assert torch.equal(r['state'], res[0]['state'])                # identical outer step everywhere
        assert r['engines'] == (2 if mbs == 8 else 1)
    assert sum(r['skipped'] for r in res) == 1 == one['skipped']       # the NaN task, counted once
    assert [len(l) for l in res[3]['losses']] == ([1, 1, 1, 0] if mbs == 4 else [2, 2, 2, 1])      # rank 3 lost tasks in the tail
    assert [len(l) for l in res[0]['losses']] == ([1, 1, 1, 1] if mbs == 4 else [2, 2, 2, 2])
    assert torch.allclose(one['state'], res[0]['state'], rtol=1e-5, atol=1e-8)
    assert float((one['state'] - res[0]['state']).abs().max()) < 1e-6
