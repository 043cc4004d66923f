"""Benchmark of the e-OSVOS fine-tuning hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
(for N > 1 the driver launches it under torch.distributed.run, one rank per GPU).

Workload = BASELINE.json configs[1] "e-OSVOS-50 DAVIS-2017 val, 50 fine-tune iters,
batch=3": one *step* is one fine-tune iteration (DeepLabV3+-ResNet50 forward, fused BCE
loss+grad, backward, fused per-neuron-lr SGD update) on a batch of 3 synthetic 480x854
frames that are already resident in HBM.  Each rank fine-tunes its own (sequence, object)
replica -- evaluation shards by (sequence, object) with no collective -- so
scaling is weak and `value` = fine-tune iterations/s summed over ranks.
`extra.meta_tasks_per_sec` reports the meta-train metric (K=5 inner steps + meta frame,
B=1, RCCL all-reduce of the 161 MB meta-gradient + fused RAdam at N > 1);
`--metric meta` makes that the headline of the JSON line instead (BASELINE configs[3..4]:
one task per rank per meta-iteration, a step = one meta-iteration).

`roofline` is about the kernel symbol that takes the most time in a step, found and timed live: after the timed
region the same steps run once more with HIP events around every matrix-core launch, recorded on the stream each
launch runs on (eosvos_profile_launches); achieved = that kernel's executed fp32-equivalent FLOPs / its summed
duration.  Tensors, accumulators and epilogues are fp32; `dtype` names how the contractions use the matrix cores:
"f32 (f16x3 split)" (default) = per-tensor power-of-two scale, 2 fp16 pieces per operand, 3 of the 4 partial products on
v_mfma_f32_16x16x32_f16 with fp32 accumulation (roof = dense 16-bit MFMA peak / 3); "f32 (bf16x6 split)" = exact 3-way
bf16 split, 6 partial products (peak / 6, no range assumption); "f32" = the fp32 MFMA.  EOSVOS_MFMA selects the mode.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process starts N rank processes itself
(`python -m torch.distributed.run --nproc-per-node N bench.py ...`, fresh children, before anything here touches the
GPU) and relays rank 0's line; under torch.distributed.run (WORLD_SIZE set) it is one of the ranks.
`configs` (top level) keeps the other BASELINE shapes next to the headline: batch-1 iteration (C1), one online-adaptation
round (C3), meta-tasks/s with ONE task per rank (the configs[3] / [4] shape: meta_batch_size = ranks) and with
`--tasks-per-rank` in flight, each with its all-reduce time, and the same iteration in the other matrix modes.

The timed region is exactly `--steps` steps, run once; `ms_per_step` is its duration / steps.  `--dump-outputs DIR`
writes what the last timed step computed (`dump_outputs`) as DIR/<name>.npy, read back before anything else runs.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, `--dump-outputs`, the result line
(headline fields, `config`, and in `extra` the matrix mode, guard log, library version and timed-region sample).
`--full` also measures everything else the line has carried: `roofline` (its profiled pass and the one-stream engine),
`cpu_baseline`, `configs` and the rest of `extra` (C1 / C3 shapes, the meta metric beside the fine-tune one, the other
matrix modes, 3 objects in flight, GroupNorm mode); `--no-cpu-baseline` / `--no-meta` / `--no-ab` leave parts of that out.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, BATCH = 480, 854, 3
FLOPS_PER_FRAME_ITER = 647.8e9      # fwd + dgrad + wgrad as direct convolutions, no stem dgrad
FP32_MATRIX_PEAK = 157.3            # TFLOP/s, MI355X_MICROARCH.md "Peak FP32 (matrix)"
BF16_DENSE_PEAK = 2500.0            # TFLOP/s, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"
PMC_FILES = [os.path.join(ROOT, 'profiles', n) for n in ('r06_pmc_dominant_kernel.json', 'r05_pmc_dominant_kernel.json', 'r04_pmc_dominant_kernel.json')]


MFMAS_PER_FMA = {'f16x3': 3, 'bf16x6': 6}      # 16-bit MFMA issues per fp32 multiply-accumulate
DUMP_SAMPLE = 1 << 23                           # --dump-outputs: weight vectors are written as a fixed sample of this many values


def param_sample(flat):
    """A fixed sample of a flat weight vector for --dump-outputs: DUMP_SAMPLE positions drawn with seed 0 (in index order),
    the same positions in every run; the whole vector when it is not larger."""
    flat = flat.detach().float().cpu()
    if flat.numel() <= DUMP_SAMPLE:
        return flat
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_SAMPLE].sort().values
    return flat[idx]


def dump_outputs(path, arrays):
    """--dump-outputs DIR: one DIR/<name>.npy per array, float32 or float64 (about 37 MB in all)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(path, name + '.npy'), a)


def matrix_peak(mode):
    """fp32-equivalent TFLOP/s roof of the matrix mode = the dense 16-bit MFMA peak / the MFMAs it issues per fp32
    multiply-accumulate (f16x3: 3, bf16x6: 6); the fp32 MFMA peak in the f32 mode."""
    return BF16_DENSE_PEAK / MFMAS_PER_FMA[mode] if mode in MFMAS_PER_FMA else FP32_MATRIX_PEAK


def mode_of(eng, engine_mod):
    """The matrix mode this engine's launches run in (its own if the range guard or a caller gave it one, else the process's)."""
    return eng.matrix_mode if hasattr(eng, 'matrix_mode') else engine_mod.get_matrix_mode()


def dtype_name(mode):
    """fp32 tensors / accumulators throughout; the split the contractions run in is part of the name."""
    return f'f32 ({mode} split)' if mode in MFMAS_PER_FMA else 'f32'


def self_launch(a, argv, script=None, need_gpus=True):
    """`--gpus N > 1` outside torch.distributed.run: start the N ranks as fresh child processes (this process has not
    touched the GPU: counting devices does not initialise it) and relay rank 0's JSON line.  A rank that fails takes the
    run with it: torch.distributed.run tears the other ranks down and this process exits non-zero without a result line.
    (`script` / `need_gpus`: the CPU test of exactly that, tests/test_multiprocess.py.)"""
    import socket
    import subprocess
    n = torch.cuda.device_count()
    if need_gpus and n < a.gpus:
        raise SystemExit(f'bench.py --gpus {a.gpus}: only {n} GPU(s) visible')
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={a.gpus}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), script or os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for out in proc.stdout:
        try:
            if 'metric' in json.loads(out):
                line = out.strip()
                continue
        except ValueError:
            pass
        sys.stderr.write(out)                       # anything else the ranks print is not the result line
    rc = proc.wait()
    if rc != 0 or line is None:
        raise SystemExit(f'bench.py --gpus {a.gpus}: the rank processes failed (exit code {rc}, result line: {line is not None})')
    print(line, flush=True)


def cpu_threads():
    # oneDNN stops scaling (and thrashes) far below the hardware threads of the GPU box's host
    return min(os.cpu_count() or 1, 32)


def cpu_model():
    """Model string and thread count of the host the CPU baseline runs on ('state core count and CPU model')."""
    name = None
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                name = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    return {'model': name, 'hardware_threads': os.cpu_count()}


def cpu_baseline_finetune(sd, lrs, x, y, seconds_budget=25.0):
    """The CPU oracle (oracle/meta.py, torch fp32) timed on whole batch-3 fine-tune iterations of the benchmarked
    workload: 1 warm-up + >= 3 timed iterations (bounded by ~seconds_budget)."""
    from oracle import meta
    cores = cpu_threads()
    torch.set_num_threads(cores)
    _, _, P = meta.finetune_step(sd, lrs, x, y)              # warm-up (oneDNN primitives, page-in)
    n, t0 = 0, time.time()
    while True:
        _, _, P = meta.finetune_step(P, lrs, x, y)
        n += 1
        dt = time.time() - t0
        if n >= 3 and (dt > seconds_budget or n >= 8):
            break
    return {'value': n / dt, 'unit': 'finetune_iters/s', 'cores': cores, 'kind': 'port', 'cpu': cpu_model(),
            'sample': f'{n} batch-{x.shape[0]} fine-tune iterations ({H}x{W}, the benchmarked workload) of the torch-CPU '
                      f'oracle (oracle/meta.py) on {cores} threads in {dt:.1f}s after 1 warm-up iteration'}


def cpu_baseline_meta(sd, lrs, x1, y1, xm, ym):
    """One meta task (5 inner steps + meta frame, batch 1) of the CPU oracle after one warm-up inner step."""
    from oracle import meta
    cores = cpu_threads()
    torch.set_num_threads(cores)
    meta.finetune_step(sd, lrs, x1, y1)
    t0 = time.time()
    meta.meta_task(sd, lrs, [(x1, y1)] * 5, (xm, ym))
    dt = time.time() - t0
    return {'value': 1.0 / dt, 'unit': 'meta_tasks/s', 'cores': cores, 'kind': 'port', 'cpu': cpu_model(),
            'sample': f'1 meta task (5 inner steps + 1 meta frame, batch 1, {H}x{W}) of the torch-CPU oracle '
                      f'(oracle/meta.py meta_task) on {cores} threads in {dt:.1f}s after 1 warm-up inner step'}


def pmc_traffic(kernel, lib_version, batch):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (tools/pmc_dominant.sh), if they were
    taken for this library version / kernel / batch; else None."""
    why = 'no PMC artifact'
    for path in PMC_FILES:
        try:
            p = json.load(open(path))
        except (OSError, ValueError):
            continue
        if p.get('lib_version') != lib_version or p.get('batch') != batch:
            why = f"PMC artifact is for {p.get('kernel')} / {p.get('lib_version')} / batch {p.get('batch')}"
            continue
        # (three symbols take 20-24 % of the step each and which one leads flips between runs: the passes record all of them)
        for q in [p] + list(p.get('others', [])):
            if q.get('kernel') == kernel:
                return q['traffic_bytes_per_launch'], p.get('note', '')
        why = f"PMC artifact is for {p.get('kernel')} / {p.get('lib_version')} / batch {p.get('batch')}"
    return None, why


def profiled_pass(eng, run_step, steps):
    """Per-kernel totals over `steps` more steps with HIP events around every matrix-core launch."""
    eng.profile_launches(True)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run_step()
    eng.synchronize()
    dt = time.perf_counter() - t0
    rows = eng.profile_read()
    eng.profile_launches(False)
    return rows, dt / steps


def roofline_from(rows, steps, mode, lib_version, batch, ms_per_step):
    mf = {k: v for k, v in rows.items() if 'fixup' not in k}
    kernel = max(mf, key=lambda k: mf[k][1])
    launches, ms, flops = mf[kernel]
    achieved = flops / (ms * 1e-3) / 1e12
    peak = matrix_peak(mode)
    total_flops = sum(v[2] for v in mf.values()) / steps
    traffic, note = pmc_traffic(kernel, lib_version, batch)
    return {
        'bound': 'mfma', 'kernel': kernel, 'achieved': achieved, 'peak': peak, 'unit': 'TFLOP/s', 'frac': achieved / peak,
        'peak_basis': (f'dense 16-bit MFMA peak 2500 TFLOP/s / {MFMAS_PER_FMA[mode]} MFMAs per fp32 multiply-accumulate in the '
                       f'{mode} mode (fp32-equivalent)' if mode in MFMAS_PER_FMA else 'fp32 MFMA peak'),
        'frac_of_bf16x6_roof': achieved / (BF16_DENSE_PEAK / 6.0),      # the yardstick of rounds 2-3 (416.7 TFLOP/s)
        # what the same MFMA stream reaches with its fragments in registers (no memory at all) on random operands -- the chip is
        # power-limited (profiles/r03_h3_phases_probe.txt: f16x3 516, constant operands 753; r02_x6_phases_probe.txt: bf16x6 305)
        'measured_mfma_only_tflops': {'f16x3': 516.0, 'bf16x6': 305.0}.get(mode),
        'achieved_is': 'executed fp32-equivalent FLOPs of all launches of this kernel symbol in the profiled steps / their '
                       'summed HIP-event durations (padding taps skipped by the tap tables are not counted)',
        'launches_per_step': launches / steps, 'avg_launch_us': 1e3 * ms / launches,
        'flops_per_launch': flops / launches, 'share_of_step_kernel_time': ms / sum(v[1] for v in rows.values()),
        'executed_16bit_mfma_tflops': MFMAS_PER_FMA[mode] * achieved if mode in MFMAS_PER_FMA else None,
        'frac_of_fp32_matrix_peak': achieved / FP32_MATRIX_PEAK,
        'traffic': traffic, 'traffic_note': note,
        'whole_step_executed_gflop': total_flops / 1e9,
        'whole_step_executed_tflops': total_flops / (ms_per_step * 1e-3) / 1e12,
        'whole_step_executed_frac': total_flops / (ms_per_step * 1e-3) / 1e12 / peak,
        'whole_step_frac_of_fp32_matrix_peak': total_flops / (ms_per_step * 1e-3) / 1e12 / FP32_MATRIX_PEAK,
        'per_kernel': {k: {'launches_per_step': v[0] / steps, 'ms_per_step': v[1] / steps,
                           'tflops': (v[2] / (v[1] * 1e-3) / 1e12) if v[1] > 0 else None} for k, v in sorted(rows.items())},
    }


def timed_median(fn, steps, barrier, dist, dev, repeats=None):
    """Timed region of EXACTLY `steps` steps; when it is short (< 100 steps) it is run three times and the MEDIAN is
    reported (one 0.2 s sample is at the mercy of the clock the chip happens to hold).  Returns (seconds, all samples)."""
    reps = repeats if repeats is not None else (3 if steps < 100 else 1)
    samples = sorted(timed(fn, steps, barrier, dist, dev) for _ in range(reps))
    return samples[len(samples) // 2], samples


def timed(fn, steps, barrier, dist, dev):
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def meta_setup(eng, dist, world, rank, sd, lrs, dev, tasks_per_rank, engine_factory):
    """MetaTrainer with `tasks_per_rank` tasks per meta-iteration on this GPU, in flight together on as many engines (each
    on its own stream), and the step function of one meta-iteration."""
    from eosvos_amd import synthetic
    from eosvos_amd.meta_run import MetaTrainer
    extra = []
    real = engine_factory.__name__ == 'Engine' and torch.cuda.is_available()
    if real and tasks_per_rank > 1:
        # Engines in flight: one queue each, every one built fresh and back to back on a new stream.  ROCm deals streams onto
        # its hardware queues in creation order; engines whose queues share one or sit on the same pipe lose a quarter of
        # their rate (33 instead of 41 tasks/s, profiles/r03_hw_queue_sweep.txt), so the headline's engine (default stream +
        # its side stream) is left out of this.
        fresh = []
        for _ in range(tasks_per_rank):
            with torch.cuda.stream(torch.cuda.Stream()):
                fresh.append(engine_factory('resnet50', H, W, max_batch=1, device=dev, side_stream=False))
        eng, extra = fresh[0], fresh[1:]
    else:
        for _ in range(tasks_per_rank - 1):
            extra.append(engine_factory('resnet50', H, W, max_batch=1, device=dev))
    mt = MetaTrainer(eng, dist=dist, meta_batch_size=world * tasks_per_rank, extra_engines=extra)
    mt.load_state(sd, lrs)
    tasks = []
    for t in range(tasks_per_rank):
        x, y = synthetic.synthetic_frames(1, H, W, seed=1000 + rank * tasks_per_rank + t)
        x, y = x.to(dev), y.to(dev)
        tasks.append((x, y, torch.flip(x, dims=[3]).contiguous(), torch.flip(y, dims=[3]).contiguous()))
    losses = []

    def step():
        losses[:] = mt.meta_iteration(tasks, inner_steps=5)
    return mt, step, losses, (extra + [eng] if real and tasks_per_rank > 1 else extra)


def bench_meta(a, eng, dist, rank, world, sd, lrs, x, y, xg, yg, barrier, dev, mode, lib_version, engine_factory):
    """meta-tasks/s: every rank runs `--tasks-per-rank` tasks (5 inner steps at batch 1 + the meta frame each) per
    meta-iteration, in flight together on one engine each, then ONE all-reduce of the 161 MB meta-gradient and the fused
    RAdam step + lr clamp on every rank."""
    tpr = a.tasks_per_rank
    mt, step, losses, extra = meta_setup(eng, dist, world, rank, sd, lrs, dev, tpr, engine_factory)
    for _ in range(max(a.warmup, 1)):
        step()                                                                  # (the collective range-guard verdict falls in the first)
    from eosvos_amd import engine as engine_mod
    mode = mode_of(mt.eng, engine_mod)                                           # the mode the timed meta-iterations run in
    dt = timed(step, a.steps, barrier, dist, dev)
    samples = [dt]
    ms_per_step = 1e3 * dt / a.steps
    if a.dump_outputs and rank == 0:
        # the last timed meta-iteration: its tasks' meta losses and the learned state (lrs + model init) after its outer step
        dump_outputs(a.dump_outputs, {'meta_losses': torch.tensor([float(l) for l in losses], dtype=torch.float64),
                                      'state_sample': param_sample(mt.state)})
    if mode_of(mt.eng, engine_mod) != mode:
        raise SystemExit(f'bench.py: the matrix mode changed inside the timed region ({mode} -> {mode_of(mt.eng, engine_mod)})')
    head = {
        'metric': 'meta_tasks_per_sec', 'value': world * tpr * a.steps / dt, 'unit': 'meta_tasks/s', 'n_gpus': world,
        'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': ms_per_step, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': dtype_name(mode), 'data': 'synthetic',
        'config': {'workload': f'meta-train iteration (BASELINE configs[3..4]): meta_batch_size = {tpr} x ranks, {tpr} tasks per '
                               f'rank in flight together (one engine each), a task = 5 inner fine-tune steps + 1 meta frame at '
                               f'batch 1, {H}x{W}, BCE; one all-reduce(sum) of the 40.3 M-float meta-gradient, RAdam + lr clamp '
                               'on every rank',
                   'meta_batch_size': world * tpr, 'tasks_per_rank': tpr, 'inner_steps': 5, 'height': H, 'width': W,
                   'parallelism': f'tasks sharded x{world}'},
    }
    if not a.full:
        if rank == 0:
            print(json.dumps(dict(head, extra={'matrix_mode': mode, 'guard_log': [list(g) for g in engine_mod.GUARD_LOG],
                                               'lib_version': lib_version, 'timed_region_samples_s': samples})), flush=True)
        for e in extra:
            e.close()
        eng.close()
        if dist is not None:
            dist.destroy_process_group()
        return
    mt.profile = {}
    for _ in range(2):
        step()                                                                  # all-reduce / outer-step split (drains the GPU per phase)
    split = {k: v / mt.profile['iterations'] for k, v in mt.profile.items() if k != 'iterations'}
    mt.profile = None
    rows, _ = profiled_pass(eng, step, min(a.steps, 4))
    roof = roofline_from(rows, min(a.steps, 4), mode, lib_version, 1, ms_per_step)
    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline_meta(sd, lrs, x[:1], y[:1], torch.flip(x[:1], dims=[3]), torch.flip(y[:1], dims=[3]))
    for e in extra:
        e.close()
    if rank == 0:
        out = dict(head, roofline=roof, cpu_baseline=cpu,
                   extra={'last_meta_loss': losses[-1], 'matrix_mode': mode, 'guard_log': [list(g) for g in engine_mod.GUARD_LOG],
                          'lib_version': lib_version, 'timed_region_samples_s': samples, 'phase_ms_per_meta_iteration': split})
        print(json.dumps(out), flush=True)
    eng.close()
    if dist is not None:
        dist.destroy_process_group()


def main(argv=None, engine_factory=None, device=None, backend='nccl'):
    """`engine_factory` / `device` / `backend`: the gloo CPU tests of this control flow pass a stand-in engine, 'cpu' and
    'gloo' (tests/test_multiprocess.py); the benchmark itself always runs the HIP engine on cuda under RCCL."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=None, help='timed steps (default: 200 fine-tune iterations / 40 '
                                                             'meta-iterations, a timed region of about 2 s)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed to DIR/<name>.npy (fine-tune: loss, logits and a fixed sample '
                         'of the updated weights; meta: the meta losses and a fixed sample of the learned state)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline also measure the roofline, CPU baseline, other shapes, modes and configurations '
                         '(a plain run does only set-up, warm-up, the timed steps, --dump-outputs and the result line)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full: skip the CPU baseline')
    ap.add_argument('--no-meta', action='store_true', help='--full: skip the meta metric in extra')
    ap.add_argument('--no-ab', action='store_true', help='--full: skip the other matrix modes and engine configurations in extra')
    ap.add_argument('--tasks-per-rank', type=int, default=4,
                    help='meta metric: tasks per GPU per meta-iteration, run concurrently on one engine each (default 4: '
                         'measured 26.8 / 31.0 / 34.2 / 34.2 tasks/s with 1 / 3 / 4 / 6 in flight)')
    ap.add_argument('--metric', choices=['finetune', 'meta'], default='finetune',
                    help="'meta': the JSON line reports meta-tasks/s (BASELINE configs[3..4]: one task per rank per "
                         "meta-iteration, all-reduce + RAdam included); a step is then one meta-iteration")
    a = ap.parse_args(argv)
    if a.steps is None:
        a.steps = 200 if a.metric == 'finetune' else 40
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ and engine_factory is None:
        return self_launch(a, argv)

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world != a.gpus:
        raise SystemExit(f'bench.py --gpus {a.gpus} was started with WORLD_SIZE={world}: one rank per GPU is the contract')
    dist = None
    if world > 1:
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if backend == 'nccl':
            torch.cuda.set_device(local_rank)
            dist.init_process_group('nccl', device_id=torch.device(f'cuda:{local_rank}'))
        else:
            dist.init_process_group(backend)
    dev = device or f'cuda:{local_rank}'

    from eosvos_amd import _ffi, synthetic
    from eosvos_amd import engine as engine_mod
    from eosvos_amd.engine import Engine
    from eosvos_amd.meta_run import MetaTrainer

    lib_version = _ffi.load().eosvos_version().decode()
    mode = engine_mod.get_matrix_mode()
    sd = synthetic.synthetic_state('resnet50')
    lrs = synthetic.synthetic_lrs('resnet50')
    x, y = synthetic.synthetic_frames(BATCH, H, W, seed=7 + rank)
    eng = (engine_factory or Engine)('resnet50', H, W, max_batch=BATCH, device=dev)
    eng.load_model_state(sd, lrs)
    xg, yg = x.to(dev), y.to(dev)

    def barrier():
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    if a.metric == 'meta':
        return bench_meta(a, eng, dist, rank, world, sd, lrs, x, y, xg, yg, barrier, dev, mode, lib_version,
                          engine_factory or Engine)

    step = lambda: eng.finetune_step(xg, yg, sync_loss=False)
    for _ in range(max(a.warmup, 1)):
        step()                                       # (the f16x3 range guard looks at the first step after the state load)
    # the mode the TIMED steps run in: read after the warm-up, in which the guard may have moved the engine to bf16x6
    mode = mode_of(eng, engine_mod)
    guard_log0 = list(engine_mod.GUARD_LOG)
    dt = timed(step, a.steps, barrier, dist, dev)    # exactly the K steps the caller asked for, one region
    samples = [dt]
    ms_per_step = 1e3 * dt / a.steps
    value = world * a.steps / dt
    if a.dump_outputs and rank == 0:
        # what the last timed step computed: its loss, the logits of its forward pass and the weights after its update
        dump_outputs(a.dump_outputs, {'loss': eng.last_loss(), 'logits': eng.debug_tensor('logits'),
                                      'params_sample': param_sample(eng.get_params())})
    if a.full:
        last_loss = eng.finetune_step(xg, yg)       # sanity: still finite after K steps
    if mode_of(eng, engine_mod) != mode or list(engine_mod.GUARD_LOG) != guard_log0:
        raise SystemExit(f'bench.py: the matrix mode changed inside the timed region ({mode} -> {mode_of(eng, engine_mod)}, guard log '
                         f'{engine_mod.GUARD_LOG}): the line would name a mode it did not time')
    head = {
        'metric': 'finetune_iters_per_sec', 'value': value, 'unit': 'finetune_iters/s', 'n_gpus': world,
        'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': ms_per_step, 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': dtype_name(mode), 'data': 'synthetic',
        'config': {'workload': 'e-OSVOS-50 fine-tune iteration (BASELINE configs[1]): DeepLabV3+-ResNet50, '
                               f'batch {BATCH}, {H}x{W}, BCE, per-neuron-lr SGD; one (sequence, object) per rank',
                   'batch': BATCH, 'height': H, 'width': W, 'parallelism': f'replicas x{world}'},
    }
    if not a.full:
        if rank == 0:
            print(json.dumps(dict(head, extra={'matrix_mode': mode, 'guard_log': [list(g) for g in engine_mod.GUARD_LOG],
                                               'guard_enabled': engine_mod._guard_enabled(), 'lib_version': lib_version,
                                               'timed_region_samples_s': samples})), flush=True)
        eng.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    # dominant kernel: the same steps once more with HIP events around every matrix-core launch
    psteps = min(a.steps, 20)
    rows, prof_step_s = profiled_pass(eng, step, psteps)
    roofline = roofline_from(rows, psteps, mode, lib_version, BATCH, ms_per_step)
    roofline['profiled_pass_ms_per_step'] = 1e3 * prof_step_s
    if not a.no_ab and world == 1 and torch.cuda.is_available() and engine_factory is None:
        # `achieved` above times the kernel while the other stream's launches share the chip with it (weight-gradient
        # launches run beside the data-gradient chain).  The same kernel with the chip to itself: an engine without the
        # side stream, every launch in one queue.
        os.environ['EOSVOS_TUNE_PRESPLIT_INFLIGHT'] = '1'      # the SAME kernels as the two-stream step (the pre-split weight
        e1 = Engine('resnet50', H, W, max_batch=BATCH, device=dev, side_stream=False)      # gradients are for side-stream engines)
        os.environ.pop('EOSVOS_TUNE_PRESPLIT_INFLIGHT', None)
        e1.load_model_state(sd, lrs)
        step1 = lambda: e1.finetune_step(xg, yg, sync_loss=False)
        for _ in range(3):
            step1()
        rows1, s1 = profiled_pass(e1, step1, 10)
        e1.close()
        if roofline['kernel'] in rows1:
            l1, ms1, fl1 = rows1[roofline['kernel']]
            ach1 = fl1 / (ms1 * 1e-3) / 1e12
            mf1 = {k: v for k, v in rows1.items() if 'fixup' not in k}
            roofline['single_stream'] = {
                'note': 'same kernel symbol, engine built without the side stream (one queue, no launch shares the chip '
                        'with another): the quality of the kernel itself; the step is slower this way',
                'achieved': ach1, 'frac': ach1 / roofline['peak'], 'frac_of_fp32_matrix_peak': ach1 / FP32_MATRIX_PEAK,
                'avg_launch_us': 1e3 * ms1 / l1, 'ms_per_step': 1e3 * s1,
                'all_matrix_kernels_tflops': sum(v[2] for v in mf1.values()) / (sum(v[1] for v in mf1.values()) * 1e-3) / 1e12}
        # the three symbols with the largest in-step time, each beside the other stream's launches (two streams) and with the chip
        # to itself (one stream): what contention costs each of them
        top = sorted((k for k in rows if 'fixup' not in k), key=lambda k: -rows[k][1])[:3]
        roofline['top3'] = []
        for k in top:
            l2, ms2, fl2 = rows[k]
            ent = {'kernel': k, 'two_streams': {'launches_per_step': l2 / psteps, 'ms_per_step': ms2 / psteps, 'avg_launch_us': 1e3 * ms2 / l2,
                                                'tflops': fl2 / (ms2 * 1e-3) / 1e12, 'frac': fl2 / (ms2 * 1e-3) / 1e12 / roofline['peak']}}
            if k in rows1:
                l1, ms1, fl1 = rows1[k]
                ent['one_stream'] = {'launches_per_step': l1 / 10, 'ms_per_step': ms1 / 10, 'avg_launch_us': 1e3 * ms1 / l1,
                                     'tflops': fl1 / (ms1 * 1e-3) / 1e12, 'frac': fl1 / (ms1 * 1e-3) / 1e12 / roofline['peak']}
            roofline['top3'].append(ent)

    extra = {'last_loss': last_loss, 'matrix_mode': mode, 'matrix_mode_read': 'after the warm-up steps (the range guard runs in the first)',
             'guard_log': [list(g) for g in engine_mod.GUARD_LOG], 'guard_enabled': engine_mod._guard_enabled(),
             'lib_version': lib_version, 'timed_region_samples_s': samples,
             'mfma_probe_fp32_tflops': eng.mfma_probe(),
             'direct_conv_equivalent_tflops': BATCH * FLOPS_PER_FRAME_ITER / (ms_per_step * 1e-3) / 1e12,
             'conv_algorithms': 'fp32 tensors throughout; contractions on the 16-bit matrix cores: f16x3 = per-tensor power-of-two '
                                'scale, 2-way fp16 split, 3 partial products (default); bf16x6 = exact 3-way bf16 split, 6 partial '
                                'products; 6 of the 63 convs (decoder 3x3 x2, layer4 conv2 x3: Winograd F(4x4,3x3); ASPP d=6: '
                                'F(2x2,3x3)) run all three passes in the Winograd domain; direct_conv_equivalent_tflops counts '
                                '9-tap-equivalent FLOPs, roofline.* executed FLOPs'}
    # fine-tune iterations/s for the C1 / C3 shapes as well (C2 is the headline).
    n1 = min(a.steps, 60)
    step_b1 = lambda: eng.finetune_step(xg[:1], yg[:1], sync_loss=False)
    for _ in range(3):
        step_b1()
    dt1, _ = timed_median(step_b1, n1, barrier, dist, dev)
    rows_b1, _ = profiled_pass(eng, step_b1, min(n1, 10))
    fl_b1 = sum(v[2] for k, v in rows_b1.items() if 'fixup' not in k) / min(n1, 10)
    extra['c1_batch1'] = {'workload': f'BASELINE configs[0] shape: fine-tune iteration at batch 1, {H}x{W} (the reference runs it on CPU)',
                          'finetune_iters_per_sec': world * n1 / dt1, 'ms_per_step': 1e3 * dt1 / n1,
                          'whole_step_executed_tflops': fl_b1 / (dt1 / n1) / 1e12,
                          'whole_step_executed_frac': fl_b1 / (dt1 / n1) / 1e12 / matrix_peak(mode)}
    # C3: one online-adaptation round of e-OSVOS-100-OnA = 10 iterations on [first frame + 2 pseudo-labelled frames] (batch 3)
    # + the inference of the next 5 frames (evaluate.py:227-253,293-314); a round restores the first-step weights first
    xa = torch.cat([xg[:1], torch.roll(xg[:1], 12, dims=3), torch.roll(xg[:1], 16, dims=3)]).contiguous()
    ya = torch.cat([yg[:1], torch.roll(yg[:1], 12, dims=3), torch.roll(yg[:1], 16, dims=3)]).contiguous()
    x5 = torch.cat([torch.roll(xg[:1], 4 * i, dims=3) for i in range(5)])[:min(5, BATCH)].contiguous()
    eng.snapshot()

    def ona_round():
        eng.restore()
        for _ in range(10):
            eng.finetune_step(xa, ya, sync_loss=False)
        for i in range(0, 5, x5.shape[0]):
            eng.infer(x5[:min(x5.shape[0], 5 - i)])
    ona_round()
    nr = 3
    dtr, _ = timed_median(ona_round, nr, barrier, dist, dev, repeats=3)
    extra['c3_online_adaptation_round'] = {
        'workload': 'BASELINE configs[2] shape: restore first-step weights, 10 fine-tune iterations at batch 3 on [first frame + 2 '
                    f'pseudo-labelled frames], inference of 5 frames, {H}x{W}',
        'ms_per_round': 1e3 * dtr / nr, 'finetune_iters_per_sec': world * 10 * nr / dtr,
        'note': 'iterations/s over the whole round (inference and the weight restore included)'}
    eng.reset()
    configs = {'c1_b1_ms': extra['c1_batch1']['ms_per_step'], 'c1_b1_iters_per_sec': extra['c1_batch1']['finetune_iters_per_sec'],
               'c1_b1_executed_frac': extra['c1_batch1']['whole_step_executed_frac'],
               'c3_round_ms': extra['c3_online_adaptation_round']['ms_per_round']}
    if not a.no_meta:
        # meta-train metric: tasks/s with K=5 inner steps + meta frame at B=1 (configs[3..4]).  Two shapes: `--tasks-per-rank`
        # tasks in flight together on one engine each (what a GPU can do), and ONE task per rank per meta-iteration -- the
        # shape BASELINE configs[3] / [4] name (meta_batch_size = ranks; src/util/meta_run.py:39).
        # (Before the A/B extras below: they create and destroy streams, and which hardware queue a later stream lands on
        # depends on that history -- engines whose streams share a pipe lose a quarter of their rate, profiles/r03_hw_queue_sweep.txt.)
        # An extra of this line: a failure here (every rank raises alike: the only rank-dependent step is the all-reduce)
        # is recorded, not allowed to take the headline with it.
        def measure_meta(tpr, with_roofline):
            mt, mstep, _, extra_eng = meta_setup(eng, dist, world, rank, sd, lrs, dev, tpr, engine_factory or Engine)
            mstep()                                                             # warm-up
            n_it = 4 if tpr > 1 else 8
            dtm, msamples = timed_median(mstep, n_it, barrier, dist, dev, repeats=3)
            out = {'tasks_per_sec': world * tpr * n_it / dtm, 'ms_per_meta_iteration': 1e3 * dtm / n_it,
                   'config': (f'meta_batch_size={world * tpr} ({tpr} task(s) per GPU' + (' in flight on one engine each' if tpr > 1 else '') +
                              f'), 5 inner steps + 1 meta frame, batch 1, {H}x{W}'), 'timed_region_samples_s': msamples}
            mt.profile = {}
            for _ in range(2):
                mstep()
            out['phase_ms_per_meta_iteration'] = {k: v / mt.profile['iterations'] for k, v in mt.profile.items() if k != 'iterations'}
            mt.profile = None
            if with_roofline:
                mrows, _ = profiled_pass(mt.eng, mstep, 2)                      # the first engine's launches (one of `tpr` in flight)
                out['roofline'] = roofline_from(mrows, 2, mode, lib_version, 1, 1e3 * dtm / n_it)
                out['roofline']['note'] = ('HIP-event profile of the first of the engines that run tasks side by side; whole_step_* '
                                           'fields relate its FLOPs to the whole meta-iteration time and are not meaningful here')
            for e in extra_eng:
                e.close()
            return out
        tpr = a.tasks_per_rank
        try:
            m4 = measure_meta(tpr, True)
            extra['meta_tasks_per_sec'] = m4['tasks_per_sec']
            extra['meta_config'] = m4['config']
            extra['meta_phase_ms_per_meta_iteration'] = m4['phase_ms_per_meta_iteration']
            extra['meta_roofline'] = m4['roofline']
            extra['meta_timed_region_samples_s'] = m4['timed_region_samples_s']
            configs[f'meta_tasks_per_sec_tpr{tpr}'] = m4['tasks_per_sec']
            configs[f'meta_tpr{tpr}_allreduce_ms'] = m4['phase_ms_per_meta_iteration'].get('allreduce_ms')
            configs[f'meta_tpr{tpr}_outer_step_ms'] = m4['phase_ms_per_meta_iteration'].get('outer_step_ms')
            if tpr != 1:
                m1 = measure_meta(1, False)
                extra['meta_one_task_per_rank'] = m1
                configs['meta_tasks_per_sec_tpr1'] = m1['tasks_per_sec']
                configs['meta_tpr1_allreduce_ms'] = m1['phase_ms_per_meta_iteration'].get('allreduce_ms')
                configs['meta_tpr1_outer_step_ms'] = m1['phase_ms_per_meta_iteration'].get('outer_step_ms')
                eng.reset()
            if rank == 0 and world == 1 and not a.no_cpu_baseline:
                extra['meta_cpu_baseline'] = cpu_baseline_meta(sd, lrs, x[:1], y[:1], torch.flip(x[:1], dims=[3]), torch.flip(y[:1], dims=[3]))
        except Exception as exc:                                                # noqa: BLE001
            extra['meta_tasks_per_sec'] = None
            extra['meta_error'] = f'{type(exc).__name__}: {exc}'
            configs['meta_error'] = extra['meta_error']

    if not a.no_ab and world == 1:
        # same engine, same buffers, fp32-MFMA kernels (v_mfma_f32_32x32x2_f32) instead of the split kernels
        for other, key in (('bf16x6', 'bf16x6_mode_ms_per_step'), ('f32', 'fp32_mfma_mode_ms_per_step')):
            if other == mode:
                continue
            if hasattr(eng, 'set_engine_matrix_mode'):
                eng.set_engine_matrix_mode(other)
            else:
                engine_mod.set_matrix_mode(other)
            for _ in range(3):
                step()
            dto = timed(step, min(a.steps, 30), barrier, dist, dev)
            if hasattr(eng, 'set_engine_matrix_mode'):
                eng.set_engine_matrix_mode(None if mode == engine_mod.get_matrix_mode() else mode)
            else:
                engine_mod.set_matrix_mode(mode)
            eng.reset()
            extra[key] = 1e3 * dto / min(a.steps, 30)
            configs['bf16x6_ms' if other == 'bf16x6' else 'fp32_mfma_ms'] = extra[key]
    if not a.no_ab and world == 1 and torch.cuda.is_available():
        # the objects of a multi-object sequence are independent fine-tunes (evaluate.py:132): three of them in flight, one
        # engine and ONE queue each (no side stream, each launch planned for half the chip, fresh consecutive streams:
        # evaluate.run_objects_in_flight), fill the tails / small grids one iteration leaves idle.  Not the headline.
        others = []
        for _ in range(3):
            with torch.cuda.stream(torch.cuda.Stream()):
                e2 = Engine('resnet50', H, W, max_batch=BATCH, device=dev, side_stream=False)
                e2.load_model_state(sd, lrs)
                e2.set_wg_budget(256)
            others.append(e2)

        def step3():
            for e2 in others:
                with torch.cuda.stream(e2.stream):
                    e2.finetune_step(xg, yg, sync_loss=False)
        for _ in range(3):
            step3()
        n3 = min(a.steps, 30)
        dt3 = timed(step3, n3, barrier, dist, dev)
        extra['finetune_iters_per_sec_3_objects_in_flight'] = 3 * n3 / dt3
        configs['iters_per_sec_3_objects_in_flight'] = extra['finetune_iters_per_sec_3_objects_in_flight']
        for e2 in others:
            e2.close()
    if not a.no_ab and world == 1 and torch.cuda.is_available() and engine_factory is None:
        # GroupNorm(16) mode -- what the reference's shipped config selects (`cfgs/meta.yaml:76`,
        # `networks/deeplabv3plus.py:180-191`): the same iteration with GN statistics / apply / backward kernels instead of the
        # frozen-BN epilogues.  Not the headline (north_star names the frozen-BN path).
        try:
            eg = Engine('resnet50', H, W, max_batch=BATCH, device=dev, norm='gn')
            eg.load_model_state(sd, lrs)
            for key, nb in (('gn_b3_ms', BATCH), ('gn_b1_ms', 1)):
                stepg = lambda: eg.finetune_step(xg[:nb], yg[:nb], sync_loss=False)
                for _ in range(3):
                    stepg()
                ng = min(a.steps, 30)
                dtg = timed(stepg, ng, barrier, dist, dev)
                configs[key] = 1e3 * dtg / ng
                eg.reset()
            configs['gn_matrix_mode'] = mode_of(eg, engine_mod)
            extra['groupnorm_mode'] = {'b3_ms_per_step': configs['gn_b3_ms'], 'b1_ms_per_step': configs['gn_b1_ms'],
                                       'vs_frozen_bn_b3': configs['gn_b3_ms'] / ms_per_step, 'matrix_mode': configs['gn_matrix_mode']}
            eg.close()
        except Exception as exc:                                                # noqa: BLE001
            configs['gn_error'] = f'{type(exc).__name__}: {exc}'
    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline_finetune(sd, lrs, x, y)
    if mode_of(eng, engine_mod) != mode:
        raise SystemExit(f'bench.py: the headline engine left the matrix mode it was timed in ({mode} -> {mode_of(eng, engine_mod)})')
    if rank == 0:
        print(json.dumps(dict(head, roofline=roofline, cpu_baseline=cpu, configs=configs, extra=extra)), flush=True)
    eng.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
