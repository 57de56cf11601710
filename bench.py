#!/usr/bin/env python
"""bench.py -- images/sec of the MVAE train step on N MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload mnist|fashionmnist|celeba|celeba19]
                    [--batch B_PER_GPU] [--dump-outputs DIR] [--full]

One "step" = zero_grad -> the three (celeba19: 20+M) ELBO terms forward -> backward ->
[gradient all-reduce] -> Adam, on a synthetic random-pixel / random-label batch that is already
resident in HBM.  Default workload = BASELINE.json configs[1]: MNIST MVAE,
n-latents 64, batch 512 per GPU.  Weak scaling: the per-GPU batch is fixed as N grows.

A plain run does only what the headline needs: set up and capture, SETTLE_STEPS untimed steps, W untimed warm-up
steps, exactly K timed steps, and ONE JSON line (rank 0) with the contract fields and `ms_per_step` (one timed step).
--dump-outputs DIR  after the timed steps, writes what the last timed step computed (`elbo` as replay() returns it,
                    the parameters, their gradients and the buffers after it) as DIR/<name>.npy, float32 / float64,
                    a fixed seeded sample where the whole would pass DUMP_BUDGET_BYTES; inputs are seeded, so two
                    builds can be compared output for output.
--full              everything else the line has carried, measured as before (it takes ~90 s on the default workload):
  step_distribution -- the settle pass becomes max(50, K) steps with one HIP event between consecutive steps,
                   ms_per_step_median / p90 come from it,
Besides the contract fields a --full line carries
  roofline      -- the dominant GEMM-shaped call of the step, IN SITU: every launcher is bracketed by HIP
                   events on the launch stream (profiler.KernelProfile) and eager single-stream steps are
                   enqueued behind a spin kernel that outlasts the host's enqueue time, so an interval
                   is the call's kernel(s) plus its launch boundary, with the caches as the previous kernel
                   left them.  ``hot_cache_reissue`` = the same call re-issued back to back in a hipGraph
                   (round 1's figure), ``conv_kernels`` / ``all_gemm_kernels`` = the in-situ aggregates,
                   ``top_hbm_kernel`` = the HBM-bound kernel with the most time, ``traffic`` = HBM-side bytes
                   per launch from the committed PMC table (profiles/r06_traffic.json) -- like ``rocprof_avg_us`` a
                   QUOTED figure: ``committed_profiles`` says on which code it was collected, ``profile_stale`` is
                   true when that is not this tree's kernel sources; ``other_workloads`` = the `also` list, compact,
  cpu_baseline  -- the oracle (CPU restatement of the reference step, kind "port") timed on the
                   host cores of this box on a bounded sample of the same workload; ``cores`` = intra-op
                   threads used (fastest of a few counts), ``host`` = nproc + CPU model,
                   ``cfg0_mnist_b128`` = BASELINE configs[0], ``elbo_delta`` = HIP vs oracle on one step,
  dist          -- (N > 1 or --force-dp) ms/step of the same launch path with the collectives switched off and
                   the difference (= exposed communication); world size, backend + RCCL version, the
                   all-reduce-of-ones check, transport and bucket sizes are on every data-parallel line,
  also          -- (MNIST at its default batch only) the CelebA B=256 step: images/sec and the fp32-MFMA
                   roofline of its conv kernels, the figure north_star's 40 % target is about.
Flags beyond the contract: --no-extras (with --full: step_distribution / dist only), --no-graph, --force-dp
(world-1 run through the data-parallel launch path), --force-tiling wm,wn[,splits] (tuning build of the library).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEFAULT_BATCH = {'mnist': 512, 'fashionmnist': 1024, 'celeba': 256, 'celeba19': 256}
LAMBDA_LABEL = {'mnist': 50.0, 'fashionmnist': 50.0, 'celeba': 10.0, 'celeba19': 10.0}
N_LATENTS = {'mnist': 64, 'fashionmnist': 64, 'celeba': 100, 'celeba19': 100}
LR = {'mnist': 1e-3, 'fashionmnist': 1e-3, 'celeba': 1e-4, 'celeba19': 1e-4}
# untimed steps between the capture and the warm-up of a plain run (the first tens of replays after a capture are slower)
SETTLE_STEPS = 50
# --dump-outputs writes at most this much (the contract allows 64 MB); larger models are sampled, see dump_outputs()
DUMP_BUDGET_BYTES = 60 << 20


def synthetic(kind, batch, seed, device):
    g = torch.Generator().manual_seed(seed)
    if kind in ('mnist', 'fashionmnist'):
        image = torch.rand(batch, 1, 28, 28, generator=g)
        label = torch.randint(0, 10, (batch,), generator=g)
    else:
        image = torch.rand(batch, 3, 64, 64, generator=g)
        label = torch.randint(0, 2, (batch, 18), generator=g).float()
    return image.to(device), label.to(device)


def build(kind, batch, device, world, seed=0, faithful_bn_stats=True):
    import mvae_amd
    from mvae_amd.optim import FusedAdam
    torch.manual_seed(seed)
    model = getattr(mvae_amd, kind).model.MVAE(N_LATENTS[kind]).to(device).train()
    model.finalize()
    if kind == 'celeba19':
        from mvae_amd.engine import Celeba19Step
        eng = Celeba19Step(model, batch, 1.0, LAMBDA_LABEL[kind], approx_m=1, seed=1234,
                           faithful_bn_stats=faithful_bn_stats)
    else:
        from mvae_amd.engine import BimodalStep
        eng = BimodalStep(model, batch, 1.0, LAMBDA_LABEL[kind], seed=1234)
    opt = FusedAdam(model.parameters(), lr=LR[kind], grad_scale=1.0 / world)
    return model, eng, opt


def annealing(step, total=2000):
    return min(1.0, float(step + 1) / total)


def dump_outputs(out_dir, model, elbo):
    """What the last timed step handed its caller: ``elbo`` as replay() / step() returned it, every parameter, its
    gradient (the gradient arena: ``p.grad`` may be None between steps) and every buffer, as ``<name>.npy`` (float32;
    integer buffers as float64).  If the whole would pass DUMP_BUDGET_BYTES, arrays of up to 4096 elements stay whole and
    every larger one keeps the same fraction of its elements at sorted positions drawn by a generator seeded with 0 --
    fixed by the shapes alone, so two builds of the project sample the same elements."""
    import numpy as np
    arrays = [('elbo', elbo)]
    params = dict(model.named_parameters())
    for name, p in params.items():
        arrays.append(('param.' + name, p))
        arena = getattr(p, '_arena', None)
        arrays.append(('grad.' + name, arena.grad_view(p) if arena is not None else p.grad))
    for name, b in model.state_dict().items():          # state_dict() flushes the lazily counted num_batches_tracked
        if name not in params:
            arrays.append(('buffer.' + name, b))
    arrays = [(n, t.detach().cpu().numpy()) for n, t in arrays if t is not None]
    arrays = [(n, a.astype(np.float32 if a.dtype.kind == 'f' and a.itemsize <= 4 else np.float64)) for n, a in arrays]
    small = sum(a.nbytes for _, a in arrays if a.size <= 4096)
    large = sum(a.nbytes for _, a in arrays if a.size > 4096)
    frac = min(1.0, (DUMP_BUDGET_BYTES - small) / float(max(large, 1)))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays:
        if frac < 1.0 and a.size > 4096:
            k = max(1, int(a.size * frac))
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, k, replace=False))]
        np.save(os.path.join(out_dir, name + '.npy'), a)


def timed_run(kind, batch, steps, warmup, device, world, rank, use_graph=True, force_dp=False, faithful_bn_stats=True,
              full=True, dump_dir=None):
    import torch.distributed as dist
    model, eng, opt = build(kind, batch, device, world, faithful_bn_stats=faithful_bn_stats)
    dp = None
    if world > 1 or force_dp:
        from mvae_amd.parallel import DataParallel
        dp = DataParallel(model, eng)
    batches = [synthetic(kind, batch, 1234 + rank * 100 + i, device) for i in range(4)]
    if use_graph:
        eng.capture(opt, batches[0][0].shape[1:], batches[0][1], comm=dp)

        def one(i):
            img, lbl = batches[i % 4]
            return eng.replay(img, lbl, annealing(i))
    else:
        def one(i):
            img, lbl = batches[i % 4]
            elbo = eng.step(img, lbl, annealing(i))
            if dp is not None:
                dp.finish(opt)
            else:
                opt.step()
            return elbo
    def timed(n, first):
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for i in range(n):
            last = one(first + i)
        if world > 1:
            # drain this rank's queue first: the step's collectives run on the library's own RCCL communicator, the
            # barrier on torch.distributed's -- two communicators should not have kernels in flight at once
            torch.cuda.synchronize(device)
            dist.barrier()
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = t.item()
        return dt, last

    # Order of the passes: the per-step DISTRIBUTION pass (median of >= 50 steps, one HIP event between consecutive
    # steps on the launch stream) runs FIRST, the contract region -- W untimed warm-up steps, then exactly K timed steps
    # between two barrier + synchronize fences -- behind it.  Measured on one box, x3: with the contract region first a
    # `--steps 20 --warmup 5` run (what the driver passes: a 6-ms region right after the capture) reads MNIST 0.287-0.294 ms
    # where `--steps 100 --warmup 20` reads 0.274-0.276 -- the first tens of replays after a capture are slower (clocks,
    # caches, first launches of a new graph).  The events of the distribution pass are not inside the region `value` comes from.
    # At world > 1 the same number of steps runs untimed (no events): N = 1 and N > 1 lines are taken in the same state.
    # Without `full` (a plain run) the pass is SETTLE_STEPS untimed steps, no events: only what keeps the region out of
    # the post-capture transient.
    n_pre = max(50, steps) if full else SETTLE_STEPS
    dist_steps = None
    if full and device.type == 'cuda' and world == 1:
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_pre + 1)]
        torch.cuda.synchronize(device)
        for i in range(n_pre):
            evs[i].record()
            one(i)
        evs[n_pre].record()
        torch.cuda.synchronize(device)
        per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(n_pre))
        dist_steps = {'steps': n_pre, 'ms_per_step_median': round(per[n_pre // 2], 4), 'ms_per_step_p10': round(per[n_pre // 10], 4),
                      'ms_per_step_p90': round(per[(n_pre * 9) // 10], 4), 'ms_per_step_max': round(per[-1], 4),
                      'how': 'separate pass BEFORE the timed region: one HIP event between consecutive steps on the launch stream'}
    else:
        for i in range(n_pre):
            one(i)
    for i in range(warmup):
        one(n_pre + i)
    dt, elbo = timed(steps, n_pre + warmup)
    if dump_dir is not None and rank == 0:
        dump_outputs(dump_dir, model, elbo)
    info = None
    if dp is not None:
        sizes = [(hi - lo) * 4 for lo, hi in dp.buckets.ranges]
        info = {'bucket_bytes': sizes, 'transport': dp.transport}
    if dp is not None and full:
        # what the data-parallel exchange costs: the same launch path with the collectives switched off
        # (replicas diverge from here on -- nothing is measured after this)
        dp.buckets.launch = lambda k: None
        dp.buckets.wait = lambda k=None: None
        if use_graph and dp.in_graph:
            # the collectives are nodes of the captured graph: capture the same step once more without them
            eng.capture(opt, batches[0][0].shape[1:], batches[0][1], comm=dp)
        n2 = max(5, steps // 2)
        dt_off, _ = timed(n2, n_pre + warmup + steps)
        info.update({'ms_per_step_without_collectives': round(dt_off / n2 * 1e3, 4),
                     'exposed_comm_ms_per_step': round((dt / steps - dt_off / n2) * 1e3, 4)})
    loss = float(elbo[-1].item())
    return dt, loss, (model, eng, opt, batches, info, dist_steps)


def _spin_cycles_per_second():
    """Calibrate torch.cuda._sleep (a spin kernel): cycles of its argument per second of GPU time."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0.record(); torch.cuda._sleep(20_000_000); e1.record()
    torch.cuda.synchronize()
    return 20_000_000 / (e0.elapsed_time(e1) * 1e-3)


def roofline_from_profile(eng, opt, batches, n_steps=3, kind=None):
    """Which launches make up a step, and how fast each runs IN the step.

    Every launcher of kernels.py is bracketed by a pair of HIP events on the launch stream and tagged with
    its algorithmic work; ``n_steps`` eager single-stream steps are enqueued BEHIND a spin kernel that
    outlasts the host's enqueue time, so when the GPU reaches them the queue is full: an interval holds
    the kernel(s) of one call plus its launch boundary, no host gap, and the caches are in the state the
    step's previous kernel left them (in-situ).  achieved = algorithmic flops of the call / that interval,
    averaged over the calls of the three steps.  For the dominant call the old hot-cache figure (the same
    call re-issued 20x inside a hipGraph on the same operands) is reported next to it, labelled."""
    from mvae_amd.profiler import GEMM_COSTS, HBM_PEAK_GBS, MFMA_F32_PEAK_TFLOPS, KernelProfile
    streams = (eng.side, eng.wg_main, eng.wg_side)
    eng.side = eng.wg_main = eng.wg_side = None          # single stream: one ordered queue
    try:
        eng.step(batches[0][0], batches[0][1], 0.5); opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.step(batches[0][0], batches[0][1], 0.5); opt.step()
        host_s = time.perf_counter() - t0                # host time to enqueue one eager step
        torch.cuda.synchronize()
        spin_s = 3.0 * host_s * n_steps + 0.010          # the event pairs make the enqueue ~1.5x slower
        for attempt in range(4):
            with KernelProfile() as prof:
                torch.cuda._sleep(int(_spin_cycles_per_second() * spin_s))
                spin_done = torch.cuda.Event()
                spin_done.record()
                for i in range(n_steps):
                    eng.step(batches[i % 4][0], batches[i % 4][1], 0.5)
                    opt.step()
                queue_was_full = not spin_done.query()   # the spin kernel outlasted the whole enqueue
            if queue_was_full:
                break
            torch.cuda.synchronize()
            spin_s *= 2.0                                # a host stall (allocator, table ring) drained the queue: again
        rows = prof.summary()
        gemm = [r for r in rows if r['name'] in GEMM_COSTS]
        for r in gemm:
            r['tflops'] = r['flops'] / (r['ms_avg'] * 1e-3) / 1e12
        gemm.sort(key=lambda r: -r['ms_total'])
        dom = gemm[0]
        hot_ms = prof.steady_state_ms(dom['name'], dom['key'])
        hbm = [r for r in rows if r['name'] not in GEMM_COSTS and r['bytes'] > 0]
        top = max(hbm, key=lambda r: r['ms_total']) if hbm else None
        if top is not None:
            top['gbs'] = top['bytes'] / (top['ms_avg'] * 1e-3) / 1e9
    finally:
        eng.side, eng.wg_main, eng.wg_side = streams
    flops_step = sum(r['flops'] * r['calls'] for r in gemm) / n_steps
    ms_gemm = sum(r['ms_total'] for r in gemm) / n_steps
    traffic, traffic_stamp = traffic_for(dom['name'], dom['key'])
    rocprof_us, rocprof_stamp = rocprof_us_for(kind, dom['name'], dom['key'])
    roof = {
        'bound': 'mfma', 'kernel': '%s %s' % (dom['name'], dom['key']),
        'achieved': round(dom['tflops'], 3), 'peak': MFMA_F32_PEAK_TFLOPS, 'unit': 'TFLOP/s',
        'frac': round(dom['tflops'] / MFMA_F32_PEAK_TFLOPS, 4), 'traffic': traffic,
        'avg_launch_ms': round(dom['ms_avg'], 5), 'algorithmic_flops_per_launch': dom['flops'],
        # the same call in the committed rocprofv3 kernel trace of one eager step (tools/step_by_shape.py: kernel
        # durations only, no launch boundary) and the fraction that gives -- the figure a reader can recompute from profiles/
        'rocprof_avg_us': rocprof_us,
        'calls_per_step': dom['calls'] / n_steps,
        'timing': 'in-situ: HIP event pairs on the launch stream around every call of %d eager single-stream '
                  'steps enqueued behind a spin kernel (queue full, no host gap inside an interval; an interval '
                  'includes the launch boundary)' % n_steps,
        'hot_cache_reissue': {'avg_launch_ms': round(hot_ms, 5),
                              'tflops': round(dom['flops'] / (hot_ms * 1e-3) / 1e12, 3),
                              'frac': round(dom['flops'] / (hot_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                              'timing': 'the same call re-issued 20x in a hipGraph on the same operands (L2/MALL hot)'},
        'all_gemm_kernels': {'tflops': round(flops_step / (ms_gemm * 1e-3) / 1e12, 3),
                             'frac': round(flops_step / (ms_gemm * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                             'ms_per_step': round(ms_gemm, 4), 'gflop_per_step': round(flops_step / 1e9, 3)},
    }
    if roof['rocprof_avg_us']:
        roof['rocprof_frac'] = round(dom['flops'] / (roof['rocprof_avg_us'] * 1e-6) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4)
    # `frac`, `achieved`, `avg_launch_ms` are measured in THIS run; `traffic`, `rocprof_avg_us`, `rocprof_frac` are quoted from
    # committed tables: where they were collected, and whether the kernel sources have changed since
    roof['committed_profiles'] = {'traffic': traffic_stamp, 'rocprof': rocprof_stamp}
    roof['profile_head'] = (rocprof_stamp or traffic_stamp or {}).get('head')
    stamps = [st for st in (rocprof_stamp, traffic_stamp) if st]
    # true: a quoted table was collected on other kernel sources than this tree's; null: nothing is quoted for this call
    roof['profile_stale'] = any(st['stale'] for st in stamps) if stamps else None
    conv = [r for r in gemm if r['name'].startswith('conv')]
    if conv:
        fl = sum(r['flops'] * r['calls'] for r in conv) / n_steps
        ms = sum(r['ms_total'] for r in conv) / n_steps
        roof['conv_kernels'] = {'tflops': round(fl / (ms * 1e-3) / 1e12, 3),
                                'frac': round(fl / (ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                                'ms_per_step': round(ms, 4), 'gflop_per_step': round(fl / 1e9, 3)}
    if top is not None:
        roof['top_hbm_kernel'] = {'kernel': ('%s %s' % (top['name'], top['key'])).strip(), 'gbs': round(top['gbs'], 1),
                                  'frac': round(top['gbs'] / HBM_PEAK_GBS, 4), 'avg_launch_ms': round(top['ms_avg'], 5),
                                  'algorithmic_bytes_per_launch': top['bytes'],
                                  'bytes': 'SURVEY 8(d): Adam 28 B/param, BatchNorm fwd 3 / bwd 5 transfers, BCE 2*rows*P*4 (+ the '
                                           'gradient written), PoE per its formula (mvae_amd/profiler.py HBM_COSTS)'}
    roof['queue_full_during_enqueue'] = bool(queue_was_full)
    roof['launches_per_step'] = sum(r['calls'] for r in rows) / n_steps
    roof['top_kernels'] = [{'kernel': '%s %s' % (r['name'], r['key']), 'ms_per_step': round(r['ms_total'] / n_steps, 4),
                            'calls_per_step': r['calls'] / n_steps, 'tflops': round(r['tflops'], 2)} for r in gemm[:6]]
    return roof


# The two committed tables a line may quote.  They are measured in a builder's GPU session, NOT in the run that prints
# the line, so every figure taken from them carries the code they were collected on (mvae_amd.profiler.code_stamp: hash
# of the kernel sources + the git head of that session) and `stale` when the hash is not this tree's (the
# fields were silent look-ups, and fell back to tables of earlier rounds).  No fallback: a call this round's table does
# not hold reads null.
TRAFFIC_FILE = os.path.join(ROOT, 'profiles', 'r06_traffic.json')
BY_SHAPE_FILE = os.path.join(ROOT, 'profiles', 'r06_by_shape.json')


def _stamp_verdict(stamp):
    from mvae_amd.profiler import code_stamp
    if not stamp:
        return {'head': None, 'csrc_sha16': None, 'stale': True}
    return {'head': stamp.get('head'), 'csrc_sha16': stamp.get('csrc_sha16'),
            'stale': stamp.get('csrc_sha16') != code_stamp()['csrc_sha16']}


def rocprof_us_for(kind, name, key):
    """(average rocprofv3 duration (us) of the call's kernels in the committed per-(call, shape) table of this workload's
    step, the table's code stamp) -- profiles/r06_by_shape.json, made by tools/step_by_shape.py on the GPU box; (None, None)
    if not traced."""
    try:
        with open(BY_SHAPE_FILE) as f:
            table = json.load(f)
    except (IOError, ValueError):
        return None, None
    ent = table.get(kind, {}).get('%s %s' % (name, key))
    if ent is None:
        return None, None
    return ent['rocprof_avg_us'], dict(_stamp_verdict(table.get('_meta', {}).get(kind)), file='profiles/r06_by_shape.json')


def module_surface(kind, batch, device, steps=20, warmup=5):
    """The loop a reference user keeps (mnist/train.py:197-219, celeba/train.py:190-212): three ``model()`` calls, three
    ``elbo_loss`` calls, ``backward()``, ``optimizer.step()`` on the drop-in nn.Modules -- eager, autograd, no fused engine,
    no graph -- with torch.optim.Adam and with FusedAdam.  Not `value`: how far the module surface is from the headline."""
    import mvae_amd
    import mvae_amd.functional as MF
    from mvae_amd.optim import FusedAdam
    out = {'what': 'reference-shaped loop on the drop-in modules: 3 model() + 3 elbo_loss + backward + optimizer.step(), eager',
           'steps': steps, 'batch': batch}
    image, label = synthetic(kind, batch, 4321, device)
    for opt_name in ('torch.optim.Adam', 'FusedAdam'):
        torch.manual_seed(0)
        model = getattr(mvae_amd, kind).model.MVAE(N_LATENTS[kind]).to(device).train()
        model.finalize()
        opt = (torch.optim.Adam if opt_name == 'torch.optim.Adam' else FusedAdam)(model.parameters(), lr=LR[kind])
        lam = LAMBDA_LABEL[kind]

        def step(i):
            opt.zero_grad()
            beta = annealing(i)
            if kind == 'celeba':
                r1, r2, r3 = model(image, label), model(image), model(attrs=label)
                kw = dict(lambda_image=1.0, lambda_attrs=lam, annealing_factor=beta)
                elbo = MF.elbo_loss_attrs
            else:
                r1, r2, r3 = model(image, label), model(image), model(text=label)
                kw = dict(lambda_image=1.0, lambda_text=lam, annealing_factor=beta)
                elbo = MF.elbo_loss_label
            loss = (elbo(r1[0], image, r1[1], label, r1[2], r1[3], **kw) + elbo(r2[0], image, None, None, r2[2], r2[3], **kw)
                    + elbo(None, None, r3[1], label, r3[2], r3[3], **kw))
            loss.backward()
            opt.step()
            return loss
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for i in range(steps):
            loss = step(warmup + i)
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        out[opt_name] = {'ms_per_step': round(dt / steps * 1e3, 3), 'images_per_sec': round(batch * steps / dt, 1),
                         'final_loss': round(float(loss.item()), 3)}
        if opt_name == 'FusedAdam':
            # the SAME body (three model() calls, three elbo_loss calls, backward, step -- nothing restructured) handed to
            # mvae_amd.capture_step: forward, autograd backward and optimizer in ONE hipGraph, no host work per launch
            def body(img, lbl, beta):
                opt.zero_grad()
                if kind == 'celeba':
                    r1, r2, r3 = model(img, lbl), model(img), model(attrs=lbl)
                    kw = dict(lambda_image=1.0, lambda_attrs=lam, annealing_factor=beta)
                    elbo = MF.elbo_loss_attrs
                else:
                    r1, r2, r3 = model(img, lbl), model(img), model(text=lbl)
                    kw = dict(lambda_image=1.0, lambda_text=lam, annealing_factor=beta)
                    elbo = MF.elbo_loss_label
                total = (elbo(r1[0], img, r1[1], lbl, r1[2], r1[3], **kw) + elbo(r2[0], img, None, None, r2[2], r2[3], **kw)
                         + elbo(None, None, r3[1], lbl, r3[2], r3[3], **kw))
                total.backward()
                opt.step()
                return total
            try:
                cap = mvae_amd.capture_step(body, (image, label, 1.0), model=model, optimizer=opt)
                for i in range(warmup):
                    cap(image, label, annealing(i))
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                for i in range(steps):
                    loss = cap(image, label, annealing(warmup + i))
                torch.cuda.synchronize(device)
                dt = time.perf_counter() - t0
                out['FusedAdam + capture_step'] = {'ms_per_step': round(dt / steps * 1e3, 3),
                                                   'images_per_sec': round(batch * steps / dt, 1),
                                                   'final_loss': round(float(loss.item()), 3),
                                                   'what': 'mvae_amd.capture_step(body, ...): the unchanged body as one hipGraph'}
                del cap
            except Exception as e:       # reported, never fatal for the line
                out['FusedAdam + capture_step'] = {'error': '%s: %s' % (type(e).__name__, e)}
        del model, opt
    return out


def traffic_for(name, key):
    """HBM bytes per launch of the call from the committed rocprofv3 --pmc passes (FETCH_SIZE and
    WRITE_SIZE in separate runs, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950;
    tools/traffic_probe.py + tools/rocpd_summary.py --pmc).  None when that call was not probed."""
    try:
        with open(TRAFFIC_FILE) as f:
            ent = json.load(f).get('%s %s' % (name, key))
    except (IOError, ValueError):
        ent = None
    if ent is None:
        return None, None
    return ent['hbm_bytes_per_launch'], dict(_stamp_verdict(ent.get('collected_on')), file='profiles/r06_traffic.json')


def elbo_delta(kind, batch=32):
    """BASELINE.json's metric is 'images/sec ...; ELBO delta vs CPU ref': one step of the HIP engine and
    of the CPU oracle at identical weights, inputs and noise; relative difference of the summed ELBO and
    the worst relative gradient error (part of the cpu_baseline leg: the oracle is the checker)."""
    import numpy as np
    import mvae_amd
    from oracle import models as OM, steps as OS
    cls, d = OM.MODELS[kind]
    oracle = OM.fill_parameters(cls(d), 17).train()
    model = getattr(mvae_amd, kind).model.MVAE(d)
    model.load_state_dict(oracle.state_dict())
    model.cuda().train()
    image, label = OS.synthetic_batch(kind, batch, seed=18)
    torch.manual_seed(19)
    lam = LAMBDA_LABEL[kind]
    if kind == 'celeba19':
        from mvae_amd.engine import Celeba19Step, sample_subsets
        combos = sample_subsets(np.random.RandomState(3), 19, 1)
        terms = OS.celeba19_terms(combos)
        noise = OS.draw_celeba19_noise(batch, d, terms)
        total, _, _ = OS.celeba19_step(oracle, image, label, terms, noise, 1.0, lam, 0.5)
        eng = Celeba19Step(model, batch, 1.0, lam, approx_m=1)
        got = eng.step(image.cuda(), label.cuda(), 0.5, noise=noise, combos=combos)[-1].item()
    else:
        from mvae_amd.engine import BimodalStep
        noise = OS.draw_bimodal_noise(batch, d, has_dropout=(kind == 'celeba'))
        total, _, _ = OS.bimodal_step(oracle, kind, image, label, noise, 1.0, lam, 0.5)
        eng = BimodalStep(model, batch, 1.0, lam)
        got = eng.step(image.cuda(), label.cuda(), 0.5, noise=noise)[-1].item()
    total.backward()
    og = dict(oracle.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    # gradients that are zero in exact arithmetic -- the bias of a Linear that feeds a training-mode
    # BatchNorm (celeba/model.py:148-151,175-181) -- are judged on the scale of the largest gradient;
    # every other parameter on its own magnitude (same rule as tests/util.py:ZERO_GRAD_PARAMS)
    zero_grad = ('attrs_encoder.net.0.bias', 'attrs_encoder.net.3.bias', 'attrs_decoder.net.0.bias',
                 'attrs_decoder.net.3.bias', 'attrs_decoder.net.6.bias') if kind == 'celeba' else ()
    worst = 0.0
    for name, p in model.named_parameters():
        ref = og[name].grad
        scale = max(ref.abs().max().item(), 1e-2 * gmax if name in zero_grad else 0.0, 1e-30)
        worst = max(worst, (p.grad.cpu() - ref).abs().max().item() / scale)
    ref = total.item()
    return {'hip': round(got, 4), 'cpu': round(ref, 4), 'rel': float('%.3e' % (abs(got - ref) / abs(ref))),
            'worst_gradient_rel': float('%.3e' % worst), 'batch': batch, 'tolerance': 1e-4}


def host_description():
    """nproc and CPU model of this box (north_star: 'core count stated')."""
    model = 'unknown'
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.lower().startswith('model name'):
                    model = line.split(':', 1)[1].strip()
                    break
    except IOError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    return {'nproc': os.cpu_count() or 1, 'usable_cpus': usable, 'cpu_model': model}


def cpu_baseline(kind, batch, budget_s=15.0, with_delta=True, threads=None):
    """The oracle (a port of the reference's step to explicit-noise torch CPU ops) on this box's
    host cores: full steps incl. Adam on the same synthetic workload, bounded by ~budget_s.
    ``cores`` = the intra-op threads actually used (the fastest of a few counts: torch's CPU kernels do
    not scale to every core of a big host); the box itself is described under ``host``."""
    from oracle import models as OM, steps as OS
    import numpy as np
    host = host_description()
    cores = host['usable_cpus']
    cls, d = OM.MODELS[kind]
    torch.manual_seed(0)
    model = cls(d).train()
    opt = torch.optim.Adam(model.parameters(), lr=LR[kind])
    image, label = OS.synthetic_batch(kind, batch, 1234)
    rng = np.random.RandomState(7)

    def one_step():
        if kind == 'celeba19':      # 20 + 1 terms, a fresh random subset per step (approx-m 1)
            from mvae_amd.engine import sample_subsets
            terms = OS.celeba19_terms(sample_subsets(rng, 19, 1))
            noise = OS.draw_celeba19_noise(batch, d, terms)
        else:
            noise = OS.draw_bimodal_noise(batch, d, has_dropout=(kind == 'celeba'))
        t0 = time.perf_counter()
        opt.zero_grad()
        if kind == 'celeba19':
            total, _, _ = OS.celeba19_step(model, image, label, terms, noise, 1.0, LAMBDA_LABEL[kind], 0.5)
        else:
            total, _, _ = OS.bimodal_step(model, kind, image, label, noise, 1.0, LAMBDA_LABEL[kind], 0.5)
        total.backward()
        opt.step()
        return time.perf_counter() - t0

    # thread count: the MEDIAN of three timed steps per candidate (after one warm step) -- one step per candidate
    # made the choice, and with it the reported rate, swing by +-60 % between runs
    probe = (16, 32) if kind == 'celeba19' else (8, 16, 32, 64)      # a celeba19 step is ~20 model() calls
    cands = [t for t in probe if t <= cores] or [cores]
    if threads is not None:          # a second batch size of the same model: keep the main run's choice
        cands = [int(threads)]
    n_probe = 2 if kind == 'celeba19' else 3
    probed = {}
    for th in cands:
        torch.set_num_threads(th)
        one_step()                                   # warm this thread count
        probed[th] = sorted(one_step() for _ in range(n_probe))
    # the probe picks two finalists; the figure reported is the better SUSTAINED rate of the two (each runs half of
    # the budget): on a 256-CPU host a thread count can win three probe steps and then run 3x slower for 200
    order = sorted(cands, key=lambda th: probed[th][len(probed[th]) // 2])
    finalists = order[:2]
    runs = {}
    for th in finalists:
        torch.set_num_threads(th)
        times = []
        while sum(times) < budget_s / len(finalists) or len(times) < 3:
            times.append(one_step())
            if len(times) >= 200:
                break
        runs[th] = times
    threads = max(finalists, key=lambda th: len(runs[th]) / sum(runs[th]))
    torch.set_num_threads(threads)
    times = runs[threads]
    n, t_total = len(times), sum(times)
    ts = sorted(times)
    out = {'value': round(batch * n / t_total, 2), 'unit': 'images/sec', 'cores': threads, 'kind': 'port',
           'threads': threads, 'host': host,
           'best_step_images_per_sec': round(batch / ts[0], 2),
           'median_step_images_per_sec': round(batch / ts[n // 2], 2),
           'thread_probe_median_ms': {str(th): round(v[len(v) // 2] * 1e3, 2) for th, v in probed.items()},
           'sustained_images_per_sec_by_threads': {str(th): round(batch * len(r) / sum(r), 2) for th, r in runs.items()},
           'sample': '%d full train steps (fwd+bwd+Adam) of the %s oracle at batch %d, torch %s CPU, '
                     '%d intra-op threads (the better sustained rate of the two lowest probe medians, %d steps '
                     'each, among %s) on a %d-CPU host' % (
                         n, kind, batch, torch.__version__, threads, n_probe, cands, host['nproc'])}
    out['note'] = ('the hosts of this pool are shared 256-CPU boxes: the same code has read 8.3 K and 15.2 K images/sec on '
                   'MNIST in two runs -- a stated baseline beside the GPU figure, never the target')
    if with_delta:
        out['elbo_delta'] = elbo_delta(kind, 8 if kind == 'celeba19' else 32)
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(n, argv=None):
    """``python bench.py --gpus N`` with no launcher around it: re-run this script as N ranks, one per GPU, under
    ``torch.distributed.run`` (127.0.0.1 rendezvous on a free port) and hand back its exit code.  The ranks find
    WORLD_SIZE in their environment and take the launched path."""
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)]
    cmd += list(sys.argv[1:] if argv is None else argv)
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # RCCL across processes needs dmabuf IPC on this driver
    return subprocess.call(cmd, env=env)


def dist_check(backend, device):
    """World size, backend and an all-reduce of ones -- proof that N real ranks are talking."""
    import torch.distributed as dist
    ones = torch.ones(1, device=device)
    dist.all_reduce(ones)
    info = {'world_size': dist.get_world_size(), 'backend': dist.get_backend(), 'allreduce_of_ones': ones.item()}
    if backend == 'nccl':
        info['rccl_version'] = '.'.join(str(v) for v in torch.cuda.nccl.version())
    return info


def extra_workload(kind, batch, steps, warmup, device, use_graph, cpu_budget_s):
    """One more workload on the default line's ``also`` list: throughput, in-situ roofline, CPU oracle beside it."""
    import gc
    dt, loss, st = timed_run(kind, batch, steps, warmup, device, 1, 0, use_graph=use_graph)
    ent = {'workload': '%s MVAE train step, n-latents %d, batch %d, 1 GPU' % (kind, N_LATENTS[kind], batch),
           'value': round(batch * steps / dt, 1), 'unit': 'images/sec', 'steps': steps, 'warmup': warmup,
           'ms_per_step': round(dt / steps * 1e3, 3), 'final_loss': round(loss, 3),
           'step_distribution': st[5],
           'roofline': roofline_from_profile(st[1], st[2], st[3], kind=kind),
           'cpu_baseline': cpu_baseline(kind, batch, budget_s=cpu_budget_s)}
    if kind == 'celeba':
        ent['module_surface'] = module_surface(kind, batch, device)
    if kind == 'celeba19':
        # SURVEY Appendix B-4 made explicit: what reproducing the reference's BatchNorm side effects costs.  The line
        # above (and every parity test) is the 'reference' mode; this is `celeba19/train.py --bn-stats loss-bearing`
        # (the 18 image decodes nobody reads are skipped; ELBO and gradients unchanged, running statistics differ).
        del st
        gc.collect()
        torch.cuda.empty_cache()
        dt2, loss2, st = timed_run(kind, batch, steps, warmup, device, 1, 0, use_graph=use_graph, faithful_bn_stats=False)
        ent['bn_stats_loss_bearing'] = {
            'ms_per_step': round(dt2 / steps * 1e3, 3), 'value': round(batch * steps / dt2, 1), 'unit': 'images/sec',
            'what': "celeba19/train.py --bn-stats loss-bearing: image decoder run for the 2 + M terms with an image loss only; "
                    "NOT the reference's BatchNorm running statistics -- never the headline"}
    del st
    gc.collect()
    torch.cuda.empty_cache()
    return ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--workload', default='mnist', choices=sorted(DEFAULT_BATCH))
    ap.add_argument('--batch', type=int, default=None, help='per-GPU batch')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--force-tiling', default=None,
                    help='tuning aid: wm,wn,splits,kwaves forwarded to mvae_debug_set_tiling / _kwaves')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip roofline / cpu_baseline / also')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need: step distribution, roofline, cpu_baseline, '
                         'module_surface, the other workloads (`also`), exposed communication')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help="write the last timed step's outputs (ELBO terms, parameters, gradients, buffers) as DIR/<name>.npy")
    ap.add_argument('--force-dp', action='store_true',
                    help='tuning aid: run the data-parallel launch path (3 graphs + RCCL) even at world size 1')
    ap.add_argument('--backend', default='nccl', choices=('nccl', 'gloo'),
                    help='gloo: CPU-only check of the launcher (implies --dist-check); the train step needs nccl = RCCL')
    ap.add_argument('--dist-check', action='store_true',
                    help='only bring the N ranks up, all-reduce ones, print the line with the dist block, exit')
    args = ap.parse_args()
    if args.backend == 'gloo':
        args.dist_check = True
    if args.gpus < 1:
        raise SystemExit('--gpus must be >= 1')

    # multi-process GPU work on this driver needs dmabuf IPC (without it RCCL / cross-process tensor sharing fail with
    # hipIpcGetMemHandle: invalid argument); the HSA runtime reads it when the process first touches the GPU
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # the documented command, no launcher: bring the N ranks up ourselves
        if args.backend == 'nccl' and torch.cuda.device_count() < args.gpus:
            raise SystemExit('bench.py --gpus %d: only %d GPU(s) visible (torch.cuda.device_count()); refusing to '
                             'report a %d-GPU figure' % (args.gpus, torch.cuda.device_count(), args.gpus))
        sys.exit(spawn_ranks(args.gpus))

    if args.force_tiling:
        # the overrides exist only in the tuning build of the library
        os.environ['MVAE_HIP_LIB'] = os.path.join(ROOT, 'multimodal-vae-public_amd', 'libmvae_hip_tuning.so')
        from mvae_amd import _lib
        wm, wn, sp, kw = (int(v) for v in args.force_tiling.split(','))
        _lib.lib().mvae_debug_set_tiling(wm, wn, sp)
        _lib.lib().mvae_debug_set_kwaves(kw)

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: the launcher and the flag disagree' % (args.gpus, world))
    from mvae_amd import launch
    supervise = os.environ.get('MVAE_BENCH_SUPERVISE', '1')      # '0': ranks run directly; 'force': also at world size 1 (tests)
    if (world > 1 or (supervise == 'force' and 'WORLD_SIZE' in os.environ)) and launch.WORKER_ENV not in os.environ \
            and supervise != '0':
        # A launched rank is a SUPERVISOR (mvae_amd/launch.py): it runs each gradient-exchange transport in a child
        # process under a wall-clock budget -- a hung collective is killed with its process, not waited for -- and the
        # ranks agree per attempt whether it succeeded everywhere.  The first transport that completes on every rank
        # gives the line; `dist.fallbacks_tried` says what was given up on.  This process never touches the GPU.
        line, tried = launch.supervise(os.path.abspath(__file__), sys.argv[1:])
        if rank == 0:
            if line is None:
                line = {'metric': 'images/sec (MVAE train step)', 'value': None, 'unit': 'images/sec', 'n_gpus': world,
                        'steps': args.steps, 'warmup': args.warmup, 'higher_is_better': True, 'scaling': 'weak',
                        'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
                        'config': {'workload': '%s MVAE train step' % args.workload, 'parallelism': 'dp%d' % world},
                        'dist': {'world_size': world, 'transport': None, 'fallbacks_tried': tried},
                        'note': 'every gradient-exchange transport failed or timed out on at least one rank'}
            print(json.dumps(line))
            sys.stdout.flush()
        sys.exit(0 if (rank != 0 or line.get('value') is not None or args.dist_check) else 1)
    transport = os.environ.get(launch.TRANSPORT_ENV)
    on_gpu = args.backend == 'nccl'
    if on_gpu:
        if torch.cuda.device_count() <= local:
            raise SystemExit('rank %d: LOCAL_RANK %d but only %d GPU(s) visible' % (rank, local, torch.cuda.device_count()))
        device = torch.device('cuda', local)
        torch.cuda.set_device(device)
    else:
        device = torch.device('cpu')
    dist_info = None
    if world > 1 or args.force_dp or args.dist_check:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if world == 1:
            os.environ.setdefault('MASTER_PORT', str(_free_port()))
            os.environ.setdefault('RANK', '0'); os.environ.setdefault('WORLD_SIZE', '1')
        if on_gpu:
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group('gloo')
        if transport == 'fake-raise':       # tests of the supervisor chain (tests/test_parallel_cpu.py)
            raise SystemExit('fake-raise transport: this attempt fails on purpose')
        if transport == 'fake-hang' and rank == world - 1:
            while True:                     # one rank never arrives at the collective below: its peers block in it
                time.sleep(1.0)
        dist_info = dist_check(args.backend, device)
        if dist_info['world_size'] != args.gpus or dist_info['allreduce_of_ones'] != float(args.gpus):
            raise SystemExit('--gpus %d but the process group has %d ranks (all-reduce of ones = %g)' % (
                args.gpus, dist_info['world_size'], dist_info['allreduce_of_ones']))
    kind = args.workload
    batch = args.batch or DEFAULT_BATCH[kind]
    if args.dist_check:
        if rank == 0:
            print(json.dumps({'metric': 'images/sec (MVAE train step)', 'value': None, 'n_gpus': world,
                              'dist': dist_info, 'note': 'launcher check only: no step was run'}))
        import torch.distributed as dist
        dist.destroy_process_group()
        return

    dt, loss, state = timed_run(kind, batch, args.steps, args.warmup, device, world, rank,
                                use_graph=not args.no_graph, force_dp=args.force_dp, full=args.full,
                                dump_dir=args.dump_outputs)
    out = {
        'metric': 'images/sec (MVAE train step)', 'value': round(world * batch * args.steps / dt, 1),
        'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': round(dt / args.steps * 1e3, 4), 'higher_is_better': True, 'scaling': 'weak',
        'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
        'runtime_env': {k: os.environ[k] for k in ('GPU_MAX_HW_QUEUES',) if k in os.environ},   # only if the caller set it
        'config': {'workload': '%s MVAE train step, n-latents %d, batch %d per GPU' % (kind, N_LATENTS[kind], batch),
                   'global_batch': world * batch, 'parallelism': 'dp%d' % world,
                   'launch': 'eager' if args.no_graph else 'hipGraph replay', 'final_loss': round(loss, 3),
                   'value_from': 'the contract region: --warmup untimed steps, then exactly --steps steps between two barrier + '
                                 'synchronize fences (max over ranks).  It runs BEHIND a separate pass of %s steps (%s), so that a '
                                 'short region is not taken in the first milliseconds after the graph capture' % (
                                     ('max(50, steps)', 'at N = 1 with one HIP event per step: ms_per_step_median / p90 come '
                                      'from that pass') if args.full else (str(SETTLE_STEPS), 'untimed'))},
    }
    if state[4] is not None:
        out['dist'] = dict(dist_info, **state[4])
        if rank == 0 and 'exposed_comm_ms_per_step' in out['dist']:
            sys.stderr.write('[bench] world %d over %s (RCCL %s); all-reduce of ones = %g; buckets %s bytes; '
                             'exposed communication %.4f ms/step\n' % (
                                 out['dist']['world_size'], out['dist']['backend'], out['dist'].get('rccl_version'),
                                 out['dist']['allreduce_of_ones'], out['dist']['bucket_bytes'],
                                 out['dist']['exposed_comm_ms_per_step']))
    if state[5] is not None:
        out.update({k: state[5][k] for k in ('ms_per_step_median', 'ms_per_step_p90')})
        out['step_distribution'] = state[5]
    if rank == 0 and world == 1 and args.full and not args.no_extras and not args.force_dp:
        model, eng, opt, batches = state[:4]
        out['roofline'] = roofline_from_profile(eng, opt, batches, kind=kind)
        out['cpu_baseline'] = cpu_baseline(kind, batch)
        if kind in ('mnist', 'celeba'):
            out['module_surface'] = module_surface(kind, batch, device)
        if kind == 'mnist':
            # BASELINE.json configs[0]: the reference's own CPU-runnable case, mnist batch 128 -- the CPU rate and the
            # ELBO / gradient delta of the HIP engine against it at that exact batch
            out['cpu_baseline']['cfg0_mnist_b128'] = cpu_baseline('mnist', 128, budget_s=6.0, with_delta=False,
                                                                   threads=out['cpu_baseline']['threads'])
            out['cpu_baseline']['cfg0_mnist_b128']['elbo_delta'] = elbo_delta('mnist', 128)
        if kind == 'mnist' and args.batch is None:
            # the other three GPU configurations of BASELINE.json at their per-GPU batch, bounded: configs[2]
            # FashionMNIST 1024, configs[3] CelebA 256 (the conv stack north_star's 40 % MFMA target is about),
            # configs[4] CelebA-19 256 / approx-m 1 (the N = 1 anchor of the weak-scaling curve)
            import gc
            del state, model, eng, opt, batches
            gc.collect()
            torch.cuda.empty_cache()
            ug = not args.no_graph
            out['also'] = [extra_workload('celeba', 256, 30, 5, device, ug, 10.0),
                           extra_workload('fashionmnist', 1024, 30, 5, device, ug, 8.0),
                           extra_workload('celeba19', 256, 15, 3, device, ug, 8.0)]
            # the same, compact, where a record that keeps only the contract objects still holds it (the
            # driver's record dropped `also`); also on stderr as one short JSON line
            out['roofline']['other_workloads'] = [
                {'workload': e['workload'].split(' MVAE')[0], 'ms_per_step': e['ms_per_step'],
                 'ms_per_step_median': (e.get('step_distribution') or {}).get('ms_per_step_median'),
                 'images_per_sec': e['value'], 'kernel': e['roofline']['kernel'], 'frac': e['roofline']['frac'],
                 'rocprof_frac': e['roofline'].get('rocprof_frac'), 'profile_stale': e['roofline'].get('profile_stale'),
                 'conv_kernels_frac': (e['roofline'].get('conv_kernels') or {}).get('frac')} for e in out['also']]
            sys.stderr.write(json.dumps({'also_summary': out['roofline']['other_workloads']}) + '\n')
    if rank == 0:
        print(json.dumps(out))
    if world > 1 or args.force_dp:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
