#!/usr/bin/env python
"""Two measurements behind the vision experiment, each with its two sides alternated in one process:

  kernel  one segmented launch (mvae_bce_multi_fwd with fused gradient + the group-sum launch that forms the means)
          against the path without it: six mvae_bce_rowsum_fwd launches with fused gradient + the six accumulating
          group-sum launches that add them up (what functional.elbo_loss_* does per row vector) -- at R = 50 (one ELBO
          term) and R = 350 (the seven terms of a step) with the vision segment sizes.  The bare launches without the
          group sums are reported too.
  step    vision.train.train_step (eager, seven model() calls) against vision.train.fused_step at B = 50, D = 250,
          both with FusedAdam.

    python tools/vision_step_bench.py > profiles/vision_step.txt

Times come from device events: a kernel sample is a pair of events around ``--inner`` back-to-back evaluations (so the
figure is the steady-state cost in a stream, launch gaps included), a step sample a pair around one step.  Every shape is
warmed up first.  Bytes of the kernel table: logits read + dlogits written, targets counted once; the HBM peak is
MI355X's 8.0 TB/s (specification; a float4 copy reaches 6.3)."""
import argparse
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

VISION_P = (12288, 4096, 4096, 4096, 12288, 12288)
HBM_PEAK = 8.0e12


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner        # ms


def alternate(sides, samples, block, inner):
    out = {name: [] for name in sides}
    for _ in range(samples // block):
        for name, fn in sides.items():
            out[name] += [timed(fn, inner) for _ in range(block)]
    return out


def kernel_table(args):
    from mvae_amd import kernels as K
    dev = torch.device('cuda', 0)
    B = 50
    print('## kernel: segmented BCE row sums, P = %s (49,152 per row), us per evaluation, %d samples of %d evaluations '
          'per side in alternating blocks of %d' % (VISION_P, args.samples, args.inner, args.block))
    verdicts = []
    for R in (50, 350):
        g = torch.Generator().manual_seed(R)
        xs = [(3 * torch.randn(R, P, generator=g)).to(dev) for P in VISION_P]
        ts = [torch.rand(B, P, generator=g).to(dev) for P in VISION_P]
        ds = [torch.empty_like(x) for x in xs]
        drow = torch.full((R // B,), 1.0 / B, device=dev)
        drow6 = drow / 6
        coef = torch.full((R // B,), 1.0 / B, device=dev)
        coef6 = coef / 6
        rows = torch.empty(R, device=dev)
        rows6 = [torch.empty(R, device=dev) for _ in VISION_P]
        out = torch.empty(R // B + 1, device=dev)
        G = R // B
        segs = [(x, t, d, 1.0 / 6) for x, t, d in zip(xs, ts, ds)]

        def multi_bare():
            K.bce_multi_fwd(segs, rows, drow=drow, rows_per_group=B)

        def six_bare():
            for x, t, d, r in zip(xs, ts, ds, rows6):
                K.bce_rowsum_fwd(x, t, r, drow=drow6, dlogits=d, rows_per_group=B, target_rows=B)

        def multi():
            multi_bare()
            K.group_sums(rows, coef, out[:G], out[G:], G, B)

        def six():
            six_bare()
            for i, r in enumerate(rows6):
                K.group_sums(r, coef6, out[:G], out[G:], G, B, accumulate=(i > 0))

        sides = {'one segmented launch + 1 group sum': multi, 'six launches + 6 group sums': six,
                 'one segmented launch, bare': multi_bare, 'six launches, bare': six_bare}
        six(); ref = out.clone(); multi()
        err = ((out - ref).abs().max() / ref.abs().max()).item()
        for fn in sides.values():
            timed(fn, args.inner)
        t = alternate(sides, args.samples, args.block, args.inner)
        nbytes = 2 * R * sum(VISION_P) * 4 + B * sum(VISION_P) * 4
        print('R = %d (%.1f MB: logits read + dlogits written, targets once); means of the two paths differ by %.1e relative'
              % (R, nbytes / 1e6, err))
        stats = {}
        for name, v in t.items():
            m, q1, q3 = quartiles([x * 1e3 for x in v])
            stats[name] = (m, q3 - q1)
            print('  %-36s median %8.2f us  quartiles %8.2f .. %8.2f  (IQR %.2f)  %5.2f TB/s = %4.1f%% of HBM peak'
                  % (name, m, q1, q3, q3 - q1, nbytes / (m * 1e-6) / 1e12, 100 * nbytes / (m * 1e-6) / HBM_PEAK))
        (ma, _), (mb, sb) = stats['one segmented launch + 1 group sum'], stats['six launches + 6 group sums']
        ok = ma <= mb + sb
        verdicts.append(ok)
        print('  ratio segmented / six launches %.3f; not slower beyond the spread (median <= median + IQR of the six): %s'
              % (ma / mb, 'PASS' if ok else 'FAIL'))
    return all(verdicts)


def step_table(args):
    from mvae_amd.optim import FusedAdam
    from mvae_amd.vision import model as VM, train as VT
    dev = torch.device('cuda', 0)
    B, D = args.batch, args.n_latents
    models = [VM.MVAE(D), VM.MVAE(D)]
    models[1].load_state_dict(models[0].state_dict())
    for m in models:
        m.to(dev).train()
    opts = [FusedAdam(m.parameters(), lr=1e-4) for m in models]
    g = torch.Generator().manual_seed(5)
    batches = [tuple(torch.rand(B, VM.N_CHANNELS[k], 64, 64, generator=g).to(dev) for k in VM.MODALITIES) for _ in range(2)]
    count = [0, 0]

    def eager():
        count[0] += 1
        return VT.train_step(models[0], opts[0], batches[count[0] % 2], 0.5)

    def fused():
        count[1] += 1
        return VT.fused_step(models[1], opts[1], batches[count[1] % 2], 0.5)

    sides = {'train_step (eager, seven model() calls)': eager, 'fused_step (batched)': fused}
    for fn in sides.values():
        for _ in range(args.warmup):
            loss, _ = fn()
        assert torch.isfinite(loss).item()
    t = alternate(sides, args.steps, args.step_block, 1)
    print('## step: vision train step, B = %d, D = %d, FusedAdam, ms per step, %d steps per side in alternating blocks of %d '
          'after %d warm-up steps each' % (B, D, args.steps, args.step_block, args.warmup))
    stats = {}
    for name, v in t.items():
        m, q1, q3 = quartiles(v)
        stats[name] = (m, q3 - q1)
        print('  %-40s median %8.3f ms  quartiles %8.3f .. %8.3f  (IQR %.3f)' % (name, m, q1, q3, q3 - q1))
    (me, se), (mf, sf) = stats['train_step (eager, seven model() calls)'], stats['fused_step (batched)']
    faster = mf + max(se, sf) < me
    print('  ratio fused / eager %.3f; fused faster beyond the spread (median + larger IQR < eager median): %s'
          % (mf / me, 'YES' if faster else 'NO'))
    return faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=60)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--n-latents', type=int, default=250)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--step-block', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--only', choices=('kernel', 'step'), default=None)
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    assert torch.cuda.is_available(), 'vision_step_bench needs the GPU'
    print('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    if args.only in (None, 'kernel'):
        kernel_table(args)
    if args.only in (None, 'step'):
        step_table(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
