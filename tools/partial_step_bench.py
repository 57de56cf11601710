#!/usr/bin/env python
"""The ragged train step of weak supervision (``partial.PartialStep``) against a dense step that masks instead of
compacting, forward + backward without the optimizer, per paired fraction:

    ragged   ``PartialStep.step``: host plan + one upload, encoders on the rows that have the modality, one ragged PoE
             launch, each decoder once on its contiguous slice, indexed losses
    dense    (lives only here) the same modules on ALL rows of all three terms: both encoders on B rows, the dense PoE
             launches on [3, B, D] with the noise drawn inside the forward, each decoder on its two terms' 2 B rows,
             ``_BceRowsFn`` / ``_CeRowsFn`` on targets repeated once per workload (outside the timed region), and zero
             row coefficients on the inactive (term, row) pairs
    fused    at fraction 1.0 only: ``BimodalStep.step`` (the fused engine, eager, no graph)

    python tools/partial_step_bench.py [--repeats 3] [--calls 30] > profiles/partial_step.txt

Workloads: MNIST B = 512 and FashionMNIST B = 1024, D = 64, synthetic batches, models at their random initialisation,
``--unpaired-labels drop`` semantics: a fraction f of the rows observes image and label (three terms), the rest the image
alone (one term).  Term rows R = B (1 + 2 f) against the dense 3 B; decoder rows B (1 + f) + 2 f B against 4 B.  A call is
timed with a host clock around work that ends in a device synchronise, after a warm-up of every arm; the arms alternate
call by call in one process; the measurement is repeated ``--repeats`` times and the spread of the repeats' medians is
reported.  A record, not a gate: no default depends on the outcome."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (('mnist', 512), ('fashionmnist', 1024))
FRACTIONS = (1.0, 0.5, 0.1, 0.01)
D, LAM_I, LAM_L, BETA = 64, 1.0, 50.0, 0.5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, repeats, calls, warm=5):
    """{name: the repeats' medians} of the callables, alternating call by call."""
    for fn in fns.values():
        for _ in range(warm):
            timed(fn)
    meds = {name: [] for name in fns}
    for _ in range(repeats):
        times = {name: [] for name in fns}
        for _ in range(calls):
            for name, fn in fns.items():
                times[name].append(timed(fn))
        for name in fns:
            meds[name].append(statistics.median(times[name]))
    return meds


def spread(meds):
    return 'median %.3f  (repeats %s; spread %.3f)' % (statistics.median(meds), ' '.join('%.3f' % m for m in meds),
                                                        max(meds) - min(meds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=30)
    args = ap.parse_args()
    import mvae_amd
    from mvae_amd import functional as F, kernels as K, partial as P
    from mvae_amd.engine import BimodalStep
    dev = torch.device('cuda')

    class DensePoEDrawFn(torch.autograd.Function):
        """``functional.PoEFn`` with the noise drawn inside the forward launch (``mvae_poe_fwd_draw``), as the ragged arm
        draws it: the dense arm pays no separate noise launch."""

        @staticmethod
        def forward(ctx, cfg, *heads):
            masks, noise, seed, counter, variant, d = cfg
            T, Bn = masks.numel(), heads[0].shape[0]
            mu = torch.empty(T, Bn, d, dtype=torch.float32, device=heads[0].device)
            lv, z = torch.empty_like(mu), torch.empty_like(mu)
            kl = torch.empty(T, Bn, dtype=torch.float32, device=mu.device)
            K.poe_fwd_draw([h[:, :d] for h in heads], [h[:, d:] for h in heads], masks, noise, seed, counter, 0, mu, lv, z,
                           kl, variant)
            ctx.cfg = (masks, noise, variant, d)
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(mu, lv, *heads)
            return mu, lv, z, kl

        @staticmethod
        def backward(ctx, dmu, dlv, dz, dkl):
            masks, noise, variant, d = ctx.cfg
            mu, lv = ctx.saved_tensors[:2]
            heads = ctx.saved_tensors[2:]
            grads = [torch.empty_like(h) for h in heads]

            def c(t):
                return None if t is None else t.contiguous()
            K.poe_bwd([h[:, :d] for h in heads], [h[:, d:] for h in heads], masks, noise, mu, lv, c(dz), c(dmu), c(dlv),
                      c(dkl), [g[:, :d] for g in grads], [g[:, d:] for g in grads], variant)
            return (None,) + tuple(grads)
    print('# python tools/partial_step_bench.py --repeats %d --calls %d' % (args.repeats, args.calls))
    print('# %s, torch %s, libmvae_hip.so; forward + backward of one step, no optimizer; arms alternating call by call; ms'
          % (torch.cuda.get_device_name(0), torch.__version__))
    for kind, B in WORKLOADS:
        torch.manual_seed(1)
        model = importlib.import_module('mvae_amd.%s.model' % kind).MVAE(D).to(dev).train()
        model.finalize()
        g = torch.Generator().manual_seed(2)
        image = torch.rand(B, 1, 28, 28, generator=g).to(dev)
        label_full = torch.randint(0, 10, (B,), generator=g).to(dev)
        order = np.random.RandomState(3).permutation(B)
        masks_dev = torch.tensor(P.TERM_MASKS, dtype=torch.int32, device=dev)
        # constant per workload, so outside the timed region: the dense arm's repeated targets, noise buffer and counter
        image2 = image.reshape(B, -1).repeat(2, 1)
        label2 = label_full.repeat(2)
        dense_noise = torch.empty(3, B, D, dtype=torch.float32, device=dev)
        dense_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        ragged_step = P.PartialStep(model, LAM_I, LAM_L, seed=4)
        fused_step = BimodalStep(model, B, LAM_I, LAM_L, seed=4)
        print('%s: B = %d, D = %d' % (kind, B, D))
        for f in FRACTIONS:
            is_paired = np.zeros(B, dtype=bool)
            is_paired[order[:int(round(f * B))]] = True
            present, paired = P.batch_flags(is_paired, 'drop')
            pl = P.plan(present, paired)
            label = label_full.masked_fill(torch.from_numpy(~is_paired).to(dev), -1)
            # dense arm: per-(term, row) coefficients, zero where the term is inactive (decoder row order: two terms of B rows)
            act = torch.from_numpy(pl.slot >= 0).to(dev).float()                   # [3, B]: joint, image, label
            w_bce = (torch.cat([act[0], act[1]]) * (LAM_I / B)).contiguous()
            w_ce = (torch.cat([act[0], act[2]]) * (LAM_L / B)).contiguous()
            w_kl = (act * (BETA / B)).contiguous()

            def ragged():
                ragged_step.step(image, label, BETA, present=present, paired=paired)

            def dense():
                for p in model.parameters():
                    p.grad = None
                heads = (model.image_encoder.heads(image), model.label_encoder.heads(label_full))
                _, _, z, kl = DensePoEDrawFn.apply((masks_dev, dense_noise, 4, dense_counter, model.POE_VARIANT, D), *heads)
                K.counter_add(dense_counter, 1)
                xi = model.image_decoder(z[:2].reshape(2 * B, D)).reshape(2 * B, -1)
                xl = model.label_decoder(torch.cat([z[0], z[2]]))
                bce = F._BceRowsFn.apply(xi, image2)
                ce = F._CeRowsFn.apply(xl, label2)
                ((bce * w_bce).sum() + (ce * w_ce).sum() + (kl * w_kl).sum()).backward()

            def fused():
                fused_step.step(image, label_full, BETA)

            fns = {'ragged': ragged, 'dense': dense}
            if f == 1.0:
                fns['fused'] = fused
            meds = alternate(fns, args.repeats, args.calls)
            dec_rows = (pl.image_slice[1] - pl.image_slice[0]) + (pl.label_slice[1] - pl.label_slice[0])
            print('  paired fraction %.2f: term rows R = %d of %d (%.3f; (1 + 2f) / 3 = %.3f), decoder rows %d of %d (%.3f)'
                  % (f, pl.R, 3 * B, pl.R / (3.0 * B), (1 + 2 * f) / 3, dec_rows, 4 * B, dec_rows / (4.0 * B)))
            for name in fns:
                print('    %-7s %s' % (name, spread(meds[name])))
            r, d = statistics.median(meds['ragged']), statistics.median(meds['dense'])
            sp = max(max(m) - min(m) for m in (meds['ragged'], meds['dense']))
            print('    ragged / dense %.3f; ragged ahead of dense beyond the spread (%.3f): %s'
                  % (r / d, sp, 'yes' if d - r > sp else 'no'))
            if f == 1.0:
                print('    ragged / fused (eager, no graph) %.3f' % (r / statistics.median(meds['fused'])))
    print('# not measured: the step with the optimizer, the captured (hipGraph) fused step, keep mode, other batch sizes, '
          'real data, whole epochs, and the two new kernels on their own or under a profiler (no bytes/s).')
    return 0


if __name__ == '__main__':
    sys.exit(main())
