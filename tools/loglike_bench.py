#!/usr/bin/env python
"""The chunk loop of ``mvae_amd.log_likelihood`` (csrc/loglike.hip: mvae_iw_draw + mvae_iw_accumulate around the decoders
and the loss-row kernels) against a composition of what exists without the two kernels: a torch element-wise draw and
density ratio per chunk, the SAME decoders and loss-row kernels, the [K, B] log-weights stored and reduced by
``torch.logsumexp`` on the GPU.  One process, one model, alternating blocks, so both paths see the same box.

    python tools/loglike_bench.py [--steps 200] [--block 10] > profiles/loglike.txt

``model.infer`` runs once, outside the timed region (it is the same in both paths).  A call is timed with a host clock
around work that ends in a device synchronise, after a warm-up (the form of tools/gru_seq_bench.py).  The gate is the
project's own: the new path's median must not be above the baseline's median by more than the baseline's interquartile
range."""
import argparse
import math
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (('mnist', 64, 1000), ('celeba', 8, 512))       # (experiment, B, K); D = the experiment's default


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def baseline_loop(LL, model, kind, mu, logvar, image, label, score, n_samples, Kc):
    """torch element-wise draw + density ratio, stored [K, B] log-weights, torch.logsumexp."""
    B, D = mu.shape
    logw = torch.empty(n_samples, B, dtype=torch.float32, device=mu.device)
    std = torch.exp(0.5 * logvar)
    for k0 in range(0, n_samples, Kc):
        n = min(Kc, n_samples - k0)
        eps = torch.randn(n, B, D, dtype=torch.float32, device=mu.device)
        z = mu + std * eps
        lw = (0.5 * eps * eps - 0.5 * z * z + 0.5 * logvar).sum(dim=2)
        for rows, rps in LL.score_rows(model, kind, z, image, label, score):
            lw = lw - rows.view(n, B, rps).sum(dim=2)
        logw[k0:k0 + n] = lw
    return torch.logsumexp(logw, dim=0) - math.log(n_samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--chunk-rows', type=int, default=4096)
    ap.add_argument('--score', type=str, default='image,label')
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd
    from mvae_amd import loglike as LL
    from oracle import models as OM, steps as OS
    assert torch.cuda.is_available(), 'loglike_bench needs the GPU'
    dev = torch.device('cuda', 0)
    score = tuple(s for s in args.score.split(',') if s)
    print('# %s, torch %s; log_likelihood chunk loop, score %s given image+label, chunk_rows %d, eval mode, %d calls per '
          'path in alternating blocks of %d, ms per call' % (torch.cuda.get_device_name(0), torch.__version__,
                                                             '+'.join(score), args.chunk_rows, args.steps, args.block))
    ok = True
    for kind, B, n_samples in CONFIGS:
        cls, D = OM.MODELS[kind]
        model = getattr(mvae_amd, kind).model.MVAE(D)
        model.load_state_dict(OM.fill_parameters(cls(D), 3).state_dict())
        model.to(dev).eval()
        image, label = OS.synthetic_batch(kind, B, seed=1)
        image, label = LL._prepare(model, kind, image, label)
        Kc = max(1, args.chunk_rows // B)
        with torch.no_grad():
            mu, logvar = LL.infer(model, kind, image, label, ('image', 'label'))

            def call(new, i):
                if new:
                    return LL.chunk_loop(model, kind, mu, logvar, image, label, score, n_samples, Kc, seed=i)
                return baseline_loop(LL, model, kind, mu, logvar, image, label, score, n_samples, Kc)

            def run(new, n, i0):
                out = []
                for i in range(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = call(new, i0 + i)
                    torch.cuda.synchronize()
                    out.append((time.perf_counter() - t0) * 1e3)
                assert torch.isfinite(res).all().item()
                return out, res

            run(False, 15, 0); run(True, 15, 0)             # warm-up: code objects, allocator
            t_base, t_new = [], []
            for b in range(args.steps // args.block):
                t, r_base = run(False, args.block, b * args.block)
                t_base += t
                t, r_new = run(True, args.block, b * args.block)
                t_new += t
        mb, b1, b3 = quartiles(t_base)
        mn, n1, n3 = quartiles(t_new)
        passed = mn <= mb + (b3 - b1)
        ok = ok and passed
        print('%s  B = %d  K = %d  D = %d  (%d chunk(s) of %d samples)' % (kind, B, n_samples, D, -(-n_samples // Kc), min(Kc, n_samples)))
        print('  torch draw + ratio + logsumexp  median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mb, b1, b3, b3 - b1))
        print('  iw_draw + iw_accumulate         median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mn, n1, n3, n3 - n1))
        print('  ratio new / baseline %.3f; not above the baseline median by more than its IQR: %s'
              % (mn / mb, 'yes' if passed else 'no'))
        # different noise streams: the two estimates agree statistically, not bit for bit
        print('  estimates (mean over the data): baseline %.3f, new %.3f' % (r_base.mean().item(), r_new.mean().item()))
    print('gate: %s' % ('passed' if ok else 'FAILED'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
