#!/usr/bin/env python
"""The chunk loop of ``vision.loglike.log_likelihood`` -- six marginals and the joint from one pass of the six decoders --
in three arms that share the model, the data and the decoders:

    fused   one ``iw_score_multi`` per chunk (K24, csrc/loglike_multi.hip: a score launch and a fold launch)
    rows    the kernels that were there before: six single-segment ``bce_multi_fwd`` and seven ``iw_accumulate``
    torch   plain torch around the same decoders: a torch draw and density ratio, ``binary_cross_entropy_with_logits``
            row sums, the [7, K, B] log-weights stored and reduced by ``torch.logsumexp``

    python tools/vision_loglike_bench.py [--repeats 3] [--calls 20] > profiles/vision_loglike.txt
    python tools/vision_loglike_bench.py --score-only         # the score-and-fold share of the fused arm alone
    rocprofv3 --kernel-trace --stats ... -- python tools/vision_loglike_bench.py --score-only --calls 20

Default size: ``n_latents`` 250, synthetic data, B = 8, K = 512, all six modalities scored and given.  ``get_params`` runs
once, outside the timed region (the same in every arm).  A call is one whole chunk loop, timed with a host clock around
work that ends in a device synchronise, after a warm-up of every shape; the arms alternate call by call; the whole
measurement is repeated ``--repeats`` times and the spread of the repeats' medians is reported.  "score and fold" times
the arms on the stored logits of one chunk, the decoders excluded.  The bytes of the score launch are the logits plus
the targets, from the shapes."""
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

ARMS = ('fused', 'rows', 'torch')
CHUNK_ROWS = (1024, 2048, 4096)
HBM_PEAK = 8.0e12           # bytes/s, MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured with a float4 copy)


def torch_score(lw, segs, logw, k0):
    """The torch arm's share of a chunk: BCE row sums and the S + 1 log-weight rows into logw [S + 1, K, B]."""
    n, B = lw.shape
    joint = lw
    for s, (logits, target) in enumerate(segs):
        t = target.unsqueeze(0).expand(n, B, -1).reshape(n * B, -1)
        rec = torch.nn.functional.binary_cross_entropy_with_logits(logits, t, reduction='none').sum(dim=1).view(n, B)
        logw[s, k0:k0 + n] = lw - rec
        joint = joint - rec
    logw[len(segs), k0:k0 + n] = joint


def torch_loop(model, mu, logvar, targets, score, n_samples, Kc):
    B, D = mu.shape
    logw = torch.empty(len(score) + 1, n_samples, B, dtype=torch.float32, device=mu.device)
    std = torch.exp(0.5 * logvar)
    for k0 in range(0, n_samples, Kc):
        n = min(Kc, n_samples - k0)
        eps = torch.randn(n, B, D, dtype=torch.float32, device=mu.device)
        z = mu + std * eps
        lw = (0.5 * eps * eps - 0.5 * z * z + 0.5 * logvar).sum(dim=2)
        zr = z.view(n * B, D)
        segs = [(getattr(model, name + '_decoder')(zr).reshape(n * B, -1).contiguous(), targets[name]) for name in score]
        torch_score(lw, segs, logw, k0)
    return torch.logsumexp(logw, dim=1) - math.log(n_samples)


def timed(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, res


def spread(meds):
    return '%.3f  (repeats %s; spread %.3f)' % (statistics.median(meds), ' '.join('%.3f' % m for m in meds),
                                                 max(meds) - min(meds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per arm, shape and repeat')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--n-samples', type=int, default=512)
    ap.add_argument('--n-latents', type=int, default=250)
    ap.add_argument('--score-only', action='store_true', help='only the fused arm on stored logits (for a kernel trace)')
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    from mvae_amd import _lib, kernels as K
    from mvae_amd.vision import loglike as VL, model as VM
    assert torch.cuda.is_available(), 'vision_loglike_bench needs the GPU'
    dev = torch.device('cuda', 0)
    B, n_samples = args.batch, args.n_samples
    torch.manual_seed(0)
    model = VM.MVAE(args.n_latents)
    model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    data = {m: torch.rand(B, VM.N_CHANNELS[m], 64, 64, generator=g).to(dev) for m in VM.MODALITIES}
    score = VM.MODALITIES
    targets = {m: data[m].reshape(B, -1) for m in score}
    P_total = sum(t.shape[1] for t in targets.values())
    print('# %s, torch %s, %s; vision log_likelihood, B = %d, K = %d, D = %d, score and given: all six, per_modality; '
          '%d repeats of %d calls per arm, arms alternating call by call; ms'
          % (torch.cuda.get_device_name(0), torch.__version__, os.path.basename(_lib.lib()._name), B, n_samples,
             args.n_latents, args.repeats, args.calls))
    with torch.no_grad():
        mu, logvar = model.get_params(**data)
        mu, logvar = mu.contiguous(), logvar.contiguous()
        for chunk_rows in CHUNK_ROWS:
            Kc = min(max(1, chunk_rows // B), n_samples)
            n_chunks = -(-n_samples // Kc)
            R = Kc * B
            nbytes = 4 * P_total * (R + B)
            print('chunk_rows %d: %d chunk(s) of %d samples = %d rows; the score launch reads %d bytes per chunk '
                  '(logits + targets)' % (chunk_rows, n_chunks, Kc, R, nbytes))

            # ---- score and fold alone, on the stored logits of one chunk
            z = torch.empty(Kc, B, args.n_latents, device=dev)
            lw = torch.empty(Kc, B, device=dev)
            K.iw_draw(mu, logvar, z, lw, seed=3, counter_dev=torch.zeros(1, dtype=torch.int64, device=dev))
            segs = [(getattr(model, m + '_decoder')(z.view(R, -1)).reshape(R, -1).contiguous(), targets[m]) for m in score]
            rows = torch.empty(len(score), R, device=dev)
            out = torch.empty(len(score) + 1, B, device=dev)
            logw = torch.empty(len(score) + 1, Kc, B, device=dev)
            state = VL.fresh_state(len(score) + 1, B, dev)      # folded into again and again: no reset in the timed call

            def score_arm(arm):
                if arm == 'torch':
                    torch_score(lw, segs, logw, 0)
                    return torch.logsumexp(logw, dim=1) - math.log(Kc)
                VL.SCORERS[arm](lw, segs, state, out, Kc, rows)
                return out
            arms = ('fused',) if args.score_only else ARMS
            for arm in arms:
                timed(lambda: score_arm(arm), 5)
            meds = {arm: [] for arm in arms}
            for _ in range(args.repeats):
                t = {arm: [] for arm in arms}
                for _ in range(args.calls):
                    for arm in arms:
                        t[arm] += timed(lambda: score_arm(arm), 1)[0]
                for arm in arms:
                    meds[arm].append(statistics.median(t[arm]))
            for arm in arms:
                print('  score and fold, decoders excluded   %-5s  median %s' % (arm, spread(meds[arm])))
            m_f = statistics.median(meds['fused'])
            print('    fused: %d bytes in %.3f ms = %.2f TB/s = %.0f%% of the %.1f TB/s HBM peak (host clock around both '
                  'launches: a lower bound on the kernels\' rate)'
                  % (nbytes, m_f, nbytes / m_f / 1e9, 100 * nbytes / (m_f * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
            del segs, rows, logw, z
            if args.score_only:
                continue

            # ---- the whole chunk loop
            def loop_arm(arm, seed):
                if arm == 'torch':
                    return torch_loop(model, mu, logvar, targets, score, n_samples, Kc)
                return VL.chunk_loop(model, mu, logvar, targets, score, n_samples, Kc, seed=seed, path=arm)
            for arm in ARMS:
                timed(lambda: loop_arm(arm, 0), 3)
            meds = {arm: [] for arm in ARMS}
            for rep in range(args.repeats):
                t = {arm: [] for arm in ARMS}
                for i in range(args.calls):
                    for arm in ARMS:
                        t[arm] += timed(lambda: loop_arm(arm, rep * args.calls + i), 1)[0]
                for arm in ARMS:
                    meds[arm].append(statistics.median(t[arm]) / n_chunks)
            for arm in ARMS:
                print('  chunk loop, per chunk                %-5s  median %s' % (arm, spread(meds[arm])))
            mf, mr = statistics.median(meds['fused']), statistics.median(meds['rows'])
            noise = max(max(v) - min(v) for v in (meds['fused'], meds['rows']))
            print('    fused / rows %.3f; fused faster than rows beyond the spread (%.3f): %s'
                  % (mf / mr, noise, 'yes' if mr - mf > noise else 'no'))
            a = loop_arm('fused', 11)
            b = loop_arm('rows', 11)
            err = max(((a[j] - b[j]).abs().max() / b[j].abs().max()).item() for j in range(a.shape[0]))
            print('    parity fused vs rows, same seed, worst state: %.3e (max-normalised); joint means %.3f / %.3f'
                  % (err, a[-1].mean().item(), b[-1].mean().item()))
    return 0


if __name__ == '__main__':
    sys.exit(main())
