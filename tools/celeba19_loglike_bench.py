#!/usr/bin/env python
"""The chunk loop of ``celeba19.loglike.log_likelihood`` -- the image marginal, the 18 attribute marginals and the joint from
one pass of the 19 decoders -- in three arms that share the model, the data and (fused, rows) the decoders:

    fused   ``heads_bce_rows`` + one ``iw_fold_rows`` per chunk (K25, csrc/loglike_heads.hip)
    rows    the kernels that were there before: the grouped N = 1 Linear, ``bce_elem_fwd``, 20 ``iw_accumulate`` and a
            [19, R] -> [R, 19] copy
    torch   plain torch: a torch draw and density ratio, the image decoder, 18 attribute-decoder module calls,
            ``binary_cross_entropy_with_logits``, the [20, K, B] log-weights stored and reduced by ``torch.logsumexp``

    python tools/celeba19_loglike_bench.py [--repeats 3] [--calls 20] > profiles/celeba19_loglike.txt
    python tools/celeba19_loglike_bench.py --score-only       # head, score and fold of the fused arm alone
    rocprofv3 --kernel-trace --stats ... -- python tools/celeba19_loglike_bench.py --score-only --calls 20

Default size: ``n_latents`` 100, synthetic data, B = 8, K = 512, all 19 modalities scored and given.  ``infer`` runs once,
outside the timed region (the same in every arm).  A call is timed with a host clock around work that ends in a device
synchronise, after a warm-up of every shape; the arms alternate call by call; the whole measurement is repeated
``--repeats`` times and the spread of the repeats' medians is reported.  "head, score and fold" times the arms on the
stored third-layer activations of one chunk (and a stored image row), the decoders excluded; "decoders" times the image
decoder, its row sums and layers 1 - 3 of the 18 experts alone.  The bytes of ``heads_bce_rows`` are the activations, the
weight rows and biases, the targets and the rows it writes, from the shapes; its rate comes from ``--calls`` launches back
to back between two synchronises."""
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
HBM_PEAK = 8.0e12           # bytes/s, MI355X: 8.0 TB/s spec


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


def alternate(arms, fn, repeats, calls, warm, scale=1.0):
    """{arm: the repeats' medians} of ``fn(arm)``, the arms alternating call by call."""
    for arm in arms:
        timed(lambda: fn(arm), warm)
    meds = {arm: [] for arm in arms}
    for _ in range(repeats):
        t = {arm: [] for arm in arms}
        for _ in range(calls):
            for arm in arms:
                t[arm] += timed(lambda: fn(arm), 1)[0]
        for arm in arms:
            meds[arm].append(statistics.median(t[arm]) * scale)
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per arm, shape and repeat')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--n-samples', type=int, default=512)
    ap.add_argument('--n-latents', type=int, default=100)
    ap.add_argument('--score-only', action='store_true',
                    help='only the fused arm on stored activations (for a kernel trace)')
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    from mvae_amd import _lib, kernels as K
    from mvae_amd.celeba19 import loglike as CL, model as CM
    from mvae_amd.vision.loglike import fresh_state
    assert torch.cuda.is_available(), 'celeba19_loglike_bench needs the GPU'
    dev = torch.device('cuda', 0)
    B, n_samples, D = args.batch, args.n_samples, args.n_latents
    G, S = CM.N_ATTRS, CL.N_ROWS
    torch.manual_seed(0)
    model = CM.MVAE(D)
    model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    image = torch.rand(B, 3, 64, 64, generator=g).to(dev)
    attrs = torch.randint(0, 2, (B, G), generator=g).float().to(dev)
    pixels = image.reshape(B, -1)
    score = CL.MODALITIES
    sel = list(range(S))
    sel_dev = torch.arange(S, device=dev)
    F = torch.nn.functional
    print('# %s, torch %s, %s; celeba19 log_likelihood, B = %d, K = %d, D = %d, score and given: all 19, per_modality; '
          '%d repeats of %d calls per arm, arms alternating call by call; ms'
          % (torch.cuda.get_device_name(0), torch.__version__, os.path.basename(_lib.lib()._name), B, n_samples, D,
             args.repeats, args.calls))
    with torch.no_grad():
        mu, logvar = CL.infer(model, image, attrs, score)
        std = torch.exp(0.5 * logvar)
        for chunk_rows in CHUNK_ROWS:
            Kc = min(max(1, chunk_rows // B), n_samples)
            n_chunks = -(-n_samples // Kc)
            R = Kc * B
            experts = CL.AttrExperts(model, 0, G - 1, R, dev)
            H = experts.width
            nbytes = 4 * (G * R * H + G * H + G + B * G + G * R)
            print('chunk_rows %d: %d chunk(s) of %d samples = %d rows; heads_bce_rows moves %d bytes per chunk '
                  '(activations, weights, targets, rows out)' % (chunk_rows, n_chunks, Kc, R, nbytes))

            # ---- head, score and fold alone, on the stored third-layer activations of one chunk
            z = torch.empty(Kc, B, D, device=dev)
            lw = torch.empty(Kc, B, device=dev)
            K.iw_draw(mu, logvar, z, lw, seed=3, counter_dev=torch.zeros(1, dtype=torch.int64, device=dev))
            zr = z.view(R, D)
            rec = torch.empty(S, R, device=dev)
            K.bce_rowsum_fwd(model.image_decoder(zr).reshape(R, -1).contiguous(), pixels, rec[0], target_rows=B)
            h = experts.hidden(zr)
            logits = torch.empty(G, R, 1, device=dev)
            targets = attrs.t().unsqueeze(1).expand(G, Kc, B).reshape(G, R).contiguous()
            out = torch.empty(S + 1, B, device=dev)
            logw = torch.empty(S + 1, Kc, B, device=dev)
            state = fresh_state(S + 1, B, dev)                  # folded into again and again: no reset in the timed call
            heads = [(d.net[6].weight.detach(), d.net[6].bias.detach()) for d in model.attr_decoders]

            def torch_score(h, rec0, lw, logw, k0, n):
                """The torch arm's share of a chunk: 18 head products, BCE, the 20 log-weight rows into logw[:, k0:]."""
                x = torch.cat([F.linear(h[i], w, b) for i, (w, b) in enumerate(heads)], dim=1)        # [R, 18]
                t = attrs.unsqueeze(0).expand(n, B, G).reshape(n * B, G)
                bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').view(n, B, G)
                img = rec0.view(n, B)
                logw[0, k0:k0 + n] = lw - img
                logw[1:S, k0:k0 + n] = lw.unsqueeze(0) - bce.permute(2, 0, 1)
                logw[S, k0:k0 + n] = lw - img - bce.sum(dim=2)

            def score_arm(arm):
                if arm == 'torch':
                    torch_score(h, rec[0], lw, logw, 0, Kc)
                    return torch.logsumexp(logw, dim=1) - math.log(Kc)
                if arm == 'fused':
                    experts.rec_fused(h, attrs, rec[1:])
                else:
                    experts.rec_rows(h, targets, rec[1:], logits)
                CL.FOLDS[arm](lw, rec, sel, sel_dev, state, out, Kc)
                return out
            arms = ('fused',) if args.score_only else ARMS
            meds = alternate(arms, score_arm, args.repeats, args.calls, 5)
            for arm in arms:
                print('  head, score and fold, decoders excluded  %-5s  median %s' % (arm, spread(meds[arm])))

            def heads_alone():
                for _ in range(args.calls):
                    experts.rec_fused(h, attrs, rec[1:])
            timed(heads_alone, 2)
            hm = [statistics.median(timed(heads_alone, 5)[0]) / args.calls for _ in range(args.repeats)]
            m_h = statistics.median(hm)
            print('    heads_bce_rows alone, %d launches back to back: %s per launch; %d bytes = %.0f GB/s = %.0f%% of the '
                  '%.1f TB/s HBM peak' % (args.calls, spread(hm), nbytes, nbytes / m_h / 1e6,
                                          100 * nbytes / (m_h * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
            if args.score_only:
                del h, rec, logits, targets, logw, z, experts
                continue

            # ---- the decoders alone: the image decoder and its row sums, layers 1 - 3 of the 18 experts
            def decoders():
                K.bce_rowsum_fwd(model.image_decoder(zr).reshape(R, -1).contiguous(), pixels, rec[0], target_rows=B)
                return experts.hidden(zr)
            timed(decoders, 3)
            dm = [statistics.median(timed(decoders, args.calls)[0]) for _ in range(args.repeats)]
            print('  decoders alone (image decoder + row sums, experts\' layers 1 - 3)    median %s' % spread(dm))
            del h, logits, targets, experts

            # ---- the whole chunk loop
            def torch_loop():
                logw_all = torch.empty(S + 1, n_samples, B, device=dev)
                for k0 in range(0, n_samples, Kc):
                    n = min(Kc, n_samples - k0)
                    eps = torch.randn(n, B, D, device=dev)
                    zz = mu + std * eps
                    lwc = (0.5 * eps * eps - 0.5 * zz * zz + 0.5 * logvar).sum(dim=2)
                    zzr = zz.view(n * B, D)
                    img = F.binary_cross_entropy_with_logits(
                        model.image_decoder(zzr).reshape(n * B, -1),
                        pixels.unsqueeze(0).expand(n, B, -1).reshape(n * B, -1), reduction='none').sum(dim=1)
                    x = torch.cat([model.attr_decoders[i](zzr) for i in range(G)], dim=1)
                    t = attrs.unsqueeze(0).expand(n, B, G).reshape(n * B, G)
                    bce = F.binary_cross_entropy_with_logits(x, t, reduction='none').view(n, B, G)
                    img = img.view(n, B)
                    logw_all[0, k0:k0 + n] = lwc - img
                    logw_all[1:S, k0:k0 + n] = lwc.unsqueeze(0) - bce.permute(2, 0, 1)
                    logw_all[S, k0:k0 + n] = lwc - img - bce.sum(dim=2)
                return torch.logsumexp(logw_all, dim=1) - math.log(n_samples)

            seeds = iter(range(1 << 30))

            def loop_arm(arm, seed=None):
                if arm == 'torch':
                    return torch_loop()
                return CL.chunk_loop(model, mu, logvar, pixels, attrs, score, n_samples, Kc,
                                     seed=next(seeds) if seed is None else seed, path=arm)
            meds = alternate(ARMS, loop_arm, args.repeats, args.calls, 3, scale=1.0 / n_chunks)
            for arm in ARMS:
                print('  chunk loop, per chunk                    %-5s  median %s' % (arm, spread(meds[arm])))
            mf, mr = statistics.median(meds['fused']), statistics.median(meds['rows'])
            noise = max(max(v) - min(v) for v in (meds['fused'], meds['rows']))
            print('    decoders / chunk: %.0f%% (fused), %.0f%% (rows); fused / rows %.3f; fused faster than rows beyond the '
                  'spread (%.3f): %s' % (100 * statistics.median(dm) / mf, 100 * statistics.median(dm) / mr, mf / mr, noise,
                                         'yes' if mr - mf > noise else 'no'))
            a = loop_arm('fused', 11)
            b = loop_arm('rows', 11)
            err = max(((a[j] - b[j]).abs().max() / b[j].abs().max()).item() for j in range(a.shape[0]))
            print('    parity fused vs rows, same seed, worst state: %.3e (max-normalised); joint means %.3f / %.3f'
                  % (err, a[-1].mean().item(), b[-1].mean().item()))
            del rec, logw, z
    return 0


if __name__ == '__main__':
    sys.exit(main())
