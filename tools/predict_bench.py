#!/usr/bin/env python
"""The fold and score launches of ``predict.py`` (K28, csrc/predict.hip) against a torch restatement on the same decoder
outputs, per chunk, and the label decoders' share of a chunk:

    hip     one ``predict_fold`` (fresh state, finish) + one ``predict_score`` with the confusion table
    torch   ``log_softmax`` (Bernoulli: ``logsigmoid`` of +-l), ``logsumexp`` over the samples, ``argmax``, a gather for
            the NLL and ``bincount`` into the table

    python tools/predict_bench.py [--repeats 3] [--calls 50] > profiles/predict.txt

Sizes: MNIST B = 64, K = 1000 (``chunk_rows`` 4096: chunks of 64 samples, [4096, 10] logits) and CelebA-19 B = 8, K = 512
(one chunk of 512 samples, the [18, 4096] logits of the grouped N = 1 Linear read through their strides; torch reads the
same block).  Synthetic data, default-size models at their random initialisation, eval mode; ``infer`` runs once outside
the timed region.  A call is timed with a host clock around work that ends in a device synchronise, after a warm-up of
every shape; the arms alternate call by call in one process; the measurement is repeated ``--repeats`` times and the
spread of the repeats' medians is reported.  "decoder" is the label decoder alone on a chunk's rows, "chunk" the draw, the
decoder and the fold of one chunk as ``predict.fold_chunks`` issues them."""
import argparse
import importlib
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (('mnist', 64, 64, 1000), ('celeba19', 100, 8, 512))      # kind, n_latents, B, K
CHUNK_ROWS = 4096


def timed(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def spread(meds):
    return 'median %.3f  (repeats %s; spread %.3f)' % (statistics.median(meds), ' '.join('%.3f' % m for m in meds),
                                                        max(meds) - min(meds))


def alternate(fns, repeats, calls, warm=5):
    """{name: the repeats' medians} of the callables, alternating call by call."""
    for fn in fns.values():
        timed(fn, warm)
    meds = {name: [] for name in fns}
    for _ in range(repeats):
        times = {name: [] for name in fns}
        for _ in range(calls):
            for name, fn in fns.items():
                times[name] += timed(fn, 1)
        for name in fns:
            meds[name].append(statistics.median(times[name]))
    return meds


def torch_fold_score(logits, B, mode, y, table):
    """The restatement on a chunk's logits [R, C] (any strides)."""
    R, C = logits.shape
    Kc = R // B
    if mode == 'categorical':
        logp = torch.logsumexp(torch.log_softmax(logits, dim=1).view(Kc, B, C), dim=0) - math.log(Kc)
        pred = torch.argmax(logp, dim=1)
        nll = -logp.gather(1, y.unsqueeze(1)).squeeze(1)
        table += torch.bincount(y * C + pred, minlength=C * C).view(C, C)
    else:
        x = logits.view(Kc, B, C) if logits.is_contiguous() else logits.t().reshape(C, Kc, B).permute(1, 2, 0)
        l1 = torch.logsumexp(torch.nn.functional.logsigmoid(x), dim=0) - math.log(Kc)
        l0 = torch.logsumexp(torch.nn.functional.logsigmoid(-x), dim=0) - math.log(Kc)
        pred = (l1 > l0).long()
        yi = y.long()
        nll = -torch.where(yi == 1, l1, l0)
        cell = torch.arange(C, device=y.device).unsqueeze(0) * 4 + yi * 2 + pred
        table += torch.bincount(cell.reshape(-1), minlength=C * 4).view(C, 2, 2)
    return pred, nll, (pred == (y if mode == 'categorical' else yi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=50)
    args = ap.parse_args()
    import mvae_amd
    from mvae_amd import kernels as K
    from mvae_amd.loglike import synthetic_data
    P = importlib.import_module('mvae_amd.predict')
    dev = torch.device('cuda')
    print('# %s, torch %s, libmvae_hip.so; fold + score of one chunk on stored label logits, chunk_rows %d; %d repeats of '
          '%d calls per arm, arms alternating call by call; ms'
          % (torch.cuda.get_device_name(0), torch.__version__, CHUNK_ROWS, args.repeats, args.calls))
    for kind, D, B, Ks in SIZES:
        torch.manual_seed(1)
        model = importlib.import_module('mvae_amd.%s.model' % kind).MVAE(D).to(dev).eval()
        image, label = synthetic_data('celeba' if kind == 'celeba19' else kind, B, seed=2)
        mode = P.MODES[kind]
        image = image.to(dev)
        y = label.to(dev).float().contiguous() if mode == 'bernoulli' else label.to(dev).long()
        Kc = min(max(1, CHUNK_ROWS // B), Ks)
        R = Kc * B
        with torch.no_grad():
            mu, logvar = P._infer(model, kind, image, y, ('image',))
            head = P.LabelHead(model, kind, R, dev)
            z = torch.empty(Kc, B, D, device=dev)
            lw = torch.empty(Kc, B, device=dev)
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
            K.iw_draw(mu, logvar, z, lw, seed=3, counter_dev=counter, counter_offset=0)
            zr = z.view(R, D)
            logits = head.logits(zr)
            C = logits.shape[1]
            out = torch.empty((B, C) if mode == 'categorical' else (B, C, 2), device=dev)
            shape = (B,) if mode == 'categorical' else (B, C)
            pred = torch.empty(shape, dtype=torch.int64, device=dev)
            nll = torch.empty(shape, device=dev)
            correct = torch.empty(shape, dtype=torch.uint8, device=dev)
            table = torch.zeros((C, C) if mode == 'categorical' else (C, 2, 2), dtype=torch.int64, device=dev)
            table_t = torch.zeros_like(table)
            state = K.fresh_predict_state(B, C, mode, dev)

            def hip():
                state[..., 0] = float('-inf'); state[..., 1] = 0.0
                K.predict_fold(logits, B, mode, state, out, finish_k=Kc)
                K.predict_score(out, mode, pred, targets=y, nll=nll, correct=correct, confusion=table)

            def fold_only():
                K.predict_fold(logits, B, mode, state, None, finish_k=0)

            def score_only():
                K.predict_score(out, mode, pred, targets=y, nll=nll, correct=correct, confusion=table)

            def restated():
                return torch_fold_score(logits, B, mode, y, table_t)

            def decoder():
                head.logits(zr)

            def chunk():
                K.iw_draw(mu, logvar, z, lw, seed=3, counter_dev=counter, counter_offset=0)
                K.predict_fold(head.logits(zr), B, mode, state, None, finish_k=0)

            hip(); table.zero_(); table_t.zero_()
            hip()
            t_pred, t_nll, _ = restated()
            same = torch.equal(pred, t_pred) and torch.equal(table, table_t)
            err = ((nll - t_nll).abs().max() / t_nll.abs().max()).item()
            meds = alternate({'hip': hip, 'torch': restated, 'fold': fold_only, 'score': score_only, 'decoder': decoder,
                              'chunk': chunk}, args.repeats, args.calls)
        print('%s: B = %d, K = %d, D = %d: %d chunk(s) of %d samples = %d rows of %d logits (%s, strides %s)'
              % (kind, B, Ks, D, -(-Ks // Kc), Kc, R, C, mode, tuple(logits.stride())))
        print('  fold + score, decoders excluded   hip    %s' % spread(meds['hip']))
        print('  fold + score, decoders excluded   torch  %s' % spread(meds['torch']))
        print('    predict_fold alone              %s' % spread(meds['fold']))
        print('    predict_score alone             %s' % spread(meds['score']))
        print('  label decoder alone               %s' % spread(meds['decoder']))
        print('  chunk (draw, decoder, fold)       %s' % spread(meds['chunk']))
        h, t = statistics.median(meds['hip']), statistics.median(meds['torch'])
        sp = max(max(m) - min(m) for m in (meds['hip'], meds['torch']))
        print('    hip / torch %.3f; hip faster than torch beyond the spread (%.3f): %s; decoder / chunk: %.0f%%'
              % (h / t, sp, 'yes' if t - h > sp else 'no',
                 100.0 * statistics.median(meds['decoder']) / statistics.median(meds['chunk'])))
        print('    parity hip vs torch: predictions and counts equal: %s; nll worst %.3e (max-normalised)' % (same, err))
    print('# not measured: whole predict() / evaluate() calls over a dataset, other chunk_rows, trained checkpoints, the '
          'kernels under a profiler (no bytes/s), MultiMNIST, FashionMNIST and CelebA, and K = 0.')
    return 0


if __name__ == '__main__':
    sys.exit(main())
