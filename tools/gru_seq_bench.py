#!/usr/bin/env python
"""TextDecoder forward + backward (training mode, device-drawn dropout masks, D = 64) on the per-cell launches
(``whole_sequence = False``) and on the whole-sequence kernels of csrc/gru_seq.hip (``True``): one process, one module,
alternating blocks, so both see the same box.

    python tools/gru_seq_bench.py [--steps 200] [--block 10] > profiles/multimnist_gru_seq.txt
    python tools/gru_seq_bench.py --stack encoder > profiles/multimnist_gru_enc_seq.txt

``--stack encoder`` does the same for the TextEncoder (csrc/gru_enc_seq.hip, int64 text from
``oracle.multimnist.synthetic_text``, D = 64) and ``TextEncoder.WHOLE_SEQUENCE_DEFAULT``.

A call is timed with a host clock around work that ends in a device synchronise, after a warm-up (the method of
tools/multimnist_step_bench.py: an eager decoder is launch overhead first).  Prints medians and quartiles per batch size
and the verdict that decides ``TextDecoder.WHOLE_SEQUENCE_DEFAULT``: the new path is the default only if, at B = 100,
its median is below the per-cell median by more than the per-cell interquartile range."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--batches', type=int, nargs='+', default=[100, 256])
    ap.add_argument('--stack', choices=['decoder', 'encoder'], default='decoder')
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    from mvae_amd.multimnist import model as MM
    from oracle import models as OM, multimnist as OMM
    assert torch.cuda.is_available(), 'gru_seq_bench needs the GPU'
    dev = torch.device('cuda', 0)
    D = 64
    if args.stack == 'encoder':
        return encoder(args, dev, D, MM, OM, OMM)
    dec = MM.TextDecoder(D, MM.n_characters)
    dec.load_state_dict(OM.fill_parameters(OMM.TextDecoder(D), 41).state_dict())
    dec.to(dev).train()
    print('# %s, torch %s; TextDecoder forward + backward, D = %d, training mode, %d calls per path in alternating '
          'blocks of %d, ms per call' % (torch.cuda.get_device_name(0), torch.__version__, D, args.steps, args.block))
    verdict = None
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        zs = [torch.randn(B, D, generator=g).to(dev) for _ in range(4)]
        w8 = torch.randn(B, MM.max_length, MM.n_characters, generator=g).to(dev)

        def call(i, whole):
            dec.whole_sequence = whole
            for p in dec.parameters():
                p.grad = None
            z = zs[i % 4].clone().requires_grad_()
            (dec(z) * w8).sum().backward()
            return z.grad

        def run(whole, n, i0):
            out = []
            for i in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dz = call(i0 + i, whole)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(dz).all().item()
            return out

        run(False, 15, 0); run(True, 15, 0)             # warm-up: code objects, allocator
        t_cell, t_seq = [], []
        for b in range(args.steps // args.block):
            t_cell += run(False, args.block, b * args.block)
            t_seq += run(True, args.block, b * args.block)
        mc, c1, c3 = quartiles(t_cell)
        ms, s1, s3 = quartiles(t_seq)
        faster = ms < mc - (c3 - c1)
        print('B = %d' % B)
        print('  per-cell launches      median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mc, c1, c3, c3 - c1))
        print('  whole-sequence kernels median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (ms, s1, s3, s3 - s1))
        print('  ratio whole-sequence / per-cell %.3f; below the per-cell median by more than its IQR: %s'
              % (ms / mc, 'yes' if faster else 'no'))
        if B == 100:
            verdict = faster
    if verdict is not None:
        print('verdict at B = 100: whole_sequence %s' % ('is the default' if verdict else 'stays opt-in'))
    return 0


def encoder(args, dev, D, MM, OM, OMM):
    enc = MM.TextEncoder(D, MM.n_characters)
    enc.load_state_dict(OM.fill_parameters(OMM.TextEncoder(D), 41).state_dict())
    enc.to(dev).train()
    print('# %s, torch %s; TextEncoder forward + backward, D = %d, %d calls per path in alternating blocks of %d, '
          'ms per call' % (torch.cuda.get_device_name(0), torch.__version__, D, args.steps, args.block))
    verdict = None
    for B in args.batches:
        texts = [OMM.synthetic_text(B, 4 * B + i).to(dev) for i in range(4)]
        assert texts[0].dtype == torch.int64
        w8 = torch.randn(B, 2 * D, generator=torch.Generator().manual_seed(B)).to(dev)

        def call(i, whole):
            enc.whole_sequence = whole
            for p in enc.parameters():
                p.grad = None
            (enc.heads(texts[i % 4]) * w8).sum().backward()
            return enc.embed.weight.grad

        def run(whole, n, i0):
            out = []
            for i in range(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g = call(i0 + i, whole)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(g).all().item()
            return out

        run(False, 15, 0); run(True, 15, 0)             # warm-up: code objects, allocator
        t_cell, t_seq = [], []
        for b in range(args.steps // args.block):
            t_cell += run(False, args.block, b * args.block)
            t_seq += run(True, args.block, b * args.block)
        mc, c1, c3 = quartiles(t_cell)
        ms, s1, s3 = quartiles(t_seq)
        faster = ms < mc - (c3 - c1)
        print('B = %d' % B)
        print('  per-cell launches      median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mc, c1, c3, c3 - c1))
        print('  whole-sequence kernels median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (ms, s1, s3, s3 - s1))
        print('  ratio whole-sequence / per-cell %.3f; below the per-cell median by more than its IQR: %s'
              % (ms / mc, 'yes' if faster else 'no'))
        if B == 100:
            verdict = faster
    if verdict is not None:
        print('verdict at B = 100: whole_sequence %s' % ('is the default' if verdict else 'stays opt-in'))
    return 0


if __name__ == '__main__':
    sys.exit(main())
