#!/usr/bin/env python
"""Hot timings of the general stride-2 conv launches (csrc/conv_gen.hip) on MultiMNIST's four geometries, beside ATen's
own launch of the same operation in the same process on the same card.

    python tools/conv_gen_bench.py [--batches 100 512] [--reps 60] > profiles/multimnist_conv_gen.txt

Per (geometry, launch, batch): median of ``--reps`` launches after warm-up, each timed with a pair of device events on
an otherwise idle stream (the launch is a few to a few hundred microseconds: event resolution ~1 us; the figures are
launch-to-completion times of hot code, weights and inputs in the caches where they fit).  TFLOP/s counts the
algorithm's 2 * MACs (no padded taps); the share is of the 157.3 TFLOP/s fp32 matrix peak.  ATen: F.conv2d /
F.conv_transpose2d for the forward, aten.convolution_backward with an output mask for ONE gradient at a time."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TFLOPS = 157.3

# (name, transposed, Cin, Cout, ks, pad, H)
GEOMETRIES = [('Conv2d(32,64,4,2,1) 25->12', False, 32, 64, 4, 1, 25), ('Conv2d(128,256,4,2,0) 6->2', False, 128, 256, 4, 0, 6),
              ('ConvT2d(256,128,4,2,0) 2->6', True, 256, 128, 4, 0, 2), ('ConvT2d(64,32,5,2,1) 12->25', True, 64, 32, 5, 1, 12)]


def timed(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[100, 512])
    ap.add_argument('--reps', type=int, default=60)
    args = ap.parse_args()
    import mvae_amd  # noqa: F401
    from mvae_amd import kernels as K
    assert torch.cuda.is_available(), 'conv_gen_bench needs the GPU'
    dev = torch.device('cuda', 0)
    print('# %s, torch %s; median of %d hot launches (device events), us' % (torch.cuda.get_device_name(0), torch.__version__, args.reps))
    print('%-30s %-6s %5s %10s %9s %7s %10s %7s' % ('geometry', 'launch', 'B', 'hip us', 'TFLOP/s', 'of peak', 'ATen us', 'hip/ATen'))
    g = torch.Generator().manual_seed(0)
    for name, tr, Cin, Cout, ks, p, H in GEOMETRIES:
        for B in args.batches:
            OH = (H - 1) * 2 - 2 * p + ks if tr else (H + 2 * p - ks) // 2 + 1
            x = torch.randn(B, Cin, H, H, generator=g).to(dev)
            w = torch.randn((Cin, Cout, ks, ks) if tr else (Cout, Cin, ks, ks), generator=g).to(dev) * 0.05
            dy = torch.randn(B, Cout, OH, OH, generator=g).to(dev)
            y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
            macs = B * (Cin * H * H * Cout if tr else Cout * OH * OH * Cin) * ks * ks
            fwd, dgrad, wgrad = ((K.convT2d_gen_fwd, K.convT2d_gen_dgrad, K.convT2d_gen_wgrad) if tr else
                                 (K.conv2d_gen_fwd, K.conv2d_gen_dgrad, K.conv2d_gen_wgrad))
            conv = F.conv_transpose2d if tr else F.conv2d

            def aten_bwd(mask):
                return torch.ops.aten.convolution_backward(dy, x, w, None, [2, 2], [p, p], [1, 1], tr, [0, 0], 1, mask)
            runs = [('fwd', lambda: fwd(x, w, y, None, 2, p), lambda: conv(x, w, None, 2, p)),
                    ('dgrad', lambda: dgrad(dy, w, dx, None, 2, p), lambda: aten_bwd([True, False, False])),
                    ('wgrad', lambda: wgrad(dy, x, dw, 2, p), lambda: aten_bwd([False, True, False]))]
            for launch, hip, aten in runs:
                with torch.no_grad():
                    t_hip, t_aten = timed(hip, args.reps), timed(aten, args.reps)
                tf = 2.0 * macs / t_hip * 1e-6
                print('%-30s %-6s %5d %10.1f %9.2f %6.1f%% %10.1f %7.2f' % (name, launch, B, t_hip, tf, 100 * tf / PEAK_TFLOPS, t_aten, t_hip / t_aten))


if __name__ == '__main__':
    main()
