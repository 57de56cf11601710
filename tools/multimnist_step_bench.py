#!/usr/bin/env python
"""The eager MultiMNIST train step (three model() calls, three elbo_loss, backward, Adam) on the HIP modules, beside
the plain-torch restatement of the same model (tests/multimnist_ref.py) moved to the same GPU and stepped with
torch.optim.Adam -- same process, alternating blocks, so both see the same box.

    python tools/multimnist_step_bench.py [--batch 100] [--steps 120] > profiles/multimnist_step.txt

A step is timed with a host clock around work that ends in a device synchronise (an eager step is as much launch
overhead as kernel time: that is what its user waits for).  Prints both medians and interquartile ranges and the verdict
of the gate: the HIP median is not above the baseline's median by more than the baseline's own interquartile range."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--block', type=int, default=10)
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    from mvae_amd.multimnist import model as MM, train as MT
    from mvae_amd.optim import FusedAdam
    from oracle import models as OM
    import multimnist_ref as R
    assert torch.cuda.is_available(), 'multimnist_step_bench needs the GPU'
    dev = torch.device('cuda', 0)
    ref = OM.fill_parameters(R.MVAE(64), 1)
    hip = MM.MVAE(64)
    hip.load_state_dict(ref.state_dict())
    ref.to(dev).train(); hip.to(dev).train()
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-3)
    opt_hip = FusedAdam(hip.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    batches = [(torch.rand(args.batch, 1, 50, 50, generator=g).to(dev), MT.synthetic_text(args.batch, g).to(dev)) for _ in range(4)]

    def step_hip(i):
        return MT.train_step(hip, opt_hip, batches[i % 4][0], batches[i % 4][1], 1.0, 10.0, 0.5)

    def step_ref(i):
        opt_ref.zero_grad()
        total = R.three_call_step(ref, batches[i % 4][0], batches[i % 4][1], None, 1.0, 10.0, 0.5)[0]
        total.backward()
        opt_ref.step()
        return total.detach()

    def run(fn, n, i0):
        out = []
        for i in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = fn(i0 + i)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        assert torch.isfinite(loss).item()
        return out

    run(step_hip, 15, 0); run(step_ref, 15, 0)          # warm-up: code objects, MIOpen's algorithm search, allocator
    t_hip, t_ref = [], []
    for b in range(args.steps // args.block):
        t_hip += run(step_hip, args.block, b * args.block)
        t_ref += run(step_ref, args.block, b * args.block)
    mh, h1, h3 = quartiles(t_hip)
    mr, r1, r3 = quartiles(t_ref)
    print('# %s, torch %s; eager MultiMNIST step, B = %d, %d steps each in alternating blocks of %d, ms per step'
          % (torch.cuda.get_device_name(0), torch.__version__, args.batch, len(t_hip), args.block))
    print('hip modules + FusedAdam        median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mh, h1, h3, h3 - h1))
    print('restatement + torch.optim.Adam median %.3f  quartiles %.3f .. %.3f  (IQR %.3f)' % (mr, r1, r3, r3 - r1))
    ok = mh <= mr + (r3 - r1)
    print('ratio hip / baseline %.3f; gate (hip median <= baseline median + baseline IQR): %s' % (mh / mr, 'PASS' if ok else 'FAIL'))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
