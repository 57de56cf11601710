#!/usr/bin/env python
"""Time of the MultiMNIST dataset builder at the command line's defaults (0-4 digits, resize, translate, seed 681307):
60000 + 10000 canvases through the round driver of ``multimnist/datasets.py`` with the HIP compose kernel
(csrc/multimnist_data.hip), beside the same driver over the numpy restatement of the compose step
(tests/multimnist_data_ref.py) on the same box.

    python tools/multimnist_data_bench.py [--data-dir ./data] [--host-canvases 7000] > profiles/multimnist_datasets.txt

Without MNIST IDX files under ``--data-dir`` the digit bank is synthetic: 2000 + 500 "digits" of three random strokes
(value 255, a 128 fringe) inside the central 20 x 20 pixels -- stroke-like, so the share of rejected canvases is of
MNIST's order, unlike the solid blocks of the tests' bank.  The host restatement runs on ``--host-canvases`` canvases
(it resamples in Python loops); the rates are canvases per second of wall time, plan drawing included.  A record, not
a gate.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def stroke_bank(n, rng):
    bank = np.zeros((n, 28, 28), dtype=np.uint8)
    for i in range(n):
        pts = rng.randint(4, 24, (4, 2))
        for a, b in zip(pts[:-1], pts[1:]):
            for t in np.linspace(0.0, 1.0, 40):
                y, x = np.round(a + t * (b - a)).astype(int)
                patch = bank[i, y - 1:y + 2, x - 1:x + 2]
                patch[patch < 128] = 128
                bank[i, y, x] = 255
    return bank


def timed(composer, clock):
    def run(plan):
        t0 = time.perf_counter()
        out = composer(plan)
        clock[0] += time.perf_counter() - t0
        clock[1] += 1
        return out
    return run


def build(MD, mnist, n, composer, seed):
    clock = [0.0, 0]
    t0 = time.perf_counter()
    x, y, plans, stats = MD.mk_dataset(n, mnist, 0, 4, 50, composer=timed(composer, clock), rng=np.random.RandomState(seed),
                                       return_plans=True)
    return time.perf_counter() - t0, clock, x, plans, stats


def report(name, n, wall, clock, stats):
    composed = n + sum(stats['redrawn'])
    print('  %s: %d canvases in %.3f s = %.0f canvases/s; compose calls %d, %.3f s inside them (%d canvases composed, '
          '%.0f per second of compose time)' % (name, n, wall, n / wall, clock[1], clock[0], composed, composed / clock[0]))
    print('    rounds per chunk of at most 8192: %s' % stats['rounds'])
    shares = ['%.1f%%' % (100.0 * r / n) for r in stats['redrawn'][:12]]
    print('    share of the canvases redrawn in rounds 2.. : %s%s' % (' '.join(shares), ' ...' if len(stats['redrawn']) > 12 else ''))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--data-dir', default='./data')
    ap.add_argument('--host-canvases', type=int, default=7000)
    ap.add_argument('--seed', type=int, default=681307)
    args = ap.parse_args()
    import mvae_amd  # noqa: F401
    from mvae_amd.multimnist import datasets as MD
    from mvae_amd.train_common import _find_idx
    import multimnist_data_ref as R

    if _find_idx(args.data_dir, 'train-images-idx3-ubyte'):
        train, test = MD.load_mnist(args.data_dir)
        bank_name = 'MNIST (%d + %d digits)' % (len(train['digits']), len(test['digits']))
    else:
        rng = np.random.RandomState(1)
        train = {'digits': stroke_bank(2000, rng), 'labels': rng.randint(0, 10, 2000)}
        test = {'digits': stroke_bank(500, rng), 'labels': rng.randint(0, 10, 500)}
        bank_name = 'synthetic strokes (2000 + 500 digits; no MNIST files under %s)' % args.data_dir
    print('# %s, torch %s; MultiMNIST builder at the command-line defaults (0-4 digits, resize, translate, seed %d); bank: %s'
          % (torch.cuda.get_device_name(0), torch.__version__, args.seed, bank_name))
    MD.mk_dataset(64, train, 0, 4, 50, rng=np.random.RandomState(0))            # warm-up: tables, first launch
    torch.cuda.synchronize()
    print('device (mvae_multimnist_compose, one launch per round and chunk; canvases and flags copied to the host)')
    results = {}
    for name, mnist, n in (('train', train, 60000), ('test', test, 10000)):
        wall, clock, x, plans, stats = build(MD, mnist, n, MD.device_composer(mnist['digits']), args.seed)
        report(name, n, wall, clock, stats)
        results[name] = (wall, x, plans)
    total = results['train'][0] + results['test'][0]
    print('  both splits: 70000 canvases in %.3f s = %.0f canvases/s' % (total, 70000 / total))
    n = args.host_canvases
    print('host (numpy restatement of the compose step, same driver, same seed, first %d canvases of the train split)' % n)
    wall, clock, x, plans, stats = build(MD, train, n, R.composer(train['digits']), args.seed)
    report('train', n, wall, clock, stats)
    # the same seed draws the same counts but not the same plans once a redraw differs in order; compare through the plans
    want = R.compose(train['digits'], results['train'][2][:256])
    same = np.array_equal(want[0], results['train'][1][:256]) and not want[1].any()
    print('check: the first 256 device canvases equal the restatement applied to their plans: %s' % ('yes' if same else 'NO'))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
