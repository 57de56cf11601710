#!/usr/bin/env python
"""The conditioning step of ``celeba19.sample.generate`` at the sizes of its sweep -- C = 37 condition rows (the prior,
then every attribute at 0 and at 1), D = 100, n = 8 and n = 64 draws per row -- in two arms that share the model:

    table   ``expert_table`` (three grouped launches for the 36 attribute heads) plus ONE ``poe_table_draw`` launch
            (K27, csrc/poe_table.hip) for all 37 posteriors and their draws: what ships
    infer   the yardstick, what the surface offered before: 37 x (``model.infer`` on a batch of 1 with that row's
            modalities, then the existing draw kernel ``iw_draw``); the prior row has no ``infer`` call (zeros)

    python tools/celeba19_sample_bench.py [--repeats 3] [--calls 20] [--out profiles/celeba19_sample.txt]

Then the decoders alone (``sample.decode``: the image decoder, the 18 attribute decoders, the sigmoids) on the n * 37 rows,
and a whole ``generate`` call, to give the decoders' share of it.  A call is timed with a host clock around work that ends
in a device synchronise, after a warm-up of every shape; the two conditioning arms alternate call by call in one process;
the whole measurement is repeated ``--repeats`` times and the median and the spread of the repeats' medians are reported.
The model is synthetic (seeded weights): the times do not depend on the values.  There is no pass mark."""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def alternate(arms, fn, repeats, calls, warm):
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
            meds[arm].append(statistics.median(t[arm]))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20, help='timed calls per arm, size and repeat')
    ap.add_argument('--n-latents', type=int, default=100)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'celeba19_sample.txt'))
    args = ap.parse_args()
    warnings.simplefilter('ignore')
    import mvae_amd  # noqa: F401
    from mvae_amd import _lib, kernels as K
    from mvae_amd.celeba19 import model as CM, sample as CS
    assert torch.cuda.is_available(), 'celeba19_sample_bench needs the GPU'
    dev = torch.device('cuda', 0)
    D = args.n_latents
    torch.manual_seed(0)
    model = CM.MVAE(D)
    model.to(dev).eval()
    model.finalize()
    state = CS.sweep_states()
    C = state.shape[0]
    rows = [[torch.tensor([float(v)], device=dev) if v >= 0 else None for v in state[c].tolist()] for c in range(C)]
    lines = []

    def say(text):
        print(text)
        lines.append(text)
    say('# %s, torch %s, %s; celeba19 sample: the sweep, C = %d condition rows, D = %d; %d repeats of %d calls per arm, '
        'the conditioning arms alternating call by call; ms per call'
        % (torch.cuda.get_device_name(0), torch.__version__, os.path.basename(_lib.lib()._name), C, D, args.repeats,
           args.calls))
    with torch.no_grad():
        for n in (8, 64):
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
            mu, logvar = torch.empty(C, D, device=dev), torch.empty(C, D, device=dev)
            z = torch.empty(n, C, D, device=dev)
            z_y = torch.empty(n, C, D, device=dev)
            zero = torch.zeros(1, D, device=dev)
            z1, lw1 = torch.empty(n, 1, D, device=dev), torch.empty(n, 1, device=dev)

            def condition(arm, eps=None):
                if arm == 'table':
                    table = CS.expert_table(model)
                    if eps is not None:
                        K.poe_table_draw(table, state, mu, logvar, z, eps=eps)
                    else:
                        K.poe_table_draw(table, state, mu, logvar, z, seed=3, counter_dev=counter)
                    return mu, logvar, z
                mus, lvs = [], []
                for c in range(C):
                    m, lv = (zero, zero) if c == 0 else model.infer(attrs=rows[c])
                    m, lv = m.contiguous(), lv.contiguous()
                    if eps is not None:
                        K.iw_draw(m, lv, z1, lw1, eps=eps[:, c:c + 1].contiguous())
                    else:
                        K.iw_draw(m, lv, z1, lw1, seed=3, counter_dev=counter, counter_offset=c)
                    z_y[:, c:c + 1] = z1
                    mus.append(m); lvs.append(lv)
                return torch.cat(mus), torch.cat(lvs), z_y
            say('n = %d draws per row (%d decoder rows)' % (n, n * C))
            meds = alternate(('table', 'infer'), condition, args.repeats, args.calls, 3)
            say('  conditioning: table build + one poe_table_draw launch          median %s' % spread(meds['table']))
            say('  conditioning: yardstick, 37 x (model.infer on 1 row + iw_draw)  median %s' % spread(meds['infer']))
            mt, my = statistics.median(meds['table']), statistics.median(meds['infer'])
            say('    yardstick / table %.1fx' % (my / mt))
            tb = [statistics.median(timed(lambda: CS.expert_table(model), args.calls)[0]) for _ in range(args.repeats)]
            table = CS.expert_table(model)
            ln = [statistics.median(timed(lambda: K.poe_table_draw(table, state, mu, logvar, z, seed=3, counter_dev=counter),
                                          args.calls)[0]) for _ in range(args.repeats)]
            say('    of the table arm: expert_table alone %s' % spread(tb))
            say('    of the table arm: poe_table_draw alone (state upload + launch) %s' % spread(ln))
            eps = torch.randn(n, C, D, generator=torch.Generator().manual_seed(n)).to(dev)
            a = [t.clone() for t in condition('table', eps)]
            b = condition('infer', eps)
            say('    parity table vs yardstick, same eps (max-normalised): mu %.2e  logvar %.2e  z %.2e'
                % tuple(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(a, b)))

            zr = a[2].reshape(n * C, D)
            timed(lambda: CS.decode(model, zr), 3)
            dm = [statistics.median(timed(lambda: CS.decode(model, zr), args.calls)[0]) for _ in range(args.repeats)]
            say('  decoders alone (image decoder, 18 attribute decoders, sigmoids)    median %s' % spread(dm))
            timed(lambda: CS.generate(model, state=state, n_samples=n, seed=3), 3)
            gm = [statistics.median(timed(lambda: CS.generate(model, state=state, n_samples=n, seed=3), args.calls)[0])
                  for _ in range(args.repeats)]
            say('  a whole generate call                                               median %s' % spread(gm))
            say('    decoders / generate: %.0f%%; conditioning (table arm) / generate: %.0f%%'
                % (100 * statistics.median(dm) / statistics.median(gm), 100 * mt / statistics.median(gm)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
