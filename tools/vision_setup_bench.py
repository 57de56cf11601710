#!/usr/bin/env python
"""Rate of the Canny edge step of ``vision/setup.py`` (csrc/vision_setup.hip) on aligned-CelebA images, 218 x 178, sigma 2:

  1. ``mvae_canny`` on device-resident gray batches -- the whole call (float stage + hysteresis), the hysteresis launch
     alone on the class planes the float stage wrote, and their difference as the float stage's share -- on two kinds of
     content: the test scenes (flat shapes + noise) and smooth photograph-like images;
  2. the numpy / scipy.ndimage restatement of the same algorithm (tests/vision_setup_ref.py, fp32) on the same box, one
     image per task on a pool of 16 worker processes;
  3. ``setup.py edge`` end to end on a folder of synthetic JPEGs (decode threads, uploads, launches, downloads, JPEG
     encode), beside the decode + encode alone on the same threads;
  4. one ``CelebVisionLoader`` epoch with ``edge='folder'`` against ``edge='canny'`` on a synthetic tree of JPEGs.

    python tools/vision_setup_bench.py > profiles/vision_setup.txt

Device times are host-clock windows around a run of calls that ends in a synchronise, ``--repeats`` windows per figure,
median and min .. max; variants alternate window by window.  The edge maps of 1 are compared with the restatement's.
A record, not a gate; no number is expected in advance.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

H, W = 218, 178


def _restated(img):
    import vision_setup_ref as R
    return R.canny(img, dtype=np.float32)


def scipy_rate(images, workers, rounds):
    """images / s of the restatement over a pool of worker processes; run before this process touches the GPU."""
    import multiprocessing as mp
    with mp.get_context('fork').Pool(workers) as pool:
        pool.map(_restated, images[:workers])                          # start the workers, import scipy
        ts = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            pool.map(_restated, images, chunksize=1)
            ts.append(time.perf_counter() - t0)
    return sorted(ts)


def show(name, ts, n_images, unit=1e3, label='ms'):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    print('  %-64s median %9.3f %s   min %9.3f   max %9.3f   %10.0f images/s   (%d windows)'
          % (name, med * unit, label, ts[0] * unit, ts[-1] * unit, n_images / med, len(ts)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=str, default='64,512', help='batch sizes of the device-only figures')
    ap.add_argument('--cli-batch', type=int, default=64, help='--batch-size of the setup.py edge run')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50, help='calls per window of the device-only figures')
    ap.add_argument('--files', type=int, default=2000, help='JPEG files of the setup.py edge run')
    ap.add_argument('--tree-files', type=int, default=400, help='items of the loader tree (one epoch)')
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args()
    if not os.path.exists('/dev/kfd'):
        raise SystemExit('this tool times GPU work: no GPU here, nothing measured')
    import vision_setup_ref as R
    from vision_data_bench import smooth, write_tree
    batches = [int(b) for b in args.batches.split(',')]
    B = max(batches)
    HOST = min(batches)              # images per round of the scipy figure
    rng = np.random.RandomState(11)
    contents = {'test scenes (shapes + noise 0.02)': np.stack([R.scene(H, W, 100 + b) for b in range(B)]),
                'smooth photograph-like images': np.stack([smooth(rng, (H, W)) for _ in range(B)])}
    host = {name: scipy_rate(list(x[:HOST]), args.workers, 3) for name, x in contents.items()}

    import torch
    if not torch.cuda.is_available():
        raise SystemExit('this tool times GPU work: no GPU here, nothing measured')
    from PIL import Image
    import mvae_amd  # noqa: F401
    from mvae_amd import preprocess as PP
    from mvae_amd.vision import datasets as VD, setup as VS
    dev = torch.device('cuda', 0)
    print('# %s, torch %s, Pillow %s, scipy %s; %d x %d gray uint8 images, sigma 2, thresholds 0.1 / 0.2'
          % (torch.cuda.get_device_name(0), torch.__version__, Image.__version__, __import__('scipy').__version__, H, W))
    op = PP.Canny()
    ok = True
    print('1. device-resident batches (windows of %d calls, the two alternating):' % args.inner)
    for name, x, B in [(name, x[:b], b) for name, x in contents.items() for b in batches]:
        d = torch.from_numpy(x).to(dev)
        edges, cls, _ = op.stages(d)
        want = np.stack([R.hysteresis(c) for c in cls.cpu().numpy()])
        same = np.array_equal(edges.cpu().numpy(), want)
        ref = np.stack([R.canny(im) for im in x[:4]])
        differ = int((edges[:4].cpu().numpy() != ref).sum())
        ok = ok and same
        fns = [lambda: op(d), lambda: PP.canny_hysteresis(cls)]
        for fn in fns:
            for _ in range(10):
                fn()
        times = [[] for _ in fns]
        for _ in range(args.repeats):
            for k, fn in enumerate(fns):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.inner)
        print(' B = %d, %s: %.2f %% edge pixels, %.2f %% non-zero classes'
              % (B, name, 100.0 * (edges > 0).float().mean().item(), 100.0 * (cls > 0).float().mean().item()))
        a = show('mvae_canny, both launches (per batch)', times[0], B)
        b = show('mvae_canny_hysteresis alone (per batch)', times[1], B)
        print('  float stage by difference of the medians: %.3f ms per batch, %.0f images/s' % ((a - b) * 1e3, B / (a - b)))
        print('  edges equal the restated hysteresis of the kernel\'s classes: %s; pixels that differ from the fp64 '
              'restatement in the first 4 images: %d' % ('yes' if same else 'NO', differ))
    print('2. the scipy restatement (fp32), %d worker processes, %d images per round:' % (args.workers, HOST))
    for name, ts in host.items():
        show(name, ts, HOST)

    root = tempfile.mkdtemp(prefix='vision_setup_')
    try:
        in_dir, out_dir = os.path.join(root, 'in'), os.path.join(root, 'out')
        os.makedirs(in_dir)
        rng = np.random.RandomState(12)
        for i in range(args.files):
            Image.fromarray(smooth(rng, (H, W, 3)), 'RGB').save(os.path.join(in_dir, '%06d.jpg' % (i + 1)), quality=90)
        names = sorted(os.listdir(in_dir))
        print('3. setup.py edge on %d JPEG files (quality 90, smooth synthetic content), batches of %d, %d host threads:'
              % (args.files, args.cli_batch, args.workers))

        def cli():
            stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
            try:
                VS.build_edge_dataset(in_dir, out_dir, sigma=2.0, batch_size=args.cli_batch, decode_threads=args.workers)
            finally:
                sys.stdout.close()
                sys.stdout = stdout

        def host_only():
            from concurrent.futures import ThreadPoolExecutor
            blank = np.zeros((H, W), np.uint8)

            def one(name):
                np.asarray(Image.open(os.path.join(in_dir, name)).convert('L'))
                Image.fromarray(blank).save(os.path.join(out_dir, name))
            with ThreadPoolExecutor(args.workers) as pool:
                list(pool.map(one, names))
        cli()
        tc, th = [], []
        for _ in range(3):
            t0 = time.perf_counter(); cli(); tc.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); host_only(); th.append(time.perf_counter() - t0)
        show('the whole run', tc, args.files)
        show('decode + encode of a blank map alone, same threads', th, args.files)
    finally:
        shutil.rmtree(root, ignore_errors=True)

    root = tempfile.mkdtemp(prefix='vision_tree_')
    try:
        mark_path = write_tree(root, args.tree_files, (H, W), np.random.RandomState(8))
        loaders = [VD.CelebVisionLoader('train', root, 50, True, dev, seed=1, watermark_path=mark_path, edge=e)
                   for e in ('folder', 'canny')]
        print('4. CelebVisionLoader, one epoch of %d items (batches of 50, JPEG files, %d decode threads):'
              % (args.tree_files, loaders[0]._threads))

        def epoch(loader):
            n = sum(batch6[0].shape[0] for batch6 in loader)
            torch.cuda.synchronize()
            assert n == args.tree_files
        te = [[], []]
        for loader in loaders:
            epoch(loader)
        for _ in range(5):
            for k, loader in enumerate(loaders):
                t0 = time.perf_counter(); epoch(loader); te[k].append(time.perf_counter() - t0)
        show("edge='folder' (four files per item)", te[0], args.tree_files)
        show("edge='canny' (three files per item, Canny per batch)", te[1], args.tree_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
