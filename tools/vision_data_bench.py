#!/usr/bin/env python
"""Time of the vision experiment's input pipeline at the training batch (B = 50 aligned-CelebA images, 218 x 178 -> 64):

  1. the ``preprocess.VisionCompose`` launch (csrc/vision_data.hip) on device-resident uint8 sources, with a gray source
     and without (luma in the kernel);
  2. the path that existed before it, what ``vision/sample.py:condition_image`` does for one image, applied to the batch:
     the six modalities derived on the host (numpy, Pillow's paste per image, gray planes repeated to three channels), six
     uploads, six ``ResizeCenterCropToTensor`` launches, the channel slices and ``1 - mask`` -- whole, and its six launches
     alone on device-resident inputs;
  3. one ``CelebVisionLoader`` epoch over a synthetic tree of JPEG files, beside the file decode alone on the same threads.

    python tools/vision_data_bench.py > profiles/vision_datasets.txt

Device times are host-clock windows around a run of launches that ends in a synchronise, ``--repeats`` windows per
figure, reported as median and min .. max; the two paths alternate window by window.  The outputs of 1 and 2 are compared
(2 pastes with Pillow itself).  A record, not a gate; no ratio is expected in advance.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def smooth(rng, shape, grid=12):
    """Low-frequency random uint8 image(s): photographs compress and decode unlike white noise."""
    from PIL import Image
    h, w = shape[:2]
    c = shape[2] if len(shape) == 3 else 1
    small = rng.randint(0, 256, (grid, grid, c)).astype(np.uint8)
    planes = [np.asarray(Image.fromarray(small[:, :, k]).resize((w, h), Image.BICUBIC)) for k in range(c)]
    out = np.stack(planes, axis=2)
    return out if len(shape) == 3 else out[:, :, 0]


def host_derive(rgb, edge, mask, gray, mark_image):
    """The six uint8 [B, H, W, 3] batches the pre-existing resize kernel takes, derived on the host."""
    from PIL import Image
    obscured = np.array(rgb, copy=True)
    obscured[:, :, rgb.shape[2] // 2 + 1:, :] = 0
    marked = np.empty_like(rgb)
    for b in range(rgb.shape[0]):
        im = Image.fromarray(rgb[b], 'RGB')
        im.paste(mark_image, (0, 0), mark_image)
        marked[b] = np.asarray(im)
    rep = [np.ascontiguousarray(np.repeat(p[:, :, :, None], 3, axis=3)) for p in (gray, edge, mask)]
    return [rgb, rep[0], rep[1], rep[2], obscured, marked]


def finish_parent(transform, dev6):
    out = [transform(x) for x in dev6]
    out = [o if m in (0, 4, 5) else o[:, :1].contiguous() for m, o in enumerate(out)]
    out[3] = 1 - out[3]
    return out


def windows(fns, repeats, inner):
    """``repeats`` windows of ``inner`` calls for every function of ``fns``, alternating; seconds per call."""
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / inner)
    return times


def show(name, ts, unit=1e6, label='us'):
    ts = sorted(ts)
    fmt = '%9.1f' if label == 'us' else '%9.2f'
    print(('  %-58s median ' + fmt + ' %s   min ' + fmt + '   max ' + fmt + '   (%d windows)')
          % (name, ts[len(ts) // 2] * unit, label, ts[0] * unit, ts[-1] * unit, len(ts)))
    return ts[len(ts) // 2]


def write_tree(root, n, hw, rng):
    from PIL import Image
    from mvae_amd.vision import datasets as VD
    os.makedirs(os.path.join(root, 'Eval'))
    lines = []
    for d in (VD.IMAGE_DIR, VD.GRAY_DIR, VD.EDGE_DIR, VD.MASK_DIR):
        os.makedirs(os.path.join(root, d))
    for i in range(n):
        name = '%06d.jpg' % (i + 1)
        lines.append('%s 0' % name)
        rgb = smooth(rng, hw + (3,))
        Image.fromarray(rgb, 'RGB').save(os.path.join(root, VD.IMAGE_DIR, name), quality=90)
        Image.fromarray(rgb, 'RGB').convert('L').save(os.path.join(root, VD.GRAY_DIR, name), quality=90)
        for d in (VD.EDGE_DIR, VD.MASK_DIR):
            plane = ((smooth(rng, hw) > 128) * 255).astype(np.uint8)
            Image.fromarray(plane, 'L').save(os.path.join(root, d, name), quality=90)
    with open(os.path.join(root, VD.PARTITION_FILE), 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
    mark_path = os.path.join(root, 'watermark.png')
    mark = smooth(rng, (60, 160, 4))
    Image.fromarray(mark, 'RGBA').save(mark_path)
    return mark_path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=200, help='launches per window of the device-only figures')
    ap.add_argument('--files', type=int, default=400, help='items of the synthetic tree (one loader epoch)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this tool times GPU work: no GPU here, nothing measured')
    from PIL import Image
    import mvae_amd  # noqa: F401
    from mvae_amd import preprocess as PP
    from mvae_amd.vision import datasets as VD
    dev = torch.device('cuda', 0)
    B, H, W = args.batch, 218, 178
    rng = np.random.RandomState(7)
    rgb = np.stack([smooth(rng, (H, W, 3)) for _ in range(B)])
    edge, mask = [np.stack([smooth(rng, (H, W)) for _ in range(B)]) for _ in range(2)]
    gray = np.stack([np.asarray(Image.fromarray(x, 'RGB').convert('L')) for x in rgb])
    mark_image = Image.fromarray(smooth(rng, (60, 160, 4)), 'RGBA').resize((W, H), Image.BICUBIC)
    mark = np.array(mark_image)
    print('# %s, torch %s, Pillow %s; B = %d images of %d x %d -> 64 x 64, six modalities (12 planes)'
          % (torch.cuda.get_device_name(0), torch.__version__, Image.__version__, B, H, W))

    d_rgb, d_edge, d_mask, d_gray, d_mark = [torch.from_numpy(x).to(dev) for x in (rgb, edge, mask, gray, mark)]
    compose, transform = PP.VisionCompose(64), PP.ResizeCenterCropToTensor(64)
    host6 = host_derive(rgb, edge, mask, gray, mark_image)
    dev6 = [torch.from_numpy(x).to(dev) for x in host6]

    def one_launch():
        return compose(d_rgb, d_edge, d_mask, d_mark, gray=d_gray)

    def one_launch_luma():
        return compose(d_rgb, d_edge, d_mask, d_mark)

    def six_launches():
        return finish_parent(transform, dev6)

    def parent_whole():
        six = host_derive(rgb, edge, mask, gray, mark_image)
        return finish_parent(transform, [torch.from_numpy(x).pin_memory().to(dev, non_blocking=True) for x in six])

    def new_whole():
        up = [torch.from_numpy(x).pin_memory().to(dev, non_blocking=True) for x in (rgb, edge, mask, gray)]
        return compose(up[0], up[1], up[2], d_mark, gray=up[3])

    got, want = one_launch(), six_launches()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(got, want))
    luma_same = torch.equal(one_launch_luma()[1], got[1])            # the gray source here IS Pillow's convert('L')
    for fn in (one_launch, one_launch_luma, six_launches):
        for _ in range(20):
            fn()
    for fn in (new_whole, parent_whole):
        fn()
    print('device-resident sources, per batch (windows of %d calls, the paths alternating):' % args.inner)
    t = windows([one_launch, one_launch_luma, six_launches], args.repeats, args.inner)
    a = show('VisionCompose, gray source given (1 launch)', t[0])
    show('VisionCompose, luma in the kernel (1 launch)', t[1])
    b = show('6 x ResizeCenterCropToTensor + 3 slices + 1 - mask', t[2])
    print('  medians: %.1f us against %.1f us' % (a * 1e6, b * 1e6))
    print('host sources to device tensors, per batch (windows of 3 calls, the paths alternating):')
    t = windows([new_whole, parent_whole], args.repeats, 3)
    a = show('4 pinned uploads + VisionCompose', t[0], 1e3, 'ms')
    b = show('host derivation + 6 pinned uploads + 6 launches', t[1], 1e3, 'ms')
    t0 = time.perf_counter()
    for _ in range(3):
        host_derive(rgb, edge, mask, gray, mark_image)
    print('  of the latter, the host derivation alone: %.1f ms per batch' % ((time.perf_counter() - t0) / 3 * 1e3))
    print('  medians: %.2f ms against %.2f ms' % (a * 1e3, b * 1e3))

    root = tempfile.mkdtemp(prefix='vision_tree_')
    try:
        mark_path = write_tree(root, args.files, (H, W), np.random.RandomState(8))
        loader = VD.CelebVisionLoader('train', root, B, True, dev, seed=1, watermark_path=mark_path)
        print('CelebVisionLoader, one epoch of %d items (%d batches of %d; four JPEG files per item, quality 90, smooth '
              'synthetic content; %d decode threads):' % (args.files, len(loader), B, loader._threads))

        def epoch():
            n = 0
            for batch6 in loader:
                n += batch6[0].shape[0]
            torch.cuda.synchronize()
            assert n == args.files

        def decode_only():
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(loader._threads) as pool:
                list(pool.map(loader._decode, range(args.files)))
        epoch()
        te, td = [], []
        for _ in range(5):
            t0 = time.perf_counter(); epoch(); te.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); decode_only(); td.append(time.perf_counter() - t0)
        e = show('epoch (decode, uploads, launches)', te, 1e3, 'ms')
        d = show('the file decode alone, same threads', td, 1e3, 'ms')
        print('  %.0f items/s; the decode alone takes %.0f%% of the epoch time' % (args.files / e, 100.0 * d / e))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print('check: the one launch equals the six launches on host-derived inputs (Pillow paste), all six modalities: %s; '
          'kernel luma equals convert(\'L\'): %s' % ('yes' if same else 'NO', 'yes' if luma_same else 'NO'))
    return 0 if same and luma_same else 1


if __name__ == '__main__':
    sys.exit(main())
