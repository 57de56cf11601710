#!/usr/bin/env python
"""Golden vectors for the vision input pipeline: what Pillow itself -- ``convert('L')``, ``paste(mark, (0, 0), mark)``,
``resize(..., BILINEAR)``, crop; the calls vision/datasets.py and torchvision's Resize / CenterCrop make -- produces on the
seeded inputs of ``tests/vision_data_ref.case_inputs``.  Only the expected outputs are stored (uint8, before the division by
255, the mask not yet inverted); the inputs are regenerated from their seeds.  Needs Pillow (12.2 when this was written):

    python tests/golden/make_vision_data_golden.py      # writes tests/golden/vision_data.npz
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import vision_data_ref as R  # noqa: E402


def pil_resize_crop(image, size):
    w, h = image.size
    nh, nw = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
    top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
    arr = np.asarray(image.resize((nw, nh), Image.BILINEAR))[top:top + size, left:left + size]
    return (arr[:, :, None] if arr.ndim == 2 else arr).transpose(2, 0, 1)


def pil_item(rgb, edge, mask, mark, gray, size):
    """The six uint8 [C, size, size] arrays of one item with Pillow's own calls."""
    image = Image.fromarray(rgb, 'RGB')
    gray_image = image.convert('L') if gray is None else Image.fromarray(gray, 'L')
    obscured = np.array(image)
    obscured[:, obscured.shape[1] // 2 + 1:, :] = 0
    marked = image.copy()
    m = Image.fromarray(mark, 'RGBA')
    marked.paste(m, (0, 0), m)
    six = [image, gray_image, Image.fromarray(edge, 'L'), Image.fromarray(mask, 'L'), Image.fromarray(obscured, 'RGB'),
           marked]
    return [pil_resize_crop(x, size) for x in six]


def main():
    out = {}
    for name, with_gray in R.golden_runs():
        x = R.case_inputs(name)
        gray = x['gray'] if with_gray else None
        B = x['rgb'].shape[0]
        items = [pil_item(x['rgb'][b], x['edge'][b], x['mask'][b], x['mark'], None if gray is None else gray[b],
                          x['size']) for b in range(B)]
        want = [np.stack([items[b][m] for b in range(B)]) for m in range(6)]
        got = R.compose_u8(x['rgb'], x['edge'], x['mask'], x['mark'], gray, x['size'])
        for m, modality in enumerate(R.MODALITIES):
            assert want[m].dtype == np.uint8 and want[m].shape == got[m].shape
            assert np.array_equal(got[m], want[m]), 'restatement != Pillow: %s %s' % (name, modality)
            out[R.golden_key(name, modality, with_gray)] = want[m]
        if not with_gray:       # the luma run differs from the gray-source run in the gray modality, and only there
            assert not np.array_equal(out[R.golden_key(name, 'gray', True)], want[1])
    out['meta'] = np.array(repr({'pillow': Image.__version__, 'cases': dict(R.CASES), 'gray_twice': R.GRAY_TWICE}))
    path = os.path.join(HERE, 'vision_data.npz')
    np.savez_compressed(path, **out)
    print('wrote vision_data.npz: %d runs, %d bytes, Pillow %s' % (len(R.golden_runs()), os.path.getsize(path),
                                                                   Image.__version__))


if __name__ == '__main__':
    main()
