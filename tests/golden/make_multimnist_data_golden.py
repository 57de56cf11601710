"""Writes tests/golden/multimnist_data.npz: the MultiMNIST compose step (resize every digit of a plan to w x w, paste,
sum, flag sums above 255) computed with Pillow ITSELF -- ``Image.fromarray(digit).resize((w, w), Image.BILINEAR)`` --
on a synthetic bank of 12 "digits" (zero background with a centred 12 x 12 block of random 130..255; the last two
full-frame noise) and 40 random plans: 0-4 digits per canvas, widths 7..50, any legal position.

    python tests/golden/make_multimnist_data_golden.py

Needs Pillow (the golden was written with 12.2.0).  tests/multimnist_data_ref.py must reproduce every canvas and flag
from the bank and the plans; so must the HIP kernel.
"""
import os
import sys

import numpy as np
from PIL import Image
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import multimnist_data_ref as R  # noqa: E402


def pillow_resize(digit, w):
    return np.asarray(Image.fromarray(digit).resize((w, w), Image.BILINEAR), dtype=np.uint8)


def main():
    bank = R.block_bank(seed=7, n=12)
    rng = np.random.RandomState(20)
    canvases = []
    for m in range(40):
        records = []
        for _ in range(m % 5):
            w = int(rng.randint(7, 51))
            records.append((int(rng.randint(12)), w, int(rng.randint(0, 51 - w)), int(rng.randint(0, 51 - w))))
        canvases.append(records)
    plan = R.make_plan(canvases)
    canvas, flags = R.compose(bank, plan, resize=pillow_resize)
    meta = {'pillow': PIL.__version__, 'n_bank': 12, 'M': int(plan.shape[0]), 'flagged': int(flags.sum())}
    np.savez_compressed(os.path.join(HERE, 'multimnist_data.npz'), bank=bank, plan=plan, canvas=canvas, flags=flags,
                        meta=np.array(repr(meta)))
    print(meta)


if __name__ == '__main__':
    main()
