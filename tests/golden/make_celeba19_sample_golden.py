#!/usr/bin/env python
"""Generate celeba19_sample.npz from the UNMODIFIED reference: conditional generation from the CelebA-19 MVAE.

Run in the build container only (needs /root/reference, which never travels):

    python tests/golden/make_celeba19_sample_golden.py

The reference has no celeba19/sample.py; what its mnist/sample.py:71-113 does is ``model.infer`` of the conditioning
modalities in eval mode, z = mu + exp(logvar / 2) * eps, and the sigmoid of the decoders.  This script does exactly that
with the reference's celeba19 ``MVAE`` for six conditions, each as a batch of 1 through ``ref.infer(image_or_None,
attrs list with None)``: image only; one attribute at 0; one attribute at 1; image plus all 18 attributes; a mixed subset
without the image; a mixed subset with the image.  Weights are ``oracle.models.fill_parameters(WEIGHT_SEED)``; one
train-mode joint forward moves the BatchNorm running statistics off 0 / 1 first (make_eval_golden.py), then ``eval()``.

Recorded per condition: mu, logvar, z for a stored eps with n = 2, the sigmoid of the first 256 image logits of each
draw and the 18 attribute probabilities; plus the BatchNorm state, the conditions (``state`` [6, 18] in {-1, 0, 1},
``img_row`` [6]) and eps.  The images are stored as a seed (``oracle.steps.synthetic_batch``).  The script asserts that the
restatement the tests use (tests/celeba19_sample_ref.py on the oracle) reproduces every value before writing.  The fixture
is data; no reference source is stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import WEIGHT_SEED, bn_stats, check, import_reference   # noqa: E402
from make_eval_golden import move_running_stats   # noqa: E402
from oracle import models as OM, steps as OS  # noqa: E402
import celeba19_sample_ref as SR  # noqa: E402

ROWS = 2            # conditioning images
N_DRAWS = 2
INPUT_SEED = 2468
EPS_SEED = 97
N_ATTRS = 18


def conditions(label):
    """(state [6, 18], img_row [6]): attribute values come from the synthetic attribute matrix where they are not fixed."""
    lab = label.long()
    state = torch.full((6, N_ATTRS), -1, dtype=torch.int64)
    img_row = torch.tensor([0, -1, -1, 1, -1, 0])
    state[1, 6] = 0                                   # Eyeglasses = 0
    state[2, 9] = 1                                   # Male = 1
    state[3] = lab[1]                                 # image 1 with all its 18 attributes
    for a in (0, 3, 9, 14, 17):                       # a mixed subset, no image
        state[4, a] = lab[0, a]
    for a in (1, 2, 6, 8, 11, 14, 16):                # a mixed subset with image 0
        state[5, a] = 1 - lab[0, a]
    return state, img_row


def main():
    torch.set_num_threads(4)
    exp = 'celeba19'
    ref_model_mod, _ = import_reference(exp)
    cls, d = OM.MODELS[exp]
    oracle = OM.fill_parameters(cls(d), WEIGHT_SEED)
    ref = ref_model_mod.MVAE(d)
    ref.load_state_dict(oracle.state_dict())
    stat_image, stat_label = OS.synthetic_batch(exp, 6, seed=4321)
    move_running_stats(ref, exp, stat_image, stat_label)
    oracle.load_state_dict(ref.state_dict())
    ref.eval(); oracle.eval()

    image, label = OS.synthetic_batch(exp, ROWS, seed=INPUT_SEED)
    state, img_row = conditions(label)
    C = state.shape[0]
    eps = torch.randn(N_DRAWS, C, d, generator=torch.Generator().manual_seed(EPS_SEED))
    fx = {'state': state.numpy().astype(np.int8), 'img_row': img_row.numpy().astype(np.int32), 'eps': eps.numpy()}
    fx.update(bn_stats(ref))
    mus, lvs, zs, imgs, attrs = [], [], [], [], []
    with torch.no_grad():
        for c in range(C):
            img = image[int(img_row[c]):int(img_row[c]) + 1] if int(img_row[c]) >= 0 else None
            lst = [state[c, a].reshape(1).float() if int(state[c, a]) >= 0 else None for a in range(N_ATTRS)]
            mu, logvar = ref.infer(img, lst)
            z = mu + logvar.mul(0.5).exp() * eps[:, c]                        # [n, D], mnist/sample.py:100-109
            mus.append(mu[0]); lvs.append(logvar[0]); zs.append(z)
            imgs.append(torch.sigmoid(ref.image_decoder(z)).reshape(N_DRAWS, -1)[:, :256])
            attrs.append(torch.sigmoid(torch.cat([ref.attr_decoders[a](z) for a in range(N_ATTRS)], dim=1)))
    fx['mu'] = torch.stack(mus).numpy()                                        # [C, D]
    fx['logvar'] = torch.stack(lvs).numpy()
    fx['z'] = torch.stack(zs, dim=1).numpy()                                   # [n, C, D]
    fx['image256'] = torch.stack(imgs, dim=1).numpy()                          # [n, C, 256]
    fx['attrs'] = torch.stack(attrs, dim=1).numpy()                            # [n, C, 18]

    out = SR.generate(oracle, image, img_row, state, eps)
    check(out['mu'], fx['mu'], 'celeba19 sample mu')
    check(out['logvar'], fx['logvar'], 'celeba19 sample logvar')
    check(out['z'], fx['z'], 'celeba19 sample z')
    check(out['image'].reshape(N_DRAWS, C, -1)[:, :, :256], fx['image256'], 'celeba19 sample image probabilities')
    check(out['attrs'], fx['attrs'], 'celeba19 sample attribute probabilities')

    meta = dict(exp=exp, n_latents=d, weight_seed=WEIGHT_SEED, rows=ROWS, input_seed=INPUT_SEED, eps_seed=EPS_SEED,
                n_draws=N_DRAWS, stats_seed=4321)
    fx['meta'] = np.array(repr(meta))
    path = os.path.join(HERE, 'celeba19_sample.npz')
    np.savez_compressed(path, **fx)
    print('celeba19_sample %7.1f KB' % (os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
