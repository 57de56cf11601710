"""GPU: ``vision/train.py`` without ``--synthetic`` as a fresh child process -- one epoch from a tree of PNG files through
``CelebVisionLoader``, a finite test loss and the checkpoint ``load_checkpoint`` reads."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd.vision import model as VM, train as VT
from test_vision_data_cpu import make_vision_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VISION = os.path.join(ROOT, 'multimodal-vae-public_amd', 'vision')


def test_train_cli_trains_one_epoch_from_files(tmp_path):
    data, out_dir = str(tmp_path / 'data'), str(tmp_path / 'out')
    os.makedirs(data)
    _, mark_path = make_vision_tree(data, counts=(6, 2, 0), hw=(64, 64), seed=12)
    r = subprocess.run([sys.executable, os.path.join(VISION, 'train.py'), '--cuda', '--epochs', '1', '--batch-size', '2',
                        '--n-latents', '8', '--data-dir', data, '--watermark-file', mark_path, '--out-dir', out_dir],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=240)
    out = r.stdout
    assert r.returncode == 0, out[-3000:]
    assert 'Train Epoch: 1 [0/6 (0%)]' in out, out[-3000:]            # six files of the train partition, three batches
    line = [ln for ln in out.splitlines() if ln.startswith('====> Epoch: 1')]
    assert line and np.isfinite(float(line[0].split('Loss:')[1])), out[-3000:]
    test_line = [ln for ln in out.splitlines() if ln.startswith('====> Test Loss:')]
    assert test_line and np.isfinite(float(test_line[0].split(':')[1])), out[-3000:]
    path = os.path.join(out_dir, 'checkpoint.pth.tar')
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['best_loss', 'n_latents', 'optimizer', 'state_dict'] and ckpt['n_latents'] == 8
    model = VT.load_checkpoint(path)
    assert isinstance(model, VM.MVAE) and all(torch.isfinite(v).all() for v in model.state_dict().values())
    for name, v in model.state_dict().items():                       # three train batches: 2 / 7 BatchNorm updates each
        if name.endswith('num_batches_tracked'):
            assert int(v) == 3 * (2 if '_encoder.' in name else 7), name
    for m in VM.MODALITIES:
        assert os.path.exists(os.path.join(out_dir, 'results', m, 'reconstruction_1.png'))
