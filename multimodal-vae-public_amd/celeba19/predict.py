"""Which label does a trained checkpoint predict from the image alone, and how often is it right: ../predict.py on this
experiment.  ``label`` is the [N, 18] {0, 1} attribute matrix.

    python celeba19/predict.py model_best.pth.tar --cuda [--n-samples 0] [--batch-size N] [--chunk-rows 4096] [--seed 0] \\
        [--out-dir DIR] (--synthetic [--n-data N] | --data-file FILE.npz)

Prints per named attribute the accuracy, the 2 x 2 table and the rate of the more frequent class.
The same text is written to ``predict.txt`` under --out-dir."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.celeba19'

from ..predict import main  # noqa: E402
from .train import load_checkpoint  # noqa: E402

if __name__ == "__main__":
    sys.exit(main('celeba19', load_checkpoint, (3, 64, 64)))
