"""Which label does a trained checkpoint predict from the image alone, and how often is it right: ../predict.py on this
experiment.  ``label`` is the digit string (int64 [N, 4], FILL-padded).

    python multimnist/predict.py model_best.pth.tar --cuda [--n-samples 0] [--batch-size N] [--chunk-rows 4096] [--seed 0] \\
        [--out-dir DIR] (--synthetic [--n-data N] | --data-file FILE.npz)

Prints the per-position accuracy, the exact-match rate of whole strings and the confusion matrix.
The same text is written to ``predict.txt`` under --out-dir."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.multimnist'

from ..predict import main  # noqa: E402
from .train import load_checkpoint  # noqa: E402

if __name__ == "__main__":
    sys.exit(main('multimnist', load_checkpoint, (1, 50, 50)))
