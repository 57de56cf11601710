"""Which label does a trained checkpoint predict from the image alone, and how often is it right: ../predict.py on this
experiment.  ``label`` is the clothing class (int64 [N]).

    python fashionmnist/predict.py model_best.pth.tar --cuda [--n-samples 0] [--batch-size N] [--chunk-rows 4096] [--seed 0] \\
        [--out-dir DIR] (--synthetic [--n-data N] | --data-file FILE.npz)

Prints the accuracy, the mean NLL with its standard error and the confusion matrix.
The same text is written to ``predict.txt`` under --out-dir."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.fashionmnist'

from ..predict import main  # noqa: E402
from .train import load_checkpoint  # noqa: E402

if __name__ == "__main__":
    sys.exit(main('fashionmnist', load_checkpoint, (1, 28, 28)))
