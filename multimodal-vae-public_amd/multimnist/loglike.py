"""The ``loglike.py`` the reference's README lists for this experiment ("to compute the marginal log likelihood
``log p(x)`` using ``q(z|x,y)`` as the inference network") and never published: the importance-weighted estimate of
../loglike.py on a trained checkpoint.  ``label`` is the digit string (int64 [N, 4], FILL-padded).

    python multimnist/loglike.py model_best.pth.tar --cuda --n-samples 1000 --batch-size 64 \\
        [--score image|label|image,label] [--given image|label|image,label] (--synthetic | --data-file FILE.npz)

Prints one line: the mean of L over the data and its standard error."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.multimnist'

from ..loglike import main  # noqa: E402
from .train import load_checkpoint  # noqa: E402

if __name__ == "__main__":
    sys.exit(main('multimnist', load_checkpoint, (1, 50, 50)))
