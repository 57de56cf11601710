"""The ``loglike.py`` the reference's README lists for this experiment ("to compute the marginal log likelihood
``log p(x)`` using ``q(z|x,y)`` as the inference network") and never published: the importance-weighted estimate of
../loglike.py on a trained checkpoint.  ``label`` is the clothing class (int64 [N]).

    python fashionmnist/loglike.py model_best.pth.tar --cuda --n-samples 1000 --batch-size 64 \\
        [--score image|label|image,label] [--given image|label|image,label] (--synthetic | --data-file FILE.npz)

Prints one line: the mean of L over the data and its standard error."""
import os
import sys

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.fashionmnist'

from ..loglike import main  # noqa: E402
from .train import load_checkpoint  # noqa: E402

if __name__ == "__main__":
    sys.exit(main('fashionmnist', load_checkpoint, (1, 28, 28)))
