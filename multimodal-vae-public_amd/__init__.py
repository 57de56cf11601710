"""multimodal-vae-public_amd -- the MVAE train step of mhw32/multimodal-vae-public as hand-written
HIP kernels for MI355X (gfx950), behind the reference's own Python surface.

Import as ``import mvae_amd`` (alias module at the repo root; the directory name carries a
hyphen) or ``importlib.import_module('multimodal-vae-public_amd')``.

    mvae_amd.mnist.model.MVAE / .fashionmnist / .celeba / .celeba19   drop-in nn.Modules
    mvae_amd.functional.elbo_loss_*                                   the reference's loss functions
    mvae_amd.engine.BimodalStep / Celeba19Step                        fused, graph-captured train step
    mvae_amd.optim.FusedAdam                                          one-launch Adam over the arena
    mvae_amd.parallel.DataParallel                                    RCCL gradient all-reduce
    mvae_amd.capture_step(body, example_args, model=, optimizer=)     the reference's unchanged loop body as ONE hipGraph
    mvae_amd.log_likelihood(model, image=, label=, score=, given=)    importance-weighted marginal log-likelihood
    mvae_amd.vision.loglike.log_likelihood(model, data, score=, given=)   the same for the six vision modalities + joint
    mvae_amd.celeba19.loglike.log_likelihood(model, image=, attrs=, score=, given=)   CelebA-19: image, 18 attributes + joint
                                                                      (``from mvae_amd.celeba19 import loglike``)
    mvae_amd.predict.predict(model, image, given=, n_samples=)        the label the model predicts from the image
    mvae_amd.predict.evaluate(model, image, label, confusion=)        ... scored: nll, correct, confusion counts
                                                                      (also ``mvae_amd.predict_label`` / ``mvae_amd.evaluate``)
    mvae_amd.partial.PartialStep(model, lambda_image, lambda_label)   weak supervision: a train step on rows that observe
                                                                      only some modalities (mnist, fashionmnist)
"""
from . import _lib, kernels, arena, layers, functional, base, engine, optim, parallel, graph  # noqa: F401
from .graph import capture_step  # noqa: F401
from . import loglike  # noqa: F401
from .loglike import log_likelihood  # noqa: F401
from . import predict  # noqa: F401
from .predict import predict as predict_label, evaluate  # noqa: F401  (``predict`` itself names the module)
from . import partial  # noqa: F401
from . import mnist, fashionmnist, celeba, celeba19  # noqa: F401

__all__ = ['kernels', 'arena', 'layers', 'functional', 'base', 'engine', 'optim', 'parallel', 'graph', 'capture_step',
           'loglike', 'log_likelihood', 'predict', 'predict_label', 'evaluate', 'partial',
           'mnist', 'fashionmnist', 'celeba', 'celeba19']
