"""HIP drop-in for the reference's ``celeba19/`` experiment (model.py, train.py), and its evaluation: ``loglike.py``, the
importance-weighted image marginal, 18 attribute marginals and joint (``from mvae_amd.celeba19 import loglike``)."""
from . import model  # noqa: F401
