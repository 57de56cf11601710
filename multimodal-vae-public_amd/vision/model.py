"""Vision MVAE (six image modalities of one CelebA face: colour, gray, edge, mask, obscured, watermarked) on HIP --
drop-in for the reference's ``vision/model.py``.

    MVAE              vision/model.py:12-100    six encoders, six decoders, prior + up to six experts in the PoE
    ImageEncoder      vision/model.py:109-145   celeba's conv stack with ``n_channels`` in {1, 3}
    ImageDecoder      vision/model.py:148-180   celeba's transposed-conv stack with ``n_channels`` in {1, 3}
    ProductOfExperts variant A                  vision/model.py:183-196 (eps added twice and inside the log)

The reference text does not run; what is built is its documented behaviour with the defects that prevent running
repaired, and everything that would run kept as written:

    :32      a stray backtick after ``self.use_cuda = use_cuda`` -- ignored
    :56-57   ``forward`` returns the undefined ``rotated_recon`` -- it returns (image_recon, gray_recon, edge_recon,
             mask_recon, obscured_recon, watermark_recon, mu, logvar), the order vision/train.py:186-189 unpacks
    kept     ``n_latents`` defaults to 250; the inference method is called ``get_params`` (``infer`` is an alias, the
             name the other experiments and ``sample_common`` use)
"""
import torch.nn as nn

from .. import layers as L
from ..base import MVAEBase, Stack
# module-level names of the reference's model.py: ProductOfExperts here is variant A -- vision/model.py:183-196
from ..base import ProductOfExperts, prior_expert  # noqa: F401
from ..celeba.model import _owner_mvae
from ..layers import Swish  # noqa: F401

MODALITIES = ('image', 'gray', 'edge', 'mask', 'obscured', 'watermark')
N_CHANNELS = {'image': 3, 'gray': 1, 'edge': 1, 'mask': 1, 'obscured': 3, 'watermark': 3}   # vision/model.py:16-28


def get_batch_size(*args):
    """vision/model.py:103-106."""
    for arg in args:
        if arg is not None:
            return arg.size(0)


class ImageEncoder(Stack):
    def __init__(self, n_latents, n_channels=3):
        super().__init__()
        self.features = nn.Sequential(
            L.Conv2d(n_channels, 32, 4, 2, 1, bias=False), L.Swish(),
            L.Conv2d(32, 64, 4, 2, 1, bias=False), L.BatchNorm2d(64), L.Swish(),
            L.Conv2d(64, 128, 4, 2, 1, bias=False), L.BatchNorm2d(128), L.Swish(),
            L.Conv2d(128, 256, 4, 1, 0, bias=False), L.BatchNorm2d(256), L.Swish())
        self.classifier = nn.Sequential(
            L.Linear(256 * 5 * 5, 512), L.Swish(), L.Dropout(p=0.1), L.Linear(512, n_latents * 2))
        self.n_latents = n_latents

    def stack_modules(self):
        return [self.features, L.View(256 * 5 * 5), self.classifier]

    # the fused step runs the trunk once per batch and fans the two Dropout draws of a step out (train.fused_step)
    def trunk_plan(self):
        p = self.__dict__.get('_trunk_plan')
        if p is None:
            p = L.compile_plan([self.features, L.View(256 * 5 * 5), self.classifier[0], self.classifier[1]])
            self.__dict__['_trunk_plan'] = p
        return p

    def head_plan(self):
        p = self.__dict__.get('_head_plan')
        if p is None:
            p = self.__dict__['_head_plan'] = L.compile_plan([self.classifier[3]])
        return p

    def heads(self, x, dropout_mask=None):
        masks = None
        if self.training:
            if dropout_mask is None:
                dropout_mask = _owner_mvae(self).device_bernoulli(0.9, x.shape[0], 512)
            masks = [dropout_mask.contiguous().float()]
        return self.run(x, masks=masks)

    def forward(self, x, dropout_mask=None):
        h = self.heads(x, dropout_mask)
        return h[:, :self.n_latents], h[:, self.n_latents:]


class ImageDecoder(Stack):
    def __init__(self, n_latents, n_channels=3):
        super().__init__()
        self.upsample = nn.Sequential(L.Linear(n_latents, 256 * 5 * 5), L.Swish())
        self.hallucinate = nn.Sequential(
            L.ConvTranspose2d(256, 128, 4, 1, 0, bias=False), L.BatchNorm2d(128), L.Swish(),
            L.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), L.BatchNorm2d(64), L.Swish(),
            L.ConvTranspose2d(64, 32, 4, 2, 1, bias=False), L.BatchNorm2d(32), L.Swish(),
            L.ConvTranspose2d(32, n_channels, 4, 2, 1, bias=False))

    def stack_modules(self):
        return [self.upsample, L.View(256, 5, 5), self.hallucinate]

    def forward(self, z):
        return self.run(z)  # NOTE: logits, no sigmoid


class MVAE(MVAEBase):
    POE_VARIANT = 'A'
    KIND = 'vision'
    HAS_BN = True

    def __init__(self, n_latents=250, use_cuda=False):
        super().__init__(n_latents)
        for name in MODALITIES:
            setattr(self, name + '_encoder', ImageEncoder(n_latents, N_CHANNELS[name]))
        for name in MODALITIES:
            setattr(self, name + '_decoder', ImageDecoder(n_latents, N_CHANNELS[name]))
        for enc in self.encoders():
            enc.__dict__['_owner'] = self
        self.use_cuda = use_cuda
        self.__dict__['last_z'] = None

    def encoders(self):
        return [getattr(self, name + '_encoder') for name in MODALITIES]

    def decoders(self):
        return [getattr(self, name + '_decoder') for name in MODALITIES]

    def arena_order(self):
        return self.decoders() + self.encoders()

    def forward(self, image=None, gray=None, edge=None, mask=None, obscured=None, watermark=None, eps=None,
                dropout_masks=None):
        """Returns (image_recon, gray_recon, edge_recon, mask_recon, obscured_recon, watermark_recon, mu, logvar): all
        six decoders run on the one z, whichever modalities were given (vision/model.py:42-57).  Parity runs pass the
        noise: ``eps`` [B, D] and ``dropout_masks``, six entries in modality order ([B, 512] keep-masks, None for an
        absent modality); otherwise it comes from the model's device Philox stream.  The z used is left in
        ``last_z``."""
        mu, logvar, z = self._infer((image, gray, edge, mask, obscured, watermark), eps, dropout_masks, want_z=True)
        self.__dict__['last_z'] = z
        return tuple(dec(z) for dec in self.decoders()) + (mu, logvar)

    def get_params(self, image=None, gray=None, edge=None, mask=None, obscured=None, watermark=None):
        """vision/model.py:59-100: (mu, logvar) of the product of the prior and the encoders of the inputs given."""
        mu, logvar, _ = self._infer((image, gray, edge, mask, obscured, watermark), None, None, want_z=False)
        return mu, logvar

    infer = get_params

    def _infer(self, inputs, eps, dropout_masks, want_z):
        self.finalize()
        if dropout_masks is None:
            dropout_masks = (None,) * len(MODALITIES)
        if len(dropout_masks) != len(MODALITIES):
            raise ValueError('dropout_masks: one entry per modality (None for an absent one)')
        heads = [enc.heads(x, m) for enc, x, m in zip(self.encoders(), inputs, dropout_masks) if x is not None]
        if not heads:
            raise ValueError('at least one modality is required')
        return self._fuse(heads, eps, want_z)
