"""Test helper (not a test): the MultiMNIST image stacks and MVAE restated on plain torch CPU ops, with every noise
draw an explicit input.

Written from the layer table of multimnist/model.py -- encoder: Conv2d(1,32,4,2,1) Swish, Conv2d(32,64,4,2,1) BN Swish,
Conv2d(64,128,4,2,1) BN Swish, Conv2d(128,256,4,2,0) BN Swish, Linear(1024,512) Swish Dropout(0.1) Linear(512,2D); decoder:
Linear(D,1024) Swish, ConvTranspose2d(256,128,4,2,0) BN Swish, ConvTranspose2d(128,64,4,2,1) BN Swish,
ConvTranspose2d(64,32,5,2,1) BN Swish, ConvTranspose2d(32,1,4,2,1); maps 50 -> 25 -> 12 -> 6 -> 2 and back -- on
``nn.Conv2d`` / ``nn.ConvTranspose2d`` / ``nn.BatchNorm2d``, composed with ``oracle.multimnist``'s text stacks and
``oracle.functional``'s PoE / reparametrisation / losses.  ``state_dict`` keys equal the reference's.
tests/golden/make_multimnist_mvae_golden.py asserts that it reproduces the unmodified reference."""
import torch
import torch.nn as nn

from oracle import functional as OF, multimnist as OMM
from oracle.models import Swish, _MaskedDropout


class ImageEncoder(nn.Module):
    def __init__(self, n_latents):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 32, 4, 2, 1, bias=False), Swish(),
            nn.Conv2d(32, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.Conv2d(64, 128, 4, 2, 1, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.Conv2d(128, 256, 4, 2, 0, bias=False), nn.BatchNorm2d(256), Swish())
        self.classifier = nn.Sequential(
            nn.Linear(256 * 2 * 2, 512), Swish(), _MaskedDropout(0.1), nn.Linear(512, n_latents * 2))
        self.n_latents = n_latents

    def forward(self, x, dropout_mask=None):
        self.classifier[2].mask = dropout_mask
        h = self.classifier(self.features(x).reshape(-1, 256 * 2 * 2))
        return h[:, :self.n_latents], h[:, self.n_latents:]


class ImageDecoder(nn.Module):
    def __init__(self, n_latents):
        super().__init__()
        self.upsample = nn.Sequential(nn.Linear(n_latents, 256 * 2 * 2), Swish())
        self.hallucinate = nn.Sequential(
            nn.ConvTranspose2d(256, 128, 4, 2, 0, bias=False), nn.BatchNorm2d(128), Swish(),
            nn.ConvTranspose2d(128, 64, 4, 2, 1, bias=False), nn.BatchNorm2d(64), Swish(),
            nn.ConvTranspose2d(64, 32, 5, 2, 1, bias=False), nn.BatchNorm2d(32), Swish(),
            nn.ConvTranspose2d(32, 1, 4, 2, 1, bias=False))

    def forward(self, z):
        return self.hallucinate(self.upsample(z).reshape(-1, 256, 2, 2))


class TextDecoder(OMM.TextDecoder):
    """``oracle.multimnist.TextDecoder`` with the start characters and self-drawn masks on ``z``'s device, so that the
    restatement can also run on a GPU (tools/multimnist_step_bench.py steps it there as the baseline); same arithmetic."""
    def forward(self, z, dropout_masks=None):
        B = z.shape[0]
        if self.training and dropout_masks is None:
            dropout_masks = [torch.empty(B, self.n_hiddens, device=z.device).bernoulli_(OMM.KEEP) for _ in range(OMM.MAX_LENGTH)]
        c_in = torch.full((B,), OMM.SOS, dtype=torch.long, device=z.device)
        h0 = h1 = self.z2h(z)
        words, fed = [], []
        for i in range(OMM.MAX_LENGTH):
            fed.append(c_in)
            x = torch.cat((OF.swish(self.embed(c_in)), z), dim=1)
            h0 = OMM.gru_cell(x, h0, *OMM._gru_params(self.gru, 0))
            d = h0 * dropout_masks[i].to(z.device) / OMM.KEEP if self.training else h0
            h1 = OMM.gru_cell(d, h1, *OMM._gru_params(self.gru, 1))
            c_out = self.h2o(torch.cat((h1, z), dim=1))
            words.append(c_out)
            c_in = torch.max(torch.log_softmax(c_out, dim=1), dim=1)[1]
        return torch.stack(words, dim=1), torch.stack(fed)


class MVAE(nn.Module):
    def __init__(self, n_latents):
        super().__init__()
        self.image_encoder = ImageEncoder(n_latents)
        self.image_decoder = ImageDecoder(n_latents)
        self.text_encoder = OMM.TextEncoder(n_latents)
        self.text_decoder = TextDecoder(n_latents)
        self.n_latents = n_latents
        self.last_fed = None

    def infer(self, image=None, text=None, dropout_mask=None):
        mus, lvs = [], []
        if image is not None:
            m, v = self.image_encoder(image, dropout_mask)
            mus.append(m); lvs.append(v)
        if text is not None:
            m, v = self.text_encoder(text)
            mus.append(m); lvs.append(v)
        prior = torch.zeros(1, *mus[0].shape, device=mus[0].device)          # the N(0, 1) expert first, then the present ones
        return OF.poe(torch.cat([prior] + [m.unsqueeze(0) for m in mus], dim=0),
                      torch.cat([prior] + [v.unsqueeze(0) for v in lvs], dim=0), 'B')

    def forward(self, image=None, text=None, eps=None, dropout_mask=None, text_dropout_masks=None):
        """Parity runs pass ``eps`` [B, D], ``dropout_mask`` [B, 512] (when an image is given) and the four GRU masks; a
        training-mode call without them draws them on the parameters' device.
        Returns (img_recon, txt_recon, mu, logvar, z); the fed-back characters are left in ``last_fed``."""
        mu, logvar = self.infer(image, text, dropout_mask)
        if self.training and eps is None:
            eps = torch.randn_like(mu)
        z = OF.reparametrize(mu, logvar, eps if self.training else None)
        words, self.last_fed = self.text_decoder(z, dropout_masks=text_dropout_masks)
        return self.image_decoder(z), words, mu, logvar, z


def elbo_loss(recon_image, image, recon_text, text, mu, logvar, lambda_image=1.0, lambda_text=1.0, annealing_factor=1):
    """The three terms of multimnist/train.py's ELBO: image BCE over 2500 pixels, text cross-entropy over the 12 classes
    and 4 positions, KL; weighted mean over the batch."""
    image_bce, text_bce = 0, 0
    if recon_image is not None and image is not None:
        image_bce = OF.binary_cross_entropy_with_logits(recon_image.reshape(-1, 2500), image.reshape(-1, 2500)).sum(dim=1)
    if recon_text is not None and text is not None:
        text_bce = OMM.text_loss_rows(recon_text, text)
    return torch.mean(lambda_image * image_bce + lambda_text * text_bce + annealing_factor * OF.kl_rows(mu, logvar))


def draw_call_noise(batch, n_latents, with_image, generator=None):
    """One ``model()`` call's draws in the reference's order: the image encoder's Bernoulli(0.9) mask [B, 512] when an
    image is given, eps [B, D], then the four GRU masks."""
    mask = torch.empty(batch, 512).bernoulli_(0.9, generator=generator) if with_image else None
    eps = torch.empty(batch, n_latents).normal_(generator=generator)
    return {'mask': mask, 'eps': eps, 'gru': OMM.draw_decoder_masks(batch, generator=generator)}


CALLS = ((True, True), (True, False), (False, True))       # (image, text) of the step's three model() calls


def three_call_step(model, image, text, noise, lambda_image, lambda_text, annealing_factor, elbo=elbo_loss):
    """The reference's loop body without the optimizer: returns (total, [joint, image, text] terms, per-call outputs)."""
    terms, outs = [], []
    if noise is None:
        noise = [{'eps': None, 'mask': None, 'gru': None}] * 3
    for (wi, wt), nz in zip(CALLS, noise):
        out = model(image if wi else None, text if wt else None, eps=nz['eps'], dropout_mask=nz['mask'],
                    text_dropout_masks=nz['gru'])
        outs.append(out)
        terms.append(elbo(out[0] if wi else None, image if wi else None, out[1] if wt else None, text if wt else None,
                          out[2], out[3], lambda_image=lambda_image, lambda_text=lambda_text,
                          annealing_factor=annealing_factor))
    return terms[0] + terms[1] + terms[2], terms, outs


def argmax_margin(words):
    """min over (sample, fed-back position) of (top-1 - top-2 logit) / max|logit| of a [B, 4, 12] logits tensor (the
    arg-max of the last position is not fed back): the greedy feedback is safe against 1e-6-level differences when this
    is well above them."""
    top = torch.topk(words.detach()[:, :OMM.MAX_LENGTH - 1], 2, dim=2).values
    return ((top[..., 0] - top[..., 1]).min() / words.detach().abs().max()).item()
