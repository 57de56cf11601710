"""Weakly supervised training of the bimodal MVAEs without BatchNorm or Dropout (mnist, fashionmnist): a batch whose
rows observe different modalities, each ELBO term evaluated only on the rows that have its modalities.

The reference has no counterpart -- its loop runs the joint, image-only and label-only terms on every row
(mnist/train.py:197-218) -- but the experiment is the paper's (accuracy against the number of paired
examples).  Semantics:

    present [B]   bit 0 = image observed, bit 1 = label observed; a row with neither is a ValueError
    paired  [B]   whether a row's two modalities are known to belong together (default: all ones)
    terms         joint (both bits and paired) | image-only (bit 0) | label-only (bit 1), the reference's order
    objective     (1 / B) * sum over terms t and the rows b active in t of
                  lambda_image * BCE + lambda_label * CE + beta * KL,   one reparameterised draw per (t, b)

The divisor is the batch size, so a fully observed, fully paired batch gives the reference's three-term step and a
row's contribution does not depend on its neighbours.  An absent modality of a row is never read, by a loss or by an
encoder; parameters no active term reaches get a zero gradient.

``plan``         host: flags -> compact row order and index tables (one upload)
``PartialStep``  eager step on the drop-in modules: encoders on the rows that have their modality, ONE ragged PoE launch
                 (csrc/poe_ragged.hip), each decoder once on its contiguous slice, indexed losses (csrc/loss_ragged.hip)
``paired_subset`` / ``batch_flags`` / ``synthetic_flags``   the ``--n-paired`` protocol of mnist / fashionmnist train.py
"""
import numpy as np
import torch

from . import kernels as K
from .functional import BceRowsIndexedFn, CeRowsIndexedFn, RaggedPoEFn, RaggedTermSumsFn, _coef_tensor

IMAGE, LABEL = 1, 2                       # bits of ``present``
TERM_MASKS = (IMAGE | LABEL, IMAGE, LABEL)      # experts of the joint / image-only / label-only term (expert e = bit e)
N_TERMS, N_EXPERTS = 3, 2


class Tables(object):
    """The device side of a ``Plan``: int32 views of ONE uploaded buffer."""
    __slots__ = ('slot', 'row_of', 'erow', 'expert_rows', 'masks', 'R', 'B')


class Plan(object):
    """What ``plan`` computes; all arrays on the host (numpy int32).

    n            rows of each term, reference order [joint, image, label];  R = their sum
    n_img, n_joint, n_lbl     the same by name
    slot [3, B]  compact row of (term, batch row), -1 where the term is not evaluated on the row
    row_of [R]   batch row of a compact row
    expert_rows  per expert (0 = image, 1 = label) the batch rows that have it, ascending
    erow [2, B]  a batch row's row inside that expert's compact head buffer, or -1
    image_slice / label_slice   the compact rows the image / label decoder reads: [0, n_img + n_joint) and [n_img, R)
    """

    def __init__(self, present, paired):
        B = present.shape[0]
        has_img, has_lbl = (present & IMAGE) != 0, (present & LABEL) != 0
        active = [has_img & has_lbl & (paired != 0), has_img, has_lbl]            # reference term order
        self.B = B
        self.present, self.paired = present, paired
        self.n = [int(a.sum()) for a in active]
        self.n_joint, self.n_img, self.n_lbl = self.n
        self.R = sum(self.n)
        # compact order [image-only | joint | label-only], ascending in b inside a term: the image decoder reads
        # z[0 : n_img + n_joint] and the label decoder z[n_img : R], both contiguous, no copies
        self.offset = [self.n_img, 0, self.n_img + self.n_joint]                  # first compact row of each term
        self.slot = np.full((N_TERMS, B), -1, dtype=np.int32)
        self.row_of = np.empty(self.R, dtype=np.int32)
        for t in range(N_TERMS):
            rows = np.flatnonzero(active[t]).astype(np.int32)
            self.slot[t, rows] = self.offset[t] + np.arange(rows.size, dtype=np.int32)
            self.row_of[self.offset[t]:self.offset[t] + rows.size] = rows
        self.expert_rows = [np.flatnonzero(h).astype(np.int32) for h in (has_img, has_lbl)]
        self.erow = np.full((N_EXPERTS, B), -1, dtype=np.int32)
        for e, rows in enumerate(self.expert_rows):
            self.erow[e, rows] = np.arange(rows.size, dtype=np.int32)
        self.image_slice = (0, self.n_img + self.n_joint)
        self.label_slice = (self.n_img, self.R)
        self.masks = np.asarray(TERM_MASKS, dtype=np.int32)

    def to(self, device):
        """The index tables on ``device``, in one upload."""
        parts = [self.slot.reshape(-1), self.row_of, self.erow.reshape(-1), self.expert_rows[0], self.expert_rows[1],
                 self.masks]
        flat = torch.from_numpy(np.concatenate(parts)).to(device)
        views, lo = [], 0
        for p in parts:
            views.append(flat[lo:lo + p.size])
            lo += p.size
        t = Tables()
        t.slot = views[0].view(N_TERMS, self.B)
        t.row_of = views[1]
        t.erow = views[2].view(N_EXPERTS, self.B)
        t.expert_rows = [views[3], views[4]]
        t.masks = views[5]
        t.R, t.B = self.R, self.B
        return t


def _host_ints(x, what):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()          # a device tensor is read back here: hand host flags to avoid the sync
    a = np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in 'iub':
        raise ValueError('%s must be a 1-D integer array, got %s %s' % (what, a.dtype, a.shape))
    return a.astype(np.int32)


def plan(present, paired=None):
    """The compact layout of a batch from its row flags (host arrays; see the module text and ``Plan``)."""
    present = _host_ints(present, 'present')
    if present.size == 0:
        raise ValueError('an empty batch has no plan')
    if ((present & ~(IMAGE | LABEL)) != 0).any():
        raise ValueError('present holds bits beyond image (1) and label (2)')
    if (present == 0).any():
        raise ValueError('row %d observes no modality (present == 0)' % int(np.flatnonzero(present == 0)[0]))
    if paired is None:
        paired = np.ones(present.shape[0], dtype=np.int32)
    else:
        paired = _host_ints(paired, 'paired')
        if paired.shape != present.shape:
            raise ValueError('paired has %d entries for %d rows' % (paired.shape[0], present.shape[0]))
    return Plan(present, paired)


# ----------------------------------------------------------------------------- the --n-paired protocol
def paired_subset(n_total, n_paired, seed):
    """bool [n_total]: the ``n_paired`` training examples that keep their pairing -- the head of a seeded permutation
    of the training set's indices, so the subset is the same in every epoch and for the same seed."""
    if not 0 <= n_paired <= n_total:
        raise ValueError('--n-paired %d outside 0..%d (the size of the training set)' % (n_paired, n_total))
    keep = np.zeros(n_total, dtype=bool)
    keep[np.random.RandomState(seed).permutation(n_total)[:n_paired]] = True
    return keep


def batch_flags(is_paired, mode):
    """(present, paired) of a batch from its rows' membership in the paired subset.
    'keep': unpaired rows still observe both modalities, only the joint term is off (the paper's protocol).
    'drop': unpaired rows have no label at all and feed the image-only term alone."""
    is_paired = np.asarray(is_paired, dtype=bool)
    if mode == 'keep':
        return np.full(is_paired.shape[0], IMAGE | LABEL, dtype=np.int32), is_paired.astype(np.int32)
    if mode == 'drop':
        return np.where(is_paired, IMAGE | LABEL, IMAGE).astype(np.int32), np.ones(is_paired.shape[0], dtype=np.int32)
    raise ValueError("--unpaired-labels is 'keep' or 'drop', got %r" % (mode,))


def synthetic_flags(batch, fraction, seed, batch_idx):
    """bool [batch]: round(fraction * batch) rows of a synthetic batch flagged as paired, chosen from (seed, batch_idx)."""
    k = int(round(fraction * batch))
    keep = np.zeros(batch, dtype=bool)
    keep[np.random.RandomState([seed & 0x7fffffff, batch_idx]).permutation(batch)[:k]] = True
    return keep


# ----------------------------------------------------------------------------- the step
class PartialStep(object):
    """Eager ragged train step (forward, losses, backward) for ``mnist`` / ``fashionmnist`` MVAEs.  The caller steps
    ``FusedAdam``.  There is no hipGraph capture: the number of compact rows changes from batch to batch."""

    def __init__(self, model, lambda_image=1.0, lambda_label=1.0, seed=0):
        if getattr(model, 'HAS_BN', True) or getattr(model, 'LABEL_KIND', None) != 'class' or any(
                isinstance(m, torch.nn.Dropout) for m in model.modules()):
            raise ValueError('PartialStep is defined for the MVAEs without BatchNorm and Dropout (mnist, fashionmnist): '
                             'a term on a sub-batch must equal that term on those rows')
        model.finalize()
        self.model = model
        self.D = model.n_latents
        self.dev = next(model.parameters()).device
        self.lambda_image, self.lambda_label = float(lambda_image), float(lambda_label)
        self.seed = int(seed) or 1
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.dev)      # Philox launch index of the next draw
        self.last_plan = None
        self.noise = None
        self.last_logits = (None, None)     # (image, label) logits of the last step's compact rows (tests)

    def _flags(self, label, present, paired):
        if present is None:
            # the convenience default: the image is always there, the label where it is not the -1 sentinel
            lab = label.detach().cpu().numpy() if torch.is_tensor(label) else np.asarray(label)
            present = np.where(lab >= 0, IMAGE | LABEL, IMAGE).astype(np.int32)
        return plan(present, paired)

    def _row_coefs(self, weight, B, n):
        return _coef_tensor([weight], B, self.dev).expand(n).contiguous()

    def step(self, image, label, annealing_factor, present=None, paired=None, noise=None):
        """One forward + backward; gradients land in ``p.grad`` (the arena).  ``noise``: dense [3, B, D] in the
        reference's term order (tests), else drawn on the device at the dense Philox index of (t, b).  Returns
        ``[joint, image, label, total]`` on the device.

        Precondition: a row flagged label-present holds a label in 0..9.  The flags live on the host and the labels on
        the device, so the step does not check it.  Nothing is indexed out of bounds if it is broken -- the label
        encoder's embedding launch clamps its index (csrc/misc.hip, embedding_swish_fwd_kernel) and its backward matches
        rows to classes by equality -- and the cross-entropy row of such a label is NaN (csrc/loss_ragged.hip), so the
        label term and the total read NaN instead of training on it silently."""
        model, D, dev = self.model, self.D, self.dev
        pl = self._flags(label, present, paired)
        B = pl.B
        if image.shape[0] != B or label.shape[0] != B:
            raise ValueError('%d flags for %d images and %d labels' % (B, image.shape[0], label.shape[0]))
        tb = pl.to(dev)
        self.last_plan = pl
        for p in model.parameters():
            p.grad = None
        image = image.to(dev, torch.float32).contiguous()
        label = label.to(dev).contiguous()

        # encoders: only on the rows that have the modality
        heads = [None, None]
        n_image_rows, n_label_rows = pl.expert_rows[0].size, pl.expert_rows[1].size
        if n_image_rows:
            x = image
            if n_image_rows != B:
                x = torch.empty((n_image_rows,) + tuple(image.shape[1:]), dtype=torch.float32, device=dev)
                K.block_gather(image, tb.expert_rows[0], x, image[0].numel())
            heads[0] = model.image_encoder.heads(x)
        if n_label_rows:
            heads[1] = model.label_encoder.heads(label if n_label_rows == B else label[tb.expert_rows[1]])

        if noise is not None:
            self.noise = torch.as_tensor(noise, dtype=torch.float32).to(dev).reshape(N_TERMS, B, D).contiguous()
            draw = None
        else:
            self.noise = torch.empty(N_TERMS, B, D, dtype=torch.float32, device=dev)
            draw = (self.seed, self.counter, 0)
        _, _, z, kl = RaggedPoEFn.apply((tb, self.noise, draw, model.POE_VARIANT, D), *heads)
        if draw is not None:
            K.counter_add(self.counter, 1)

        # decoders: each once, on its contiguous slice of the compact rows; the targets are found through row_of
        bce_rows = ce_rows = img_logits = lbl_logits = None
        lo, hi = pl.image_slice
        if hi > lo:
            img_logits = model.image_decoder(z[lo:hi]).reshape(hi - lo, -1)
            bce_rows = BceRowsIndexedFn.apply(img_logits, image.reshape(B, -1), tb.row_of[lo:hi],
                                              self._row_coefs(self.lambda_image, B, hi - lo))
        lo, hi = pl.label_slice
        if hi > lo:
            lbl_logits = model.label_decoder(z[lo:hi])
            ce_rows = CeRowsIndexedFn.apply(lbl_logits, label, tb.row_of[lo:hi],
                                            self._row_coefs(self.lambda_label, B, hi - lo))
        self.last_logits = (None if img_logits is None else img_logits.detach(),
                            None if lbl_logits is None else lbl_logits.detach())
        total, elbo = RaggedTermSumsFn.apply((pl.n_img, pl.n_joint, pl.n_lbl), _coef_tensor([annealing_factor], B, dev),
                                             bce_rows, ce_rows, kl)
        total.backward()
        arena = model.arena
        for p in arena.params:              # what no active term reaches: a zero gradient, so that Adam can step
            if p.grad is None:
                p.grad = arena.grad_view(p)
                p.grad.zero_()
        return elbo
