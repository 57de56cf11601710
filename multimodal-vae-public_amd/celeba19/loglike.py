"""Importance-weighted log-likelihood of the CelebA-19 MVAE (an image and 18 separate attribute experts): the image
marginal ``log p(x)``, the 18 attribute marginals ``log p(a_i)`` and the joint of a datum from ONE set of K draws and ONE
pass of the scored decoders -- the estimator of ../loglike.py and ../vision/loglike.py for the model the paper uses for
"any subset of modalities" (the reference's README promises a ``loglike.py`` per experiment and never published one).

For one datum b, a conditioning set ``given`` and a scored set ``score`` (non-empty subsets of ``MODALITIES``: 'image' and
the 18 attribute names of celeba/datasets.py in column order; 'attrs' is shorthand for all 18), with the model in
``eval()`` mode and under ``no_grad``:

    (mu_b, logvar_b) = model.infer(the modalities in ``given``)
    z_kb     = mu_b + exp(0.5 logvar_b) * eps_kb,   eps_kb ~ N(0, I),   k = 1 .. K
    ratio_kb = sum_d (0.5 eps^2 - 0.5 z^2 + 0.5 logvar)_d                      (log p(z) - log q(z | given))
    L_b[m]     = logsumexp_k (ratio_kb + log p(x_m | z_kb)) - log K            for every m in ``score``
    L_b[joint] = logsumexp_k (ratio_kb + sum_{m in score} log p(x_m | z_kb)) - log K

log p(image | z) is minus the BCE-with-logits sum over the 3 x 64 x 64 pixels, log p(a_i | z) minus the BCE of expert i's
one logit.  Per chunk of ``Kc`` samples: one ``mvae_iw_draw`` launch; the image decoder, if 'image' is scored, and
``bce_rowsum_fwd`` into row 0 of a [19, Kc * B] buffer of loss rows; the attribute experts of the smallest contiguous
range that covers the scored attributes as grouped launches on the parameter arena (``layers.GroupedPlans``), Linear +
Swish for layers 1 - 3 with the activations alone stored; and then

    path='fused'   ``kernels.heads_bce_rows`` (K25, csrc/loglike_heads.hip): the experts' Linear(512, 1) fused with its
                   Bernoulli term into rows 1 + g of the buffer -- the final logits are never written -- and ONE
                   ``kernels.iw_fold_rows`` with ``sel`` = the scored rows: S marginal states and the joint;
    path='rows'    the same estimator on the kernels that were there before: the fourth layer as a grouped N = 1 Linear,
                   ``bce_elem_fwd`` on the [G, R] logits, one ``iw_accumulate`` per state (and a [S, R] -> [R, S] copy of
                   the scored rows for the joint).  The fallback and the yardstick.

The first layer reads the same z for every expert: it is fed with group stride 0 (``kernels.linear_fwd_grouped_shared``;
the grouped forward's loaders form ``x + group * stride`` and only read through it, and stride 0 is what a single group
already passes), so z is not copied per expert.

Measured at B = 8, K = 512, D = 100, all 19 scored and given (tools/celeba19_loglike_bench.py,
profiles/celeba19_loglike.txt): the decoders (the image decoder, its row sums and the experts' layers 1 - 3) are 86 - 92%
of a chunk in either path; head, score and fold take 0.07 - 0.13 ms per chunk fused against 0.29 - 0.32 ms on the existing
kernels (and 0.58 - 0.62 ms in torch).  A whole chunk of 4096 rows takes 4.05 ms fused, 4.18 ms on the existing kernels and
4.92 ms in torch (spread of the repeats 0.02 - 0.05); at 1024 rows 1.10 / 1.18 / 1.58 ms.  ``fused`` is ahead of ``rows`` by
more than the spread at the default ``chunk_rows`` 4096 (3%) and at 1024 (6%; at 2048 it is 1.7% ahead, inside a spread of
0.08 ms), so by the rule that made ``rows`` vision's default ``fused`` is the default path here.  ``heads_bce_rows`` itself
moves its 151 MB in 0.024 ms at 4096 rows: 6.4 TB/s, 80% of the 8 TB/s HBM peak (66% at 2048 rows, 35% at 1024, where launch
latency shows; the activations were written just before and 151 MB fit the 256 MB Infinity Cache, so part of that is cache)."""
import os
import sys

if __package__ in (None, ''):      # executed as a script (`python celeba19/loglike.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.celeba19'

import torch  # noqa: E402

from .. import kernels as K  # noqa: E402
from .. import layers as L  # noqa: E402
from ..celeba.datasets import ATTR_IX_TO_KEEP, IX_TO_ATTR_DICT  # noqa: E402
from ..draws import check_draws, draw_chunks, eval_mode, fresh_state, names, report, require_gpu  # noqa: E402
from .model import N_ATTRS  # noqa: E402

ATTRIBUTES = tuple(IX_TO_ATTR_DICT[ATTR_IX_TO_KEEP[i]] for i in range(N_ATTRS))
MODALITIES = ('image',) + ATTRIBUTES
PATHS = ('fused', 'rows')
DEFAULT_PATH = 'fused'               # profiles/celeba19_loglike.txt: faster than `rows` beyond the spread at 4096 rows
DEFAULT_CHUNK_ROWS = 4096
N_ROWS = 1 + N_ATTRS                 # loss rows per sample: the image's, then one per attribute


def _names(value, what, default):
    return names(value, what, MODALITIES, 'celeba19 log_likelihood', default=default, aliases={'attrs': ATTRIBUTES},
                 hint="the modalities are %s; 'attrs' names the 18 attributes" % ', '.join(MODALITIES))


def _check(model, image, attrs, score, given, n_samples, chunk_rows, eps, path):
    """Every refusal, before anything is launched."""
    if getattr(model, 'KIND', None) != 'celeba19':
        raise ValueError('celeba19 log_likelihood: expected the celeba19 MVAE, got %r' % type(model).__name__)
    present = (('image',) if image is not None else ()) + (ATTRIBUTES if attrs is not None else ())
    score, given = _names(score, 'score', present), _names(given, 'given', present)
    for n in sorted(set(score + given), key=MODALITIES.index):
        if (image if n == 'image' else attrs) is None:
            raise ValueError('celeba19 log_likelihood: `%s` is %s but no %s was passed'
                             % (n, ' and '.join(w for w, s in (('scored', score), ('given', given)) if n in s),
                                'image' if n == 'image' else 'attrs'))
    used_image = 'image' in score + given
    used_attrs = any(n != 'image' for n in score + given)
    if used_image and (image.dim() != 4 or tuple(image.shape[1:]) != (3, 64, 64)):
        raise ValueError('celeba19 log_likelihood: `image` must be [B, 3, 64, 64], got %s' % (tuple(image.shape),))
    if used_attrs and (attrs.dim() != 2 or attrs.shape[1] != N_ATTRS):
        raise ValueError('celeba19 log_likelihood: `attrs` must be [B, %d], got %s' % (N_ATTRS, tuple(attrs.shape)))
    if used_image and used_attrs and image.shape[0] != attrs.shape[0]:
        raise ValueError('celeba19 log_likelihood: `image` holds %d data, `attrs` %d' % (image.shape[0], attrs.shape[0]))
    B = (image if used_image else attrs).shape[0]
    if B < 1:
        raise ValueError('celeba19 log_likelihood: no data (B = 0)')
    check_draws('celeba19 log_likelihood', n_samples, chunk_rows, eps, B, model.n_latents)
    if path is None:
        path = DEFAULT_PATH
    if path not in PATHS:
        raise ValueError('celeba19 log_likelihood: path must be one of %s, got %r' % (', '.join(PATHS), path))
    require_gpu('celeba19 log_likelihood', model)
    return score, given, path, B


class AttrExperts(object):
    """The attribute decoders ``a0 .. a1`` (the smallest contiguous range that covers the scored attributes) as grouped
    launches on the parameter arena, with the activation buffers of a chunk of ``rows`` rows."""

    def __init__(self, model, a0, a1, rows, device):
        self.a0, self.G = a0, a1 - a0 + 1
        self.gp = L.GroupedPlans([model.attr_decoders[i].plan() for i in range(a0, a1 + 1)])
        plan = self.gp.plans[0]
        if [(op.kind, bool(op.act)) for op in plan] != [('lin', True)] * 3 + [('lin', False)]:
            raise RuntimeError('celeba19 log_likelihood: the attribute decoders are not Linear + Swish x 3, Linear')
        self.layers = [self.gp.layer(j) for j in range(4)]
        width = self.layers[0][0].shape[0]
        if self.layers[3][0].shape[0] != 1 or any(self.layers[j][2] is None for j in range(4)):
            raise RuntimeError('celeba19 log_likelihood: the attribute decoders must end in a Linear(., 1) with a bias')
        self.buf = [torch.empty(self.G * rows * width, dtype=torch.float32, device=device) for _ in range(2)]
        self.width = width

    def hidden(self, zr):
        """Layers 1 - 3 on zr [R, D] -> the third layer's post-Swish activations [G, R, width]."""
        R = zr.shape[0]
        a, b = (t[:self.G * R * self.width].view(self.G, R, self.width) for t in self.buf)
        w0, w_gs, b0, b_gs = self.layers[0]
        K.linear_fwd_grouped_shared(zr, self.G, w0, w_gs, b0, b_gs, None, a)      # every expert reads the same z
        for j in (1, 2):
            w0, w_gs, b0, b_gs = self.layers[j]
            K.linear_fwd_grouped(a, w0, w_gs, b0, b_gs, None, b)
            a, b = b, a
        return a

    def rec_fused(self, h, target, rec):
        """rec [G, R] = the Bernoulli terms of the experts' logits on ``h``; ``target`` [B, G]."""
        w0, w_gs, b0, b_gs = self.layers[3]
        K.heads_bce_rows(h, w0.reshape(-1), w_gs, b0, b_gs, target, rec)

    def rec_rows(self, h, target_rows, rec, logits):
        """The same on the existing kernels: the grouped N = 1 Linear into ``logits`` [G, R, 1], then a BCE per element
        against ``target_rows`` [G, R] into ``rec`` [G, R] (both contiguous)."""
        w0, w_gs, b0, b_gs = self.layers[3]
        K.linear_fwd_grouped(h, w0, w_gs, b0, b_gs, logits, None)
        K.bce_elem_fwd(logits.view(-1), target_rows.reshape(-1), rec.view(-1))


def fold_fused(lw, rec, sel, sel_dev, state, out, finish_k):
    """One ``iw_fold_rows``: the S marginal states and the joint from the scored rows of ``rec``."""
    K.iw_fold_rows(lw, rec, sel, state, out, finish_k=finish_k)


def fold_rows(lw, rec, sel, sel_dev, state, out, finish_k):
    """The same fold on the existing kernel: one ``iw_accumulate`` per state."""
    S = len(sel)
    for j, s in enumerate(sel):
        K.iw_accumulate(lw, [(rec[s], 1)], state[j], out[j], finish_k=finish_k)
    if S <= 2:
        joint = [(rec[s], 1) for s in sel]
    else:
        joint = [(rec.index_select(0, sel_dev).t().contiguous(), S)]          # [R, S]: a sample's S terms side by side
    K.iw_accumulate(lw, joint, state[S], out[S], finish_k=finish_k)


FOLDS = {'fused': fold_fused, 'rows': fold_rows}


def chunk_loop(model, mu, logvar, image, attrs, score, n_samples, Kc, eps=None, seed=0, path=DEFAULT_PATH):
    """draw -> scored decoders -> loss rows -> fold, over chunks of ``Kc`` samples (the last may be shorter).  ``image``
    [B, 12288] and ``attrs`` [B, 18] (each may be None when not scored).  Returns ``out`` [S + 1, B]: the marginals in
    ``score`` order, then the joint."""
    B, D = mu.shape
    dev = mu.device
    S = len(score)
    Kc = min(int(Kc), int(n_samples))
    sel = [MODALITIES.index(n) for n in score]                  # rows of the loss-row buffer: 0 image, 1 + i attribute i
    sel_dev = torch.tensor(sel, dtype=torch.int64, device=dev)
    scored_attrs = [s - 1 for s in sel if s > 0]
    rec_flat = torch.empty(N_ROWS * Kc * B, dtype=torch.float32, device=dev)
    experts = targets = logits_flat = None
    if scored_attrs:
        a0, a1 = scored_attrs[0], scored_attrs[-1]
        experts = AttrExperts(model, a0, a1, Kc * B, dev)
        cols = attrs[:, a0:a1 + 1]                              # [B, G]: a column range, passed as it is
        if path == 'rows':
            logits_flat = torch.empty(experts.G * Kc * B, dtype=torch.float32, device=dev)
            targets = {}                                        # samples in the chunk -> [G, n * B]
    state = fresh_state(S + 1, B, dev)
    out = torch.empty(S + 1, B, dtype=torch.float32, device=dev)
    fold = FOLDS[path]
    for zc, lwc, finish_k in draw_chunks(mu, logvar, n_samples, Kc, eps=eps, seed=seed):
        n = zc.shape[0]
        R = n * B
        zr = zc.view(R, D)
        rec = rec_flat[:N_ROWS * R].view(N_ROWS, R)             # dense for this chunk's R: every row range is contiguous
        if 'image' in score:
            logits = model.image_decoder(zr).reshape(R, -1).contiguous()
            K.bce_rowsum_fwd(logits, image, rec[0], target_rows=B)
        if experts is not None:
            h = experts.hidden(zr)
            block = rec[1 + experts.a0:1 + experts.a0 + experts.G]
            if path == 'fused':
                experts.rec_fused(h, cols, block)
            else:
                if n not in targets:
                    targets[n] = cols.t().unsqueeze(1).expand(experts.G, n, B).reshape(experts.G, R).contiguous()
                experts.rec_rows(h, targets[n], block, logits_flat[:experts.G * R].view(experts.G, R, 1))
        fold(lwc, rec, sel, sel_dev, state, out, finish_k)
    return out


def infer(model, image, attrs, given):
    """``model.infer`` with exactly the modalities in ``given`` -> contiguous (mu, logvar) [B, D]."""
    img = image if 'image' in given else None
    lst = [attrs[:, i].contiguous() if n in given else None for i, n in enumerate(ATTRIBUTES)]
    mu, logvar = model.infer(image=img, attrs=lst if any(a is not None for a in lst) else None)
    return mu.contiguous(), logvar.contiguous()


def log_likelihood(model, image=None, attrs=None, score=None, given=None, n_samples=1000, chunk_rows=DEFAULT_CHUNK_ROWS,
                   eps=None, seed=0, per_modality=False, path=None):
    """Importance-weighted estimates of ``log p(score)`` with ``q(z | given)`` as the proposal (see the module
    docstring).  ``image`` [B, 3, 64, 64], ``attrs`` the [B, 18] {0, 1} matrix; ``score`` and ``given`` (names of
    ``MODALITIES``, 'attrs' = all 18 attributes) default to every modality whose data was passed.

    Returns float32 [B] on the model's device, the joint over ``score``; with ``per_modality`` the dict
    ``{name: [B] for name in score, 'joint': [B]}`` from the same draws.

    ``n_samples`` K draws per datum, in chunks of ``max(1, chunk_rows // B)`` so that a decoder batch has about
    ``chunk_rows`` rows.  ``eps`` ([K, B, D], host or device) replaces the device draw (parity runs); otherwise the noise
    is the device Philox stream of ``seed``.  ``path``: 'fused' or 'rows' (module docstring).  The model is put in
    ``eval()`` for the call and every module's mode is restored afterwards; nothing in the model is modified."""
    score, given, path, B = _check(model, image, attrs, score, given, n_samples, chunk_rows, eps, path)
    n_samples = int(n_samples)
    dev = next(model.parameters()).device
    if image is not None and 'image' in score + given:
        image = image.to(dev).float().contiguous()
    if attrs is not None and any(n != 'image' for n in score + given):
        attrs = attrs.to(dev).float().contiguous()
    with eval_mode(model):
        mu, logvar = infer(model, image, attrs, given)
        out = chunk_loop(model, mu, logvar, image.reshape(B, -1) if 'image' in score else None, attrs, score, n_samples,
                         max(1, int(chunk_rows) // B), eps=eps, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, path=path)
    if not per_modality:
        return out[len(score)]
    res = {name: out[i] for i, name in enumerate(score)}
    res['joint'] = out[len(score)]
    return res


# ----------------------------------------------------------------------------- the loglike.py drop-in
def main(argv=None):
    """``python celeba19/loglike.py model_path --cuda [...]``: prints the mean of the joint over the data and its standard
    error; with --per-modality the same for every scored modality first.  The data format is CelebA's (an ``image`` and
    a ``label`` = the [N, 18] attribute matrix)."""
    import argparse
    from ..loglike import add_flags, load_data
    from .train import load_checkpoint
    parser = argparse.ArgumentParser()
    add_flags(parser)
    parser.set_defaults(score='image,attrs', given='image,attrs', batch_size=8)
    parser.add_argument('--per-modality', action='store_true', default=False,
                        help='also print the marginal of every scored modality (same draws)')
    args = parser.parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in evaluates with HIP kernels: pass --cuda on a ROCm GPU box')
    score = _names([s for s in args.score.split(',') if s], 'score', MODALITIES)
    given = _names([s for s in args.given.split(',') if s], 'given', MODALITIES)
    model = load_checkpoint(args.model_path, use_cuda=True)
    model.cuda().eval()
    image, label = load_data('celeba', args, (3, 64, 64))
    vals = {}
    for i in range(0, image.shape[0], args.batch_size):
        res = log_likelihood(model, image[i:i + args.batch_size], label[i:i + args.batch_size], score=score, given=given,
                             n_samples=args.n_samples, chunk_rows=args.chunk_rows, seed=args.seed + i, per_modality=True)
        for name, v in res.items():
            vals.setdefault(name, []).append(v.double().cpu())
    if not vals:
        raise SystemExit('no data to evaluate')
    if args.per_modality:
        for name in score:
            report(name, torch.cat(vals[name]), given, args.n_samples)
    report(','.join(score), torch.cat(vals['joint']), given, args.n_samples)
    return 0


if __name__ == "__main__":
    sys.exit(main())
