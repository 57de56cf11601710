"""Importance-weighted marginal log-likelihood -- the ``loglike.py`` the reference's README lists in every experiment
folder ("to compute the marginal log likelihood log p(x) using q(z|x,y) as the inference network") and never
published.  It is the number the MVAE paper's tables report.

For one datum b, a conditioning set ``given`` and a scored set ``score`` (non-empty subsets of {'image', 'label'};
'label' is the experiment's second modality: the class, the 18 attributes or the digit string), with the model in
``eval()`` mode and under ``no_grad``:

    (mu_b, logvar_b) = model.infer(the modalities in ``given``)
    z_kb   = mu_b + exp(0.5 logvar_b) * eps_kb,   eps_kb ~ N(0, I),   k = 1 .. K
    logw_kb = sum_{m in score} log p(x_m | z_kb) + sum_d (0.5 eps^2 - 0.5 z^2 + 0.5 logvar)_d
    L_b    = logsumexp_k logw_kb - log K

log p(image | z) is minus the BCE-with-logits row sum over the pixels (``elbo_loss``'s image term without its lambda);
the class term minus the ``mvae_ce_fwd`` row; CelebA's attribute term minus the BCE row sum over the 18 columns;
MultiMNIST's text term minus the four positions' cross-entropy rows.  The README's quantity is ``score=('image',)``,
``given=('image', 'label')``; the joint is ``score=('image', 'label')``; conditionals follow by subtraction.

Everything stays on the device: per chunk of ``Kc`` samples one ``mvae_iw_draw`` launch (draw + density ratio), the
scored decoders on the ``Kc * B`` sample-major rows, the existing loss-row kernels, and one ``mvae_iw_accumulate``
launch (streaming log-mean-exp).  ``celeba19`` (19 modalities) is refused here: its estimator is
``celeba19/loglike.py`` (19 marginals and the joint from one pass)."""
import torch

from . import kernels as K
from .draws import check_draws, draw_chunks, eval_mode, fresh_state, names, report, require_gpu

MODALITIES = ('image', 'label')
KINDS = ('mnist', 'fashionmnist', 'celeba', 'multimnist')


def _names(value, what):
    return names(value, what, MODALITIES, 'log_likelihood', hint="use 'image' and / or 'label'")


def _check(model, image, label, score, given, n_samples, chunk_rows, eps):
    """Every refusal, before anything is launched."""
    kind = getattr(model, 'KIND', None)
    if kind == 'celeba19':
        raise NotImplementedError('log_likelihood: celeba19 (19 modalities) is out of scope; supported: %s' % ', '.join(KINDS))
    if kind not in KINDS:
        raise ValueError('log_likelihood: expected one of the %s MVAEs, got %r' % (', '.join(KINDS), type(model).__name__))
    score, given = _names(score, 'score'), _names(given, 'given')
    data = {'image': image, 'label': label}
    for n in sorted(set(score + given)):
        if data[n] is None:
            raise ValueError('log_likelihood: `%s` is %s but no %s was passed'
                             % (n, ' and '.join(w for w, s in (('scored', score), ('given', given)) if n in s), n))
    B = (image if image is not None else label).shape[0]
    check_draws('log_likelihood', n_samples, chunk_rows, eps, B, model.n_latents)
    require_gpu('log_likelihood', model)
    return kind, score, given, B


def _prepare(model, kind, image, label):
    """The data on the model's device in the layout the loss-row kernels read."""
    dev = next(model.parameters()).device
    if image is not None:
        image = image.to(dev).float().contiguous()
    if label is not None:
        label = label.to(dev)
        label = label.float().contiguous() if kind == 'celeba' else label.long().contiguous()
    return image, label


def infer(model, kind, image, label, given):
    """``model.infer`` with exactly the modalities in ``given`` -> contiguous (mu, logvar) [B, D]."""
    img = image if 'image' in given else None
    lbl = label if 'label' in given else None
    mu, logvar = model.infer(image=img, attrs=lbl) if kind == 'celeba' else model.infer(image=img, text=lbl)
    return mu.contiguous(), logvar.contiguous()


def score_rows(model, kind, z, image, label, score, bufs=None):
    """The scored decoders on the sample-major rows ``z`` [Kc, B, D] and their loss rows (-log p):
    a list of ``(rows, rows_per_sample)`` as ``kernels.iw_accumulate`` takes them.  Row r of a decoder's batch belongs to
    datum r % B, which is how the loss-row kernels address their targets."""
    Kc, B, D = z.shape
    R = Kc * B
    zr = z.view(R, D)
    terms = []

    def rows(name, n):
        if bufs is None:
            return torch.empty(n, dtype=torch.float32, device=z.device)
        return bufs[name][:n]
    if 'image' in score:
        logits = model.image_decoder(zr).reshape(R, -1).contiguous()
        out = rows('image', R)
        K.bce_rowsum_fwd(logits, image.reshape(B, -1), out, target_rows=B)
        terms.append((out, 1))
    if 'label' in score:
        if kind == 'multimnist':
            words = model.text_decoder(zr).contiguous()                      # [R, 4, n_characters]; no tape under no_grad
            L = words.shape[1]
            out = rows('label', R * L)
            K.ce_fwd(words.view(R * L, -1), label.reshape(-1), out, label_rows=B * L)
            terms.append((out, L))
        else:
            logits = model.label_decoder(zr).contiguous()
            out = rows('label', R)
            if kind == 'celeba':
                K.bce_rowsum_fwd(logits, label, out, target_rows=B)
            else:
                K.ce_fwd(logits, label, out, label_rows=B)
            terms.append((out, 1))
    return terms


def chunk_loop(model, kind, mu, logvar, image, label, score, n_samples, Kc, eps=None, seed=0):
    """draw -> decoders -> loss rows -> accumulate over chunks of ``Kc`` samples (the last may be shorter)."""
    B = mu.shape[0]
    dev = mu.device
    Kc = min(int(Kc), int(n_samples))
    L = 4 if kind == 'multimnist' else 1          # multimnist.model.max_length text positions per sample
    bufs = {'image': torch.empty(Kc * B, dtype=torch.float32, device=dev),
            'label': torch.empty(Kc * B * L, dtype=torch.float32, device=dev)}
    state = fresh_state(1, B, dev)[0]
    out = torch.empty(B, dtype=torch.float32, device=dev)
    fed = []
    for zc, lwc, finish_k in draw_chunks(mu, logvar, n_samples, Kc, eps=eps, seed=seed):
        terms = score_rows(model, kind, zc, image, label, score, bufs)
        if kind == 'multimnist' and 'label' in score:
            fed.append(model.text_decoder.last_fed)
        K.iw_accumulate(lwc, terms, state, out, finish_k=finish_k)
    if fed:
        model.text_decoder.last_fed = torch.cat(fed, dim=1)      # [4, K * B], sample-major like z
    return out


def log_likelihood(model, image=None, label=None, score=('image',), given=('image', 'label'), n_samples=1000,
                   chunk_rows=4096, eps=None, seed=0):
    """Importance-weighted estimate of ``log p(score | ...)`` with ``q(z | given)`` as the proposal: float32 [B] on the
    model's device (see the module docstring for the estimator).

    ``n_samples`` K importance samples per datum, drawn in chunks of ``max(1, chunk_rows // B)`` so that a decoder batch has
    about ``chunk_rows`` rows.  ``eps`` ([K, B, D], host or device) replaces the device draw (parity runs); otherwise
    the noise is the device Philox stream of ``seed``.  The model is put in ``eval()`` for the call (BatchNorm running
    statistics, no Dropout) and every module's mode is restored afterwards; nothing in the model is modified.  After a
    MultiMNIST call that scores the text, ``model.text_decoder.last_fed`` holds the fed-back characters of all
    ``K * B`` rows ([4, K * B], sample-major)."""
    kind, score, given, B = _check(model, image, label, score, given, n_samples, chunk_rows, eps)
    image, label = _prepare(model, kind, image, label)
    with eval_mode(model):
        mu, logvar = infer(model, kind, image, label, given)
        return chunk_loop(model, kind, mu, logvar, image, label, score, int(n_samples), max(1, int(chunk_rows) // B),
                          eps=eps, seed=int(seed) & 0xFFFFFFFFFFFFFFFF)


# ----------------------------------------------------------------------------- the loglike.py drop-ins
def add_flags(parser, n_latents_note=''):
    parser.add_argument('model_path', type=str, help='path to trained model file')
    parser.add_argument('--n-samples', type=int, default=1000,
                        help='importance samples per datum [default: 1000]')
    parser.add_argument('--batch-size', type=int, default=64, help='data per call [default: 64]')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA [default: False]')
    parser.add_argument('--score', type=str, default='image',
                        help="modalities whose likelihood is estimated: image, label or image,label [default: image]")
    parser.add_argument('--given', type=str, default='image,label',
                        help='modalities the inference network q(z|.) sees [default: image,label]')
    parser.add_argument('--synthetic', action='store_true', default=False,
                        help='evaluate on random-pixel images and random labels when no dataset is available')
    parser.add_argument('--n-data', type=int, default=None, help='with --synthetic: number of data [default: batch size]')
    parser.add_argument('--data-file', type=str, default=None, help='.npz with arrays `image` and `label`')
    parser.add_argument('--chunk-rows', type=int, default=4096, help='decoder rows per chunk [default: 4096]')
    parser.add_argument('--seed', type=int, default=0)


def synthetic_data(kind, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind in ('mnist', 'fashionmnist'):
        return torch.rand(n, 1, 28, 28, generator=g), torch.randint(0, 10, (n,), generator=g)
    if kind == 'celeba':
        return torch.rand(n, 3, 64, 64, generator=g), torch.randint(0, 2, (n, 18), generator=g).float()
    digits = torch.randint(0, 10, (n, 4), generator=g)
    length = torch.randint(0, 5, (n,), generator=g)
    return (torch.rand(n, 1, 50, 50, generator=g),
            torch.where(torch.arange(4).unsqueeze(0) < length.unsqueeze(1), digits, torch.full_like(digits, 11)))


def load_data(kind, args, image_shape):
    import numpy as np
    if args.data_file:
        with np.load(args.data_file, allow_pickle=False) as f:
            image, label = torch.from_numpy(f['image']).float(), torch.from_numpy(f['label'])
        return image.reshape((-1,) + tuple(image_shape)), label
    if args.synthetic:
        return synthetic_data(kind, args.n_data or args.batch_size, args.seed)
    raise SystemExit('no dataset on this box: pass --data-file FILE.npz (arrays `image`, `label`) or --synthetic')


def main(kind, load_checkpoint, image_shape):
    """``python <kind>/loglike.py model_path --cuda [...]``: prints the mean of L over the data and its standard error."""
    import argparse
    parser = argparse.ArgumentParser()
    add_flags(parser)
    args = parser.parse_args()
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in evaluates with HIP kernels: pass --cuda on a ROCm GPU box')
    score = tuple(s for s in args.score.split(',') if s)
    given = tuple(s for s in args.given.split(',') if s)
    model = load_checkpoint(args.model_path, use_cuda=True)
    model.cuda().eval()
    image, label = load_data(kind, args, image_shape)
    vals = []
    for i in range(0, image.shape[0], args.batch_size):
        vals.append(log_likelihood(model, image[i:i + args.batch_size], label[i:i + args.batch_size], score=score,
                                   given=given, n_samples=args.n_samples, chunk_rows=args.chunk_rows,
                                   seed=args.seed + i).double().cpu())
    report(','.join(score), torch.cat(vals), given, args.n_samples)
    return 0
