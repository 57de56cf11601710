"""Importance-weighted log-likelihood of the vision MVAE: the six marginals ``log p(x_m)`` and the joint
``log p(x_1 .. x_6)`` of a datum from ONE set of K draws and ONE pass of the scored decoders -- the quantitative evaluation
of the experiment (the estimator of ../loglike.py, which the reference's README promises as ``loglike.py`` and never
published, for six image modalities instead of an image and a label).

For one datum b, a conditioning set ``given`` and a scored set ``score`` (non-empty subsets of ``model.MODALITIES``), with
the model in ``eval()`` mode and under ``no_grad``:

    (mu_b, logvar_b) = model.get_params(the modalities in ``given``)
    z_kb     = mu_b + exp(0.5 logvar_b) * eps_kb,   eps_kb ~ N(0, I),   k = 1 .. K
    ratio_kb = sum_d (0.5 eps^2 - 0.5 z^2 + 0.5 logvar)_d                      (log p(z) - log q(z | given))
    L_b[m]     = logsumexp_k (ratio_kb + log p(x_m | z_kb)) - log K            for every m in ``score``
    L_b[joint] = logsumexp_k (ratio_kb + sum_{m in score} log p(x_m | z_kb)) - log K

log p(x_m | z) is minus the BCE-with-logits sum over the modality's C x 64 x 64 pixels.  Per chunk of ``Kc`` samples: one
``mvae_iw_draw`` launch, the scored decoders on the ``Kc * B`` sample-major rows, and

    path='fused'   one ``kernels.iw_score_multi`` (K24, csrc/loglike_multi.hip): a score launch over all scored logits and
                   a fold launch that merges the S marginal states and the joint state;
    path='rows'    the same estimator on the kernels that were there before: one single-segment ``bce_multi_fwd`` per
                   scored modality (two launches each) and one ``iw_accumulate`` per state -- 19 launches for S = 6
                   (and a [S, R] -> [R, S] copy of the row sums for the joint).  The fallback and the yardstick.

Measured at B = 8, K = 512, D = 250 (tools/vision_loglike_bench.py, profiles/vision_loglike.txt): the six decoders are 97 - 99%
of a chunk in either path; score and fold take 0.09 - 0.23 ms per chunk fused against 0.24 - 0.27 ms on the existing kernels
(and 0.7 - 2.2 ms in torch).  The whole call is fastest at ``chunk_rows`` 4096 (17.5 ms against 18.3 ms at 1024), which is the
default, and there ``fused`` is not ahead of ``rows`` by more than the spread (17.50 against 17.47 ms per chunk, spread 0.27;
at 1024 rows it is, by 1.1%), so ``rows`` stays the default path.  The logits of the six decoders take
196,608 bytes per row, a chunk of 4096 rows about 0.8 GB, next to the decoders' own activations."""
import os
import sys

if __package__ in (None, ''):      # executed as a script (`python vision/loglike.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.vision'

import torch  # noqa: E402

from .. import kernels as K  # noqa: E402
from ..draws import check_draws, draw_chunks, eval_mode, fresh_state, names, report, require_gpu  # noqa: E402,F401
from .model import MODALITIES, N_CHANNELS  # noqa: E402

PATHS = ('fused', 'rows')
DEFAULT_PATH = 'rows'                # profiles/vision_loglike.txt: `fused` is not faster beyond the spread at 4096 rows
DEFAULT_CHUNK_ROWS = 4096
BYTES_PER_ROW = 4 * 64 * 64 * sum(N_CHANNELS.values())      # 196,608: the six decoders' logits of one row


def _names(value, what, default):
    return names(value, what, MODALITIES, 'vision log_likelihood', default=default)


def _check(model, data, score, given, n_samples, chunk_rows, eps, path):
    """Every refusal, before anything is launched."""
    if getattr(model, 'KIND', None) != 'vision':
        raise ValueError('vision log_likelihood: expected the vision MVAE, got %r' % type(model).__name__)
    for n in data:
        if n not in MODALITIES:
            raise ValueError('vision log_likelihood: unknown modality %r in `data` (the modalities are %s)'
                             % (n, ', '.join(MODALITIES)))
    present = tuple(m for m in MODALITIES if data.get(m) is not None)
    score, given = _names(score, 'score', present), _names(given, 'given', present)
    B = None
    for n in sorted(set(score + given), key=MODALITIES.index):
        x = data.get(n)
        if x is None:
            raise ValueError('vision log_likelihood: `%s` is %s but `data` holds no %s'
                             % (n, ' and '.join(w for w, s in (('scored', score), ('given', given)) if n in s), n))
        if x.dim() != 4 or tuple(x.shape[1:]) != (N_CHANNELS[n], 64, 64):
            raise ValueError('vision log_likelihood: `%s` must be [B, %d, 64, 64], got %s'
                             % (n, N_CHANNELS[n], tuple(x.shape)))
        if B is not None and x.shape[0] != B:
            raise ValueError('vision log_likelihood: `%s` holds %d data, the others %d' % (n, x.shape[0], B))
        B = x.shape[0]
    check_draws('vision log_likelihood', n_samples, chunk_rows, eps, B, model.n_latents)
    if path is None:
        path = DEFAULT_PATH
    if path not in PATHS:
        raise ValueError('vision log_likelihood: path must be one of %s, got %r' % (', '.join(PATHS), path))
    require_gpu('vision log_likelihood', model)
    return score, given, path, B


def score_fused(lw, segs, state, out, finish_k, rows=None):
    """One ``iw_score_multi``: the S marginal states and the joint from the segments ``[(logits, target)]``."""
    K.iw_score_multi(lw, segs, state, out, finish_k=finish_k)


def score_rows(lw, segs, state, out, finish_k, rows):
    """The same fold on the existing kernels: one single-segment ``bce_multi_fwd`` per segment into ``rows`` [S, >= R],
    one ``iw_accumulate`` per state."""
    S, R = len(segs), lw.numel()
    for s, (logits, target) in enumerate(segs):
        K.bce_multi_fwd([(logits, target, None, 1.0)], rows[s, :R])
        K.iw_accumulate(lw, [(rows[s, :R], 1)], state[s], out[s], finish_k=finish_k)
    if S <= 2:
        joint = [(rows[s, :R], 1) for s in range(S)]
    else:
        joint = [(rows[:, :R].t().contiguous(), S)]          # [R, S]: a sample's S row sums side by side
    K.iw_accumulate(lw, joint, state[S], out[S], finish_k=finish_k)


SCORERS = {'fused': score_fused, 'rows': score_rows}


def chunk_loop(model, mu, logvar, targets, score, n_samples, Kc, eps=None, seed=0, path=DEFAULT_PATH):
    """draw -> scored decoders -> score and fold, over chunks of ``Kc`` samples (the last may be shorter).  ``targets``:
    {name: [B, P]} for the scored modalities.  Returns ``out`` [S + 1, B]: the marginals in ``score`` order, then the
    joint."""
    B, D = mu.shape
    dev = mu.device
    S = len(score)
    Kc = min(int(Kc), int(n_samples))
    rows = torch.empty(S, Kc * B, dtype=torch.float32, device=dev) if path == 'rows' else None
    state = fresh_state(S + 1, B, dev)
    out = torch.empty(S + 1, B, dtype=torch.float32, device=dev)
    scorer = SCORERS[path]
    for zc, lwc, finish_k in draw_chunks(mu, logvar, n_samples, Kc, eps=eps, seed=seed):
        R = lwc.numel()
        zr = zc.view(R, D)
        segs = [(getattr(model, name + '_decoder')(zr).reshape(R, -1).contiguous(), targets[name]) for name in score]
        scorer(lwc, segs, state, out, finish_k, rows)
    return out


def log_likelihood(model, data, score=None, given=None, n_samples=1000, chunk_rows=DEFAULT_CHUNK_ROWS, eps=None, seed=0,
                   per_modality=False, path=None):
    """Importance-weighted estimates of ``log p(score)`` with ``q(z | given)`` as the proposal (see the module
    docstring).  ``data``: {modality name: [B, C, 64, 64]}; ``score`` and ``given`` default to every modality in it.

    Returns float32 [B] on the model's device, the joint over ``score``; with ``per_modality`` the dict
    ``{name: [B] for name in score, 'joint': [B]}`` from the same draws.

    ``n_samples`` K draws per datum, in chunks of ``max(1, chunk_rows // B)`` so that a decoder batch has about
    ``chunk_rows`` rows (the logits of all six decoders take 196,608 bytes per row).  ``eps`` ([K, B, D], host or device)
    replaces the device draw (parity runs); otherwise the noise is the device Philox stream of ``seed``.  ``path``:
    'fused' or 'rows' (module docstring).  The model is put in ``eval()`` for the call and every module's mode is
    restored afterwards; nothing in the model is modified."""
    score, given, path, B = _check(model, data, score, given, n_samples, chunk_rows, eps, path)
    n_samples = int(n_samples)
    dev = next(model.parameters()).device
    x = {n: data[n].to(dev).float().contiguous() for n in set(score + given)}
    with eval_mode(model):
        mu, logvar = model.get_params(**{n: x[n] for n in given})
        out = chunk_loop(model, mu.contiguous(), logvar.contiguous(), {n: x[n].reshape(B, -1) for n in score}, score,
                         n_samples, max(1, int(chunk_rows) // B), eps=eps, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, path=path)
    if not per_modality:
        return out[len(score)]
    res = {name: out[i] for i, name in enumerate(score)}
    res['joint'] = out[len(score)]
    return res


# ----------------------------------------------------------------------------- the loglike.py drop-in
def add_flags(parser):
    """The flags of ``loglike.add_flags`` that carry over (model_path, --n-samples, --batch-size, --cuda, --synthetic,
    --n-data, --seed); --score / --given / --chunk-rows with this experiment's defaults; the data flags of
    ``vision/train.py`` in place of --data-file."""
    every = ','.join(MODALITIES)
    parser.add_argument('model_path', type=str, help='path to trained model file')
    parser.add_argument('--n-samples', type=int, default=1000, help='importance samples per datum [default: 1000]')
    parser.add_argument('--batch-size', type=int, default=8, help='data per call [default: 8]')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA [default: False]')
    parser.add_argument('--score', type=str, default=every,
                        help='comma-separated modalities whose likelihood is estimated [default: %s]' % every)
    parser.add_argument('--given', type=str, default=every,
                        help='comma-separated modalities the inference network q(z|.) sees [default: %s]' % every)
    parser.add_argument('--per-modality', action='store_true', default=False,
                        help='also print the marginal of every scored modality (same draws)')
    parser.add_argument('--synthetic', action='store_true', default=False,
                        help='evaluate on random-pixel images when no dataset is available')
    parser.add_argument('--n-data', type=int, default=None, help='with --synthetic: number of data [default: batch size]')
    parser.add_argument('--data-dir', type=str, default='./data',
                        help="the CelebA folders vision/train.py reads; its 'val' partition is evaluated [default: ./data]")
    parser.add_argument('--watermark-file', type=str, default='./watermark.png',
                        help='the image with an alpha channel pasted on for the watermark modality [default: ./watermark.png]')
    from .train import add_edge_flag
    add_edge_flag(parser)
    parser.add_argument('--chunk-rows', type=int, default=DEFAULT_CHUNK_ROWS,
                        help='decoder rows per chunk [default: %d]' % DEFAULT_CHUNK_ROWS)
    parser.add_argument('--seed', type=int, default=0)


def batches(args, device):
    """6-tuples of device tensors: synthetic, or the split ``vision/train.py`` evaluates on ('val', not shuffled)."""
    from .train import SyntheticLoader, check_data
    if args.synthetic:
        n = args.n_data or args.batch_size
        for i, batch in enumerate(SyntheticLoader(args.batch_size, (n + args.batch_size - 1) // args.batch_size,
                                                  args.seed, device)):
            yield tuple(x[:n - i * args.batch_size] for x in batch)
        return
    from .datasets import CelebVisionLoader
    check_data(args)
    for batch in CelebVisionLoader('val', args.data_dir, args.batch_size, False, device,
                                   watermark_path=args.watermark_file, edge=args.edge):
        yield batch


def main(argv=None):
    """``python vision/loglike.py model_path --cuda [...]``: prints the mean of the joint over the data and its standard
    error; with --per-modality the same for every scored modality first."""
    import argparse
    from .train import load_checkpoint
    parser = argparse.ArgumentParser()
    add_flags(parser)
    args = parser.parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in evaluates with HIP kernels: pass --cuda on a ROCm GPU box')
    score = _names([s for s in args.score.split(',') if s], 'score', MODALITIES)
    given = _names([s for s in args.given.split(',') if s], 'given', MODALITIES)
    device = torch.device('cuda', 0)
    model = load_checkpoint(args.model_path, use_cuda=True)
    model.cuda(device).eval()
    vals = {}
    for i, batch in enumerate(batches(args, device)):
        res = log_likelihood(model, dict(zip(MODALITIES, batch)), score=score, given=given, n_samples=args.n_samples,
                             chunk_rows=args.chunk_rows, seed=args.seed + i * args.batch_size, per_modality=True)
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
