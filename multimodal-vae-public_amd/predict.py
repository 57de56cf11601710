"""Label prediction from a trained MVAE: given only the image (or any ``given`` set), which label does the model predict,
and how often is it right -- the classification accuracy the MVAE paper reports beside its log-likelihoods.

For one datum b, with the model in ``eval()`` mode and under ``no_grad``:

    (mu_b, logvar_b) = model.infer(the modalities in ``given``)               default: the image alone
    K = 0 :  z_b = mu_b, one decoder row per datum
    K >= 1:  z_kb = mu_b + exp(0.5 logvar_b) * eps_kb,   eps_kb ~ N(0, I),   k = 1 .. K

    categorical head (mnist, fashionmnist: C = 10; multimnist: C = n_characters at each of the 4 positions)
        logp[b, c] = logsumexp_k log_softmax(logits_kb)[c] - log K            (K = 0: log_softmax(logits_b)[c])
        pred[b]    = argmax_c logp[b, c]                                      (the lowest index on a tie)
        nll[b]     = -logp[b, y_b]
    Bernoulli heads (celeba: the 18 columns of one decoder; celeba19: 18 one-logit decoders)
        logp[b, a]  = logsumexp_k -softplus(-l_kba) - log K                   (log p(a = 1))
        logp0[b, a] = logsumexp_k -softplus(+l_kba) - log K                   (log p(a = 0))
        pred[b, a]  = 1 if logp > logp0 else 0
        nll[b, a]   = -(logp if y = 1 else logp0)

the Monte-Carlo posterior predictive ``E_{q(z | given)} p(y | z)`` in the log domain.  MultiMNIST's text decoder runs
greedily per sample, as everywhere else in the project; its four positions are four categorical predictions (decoder row
``(k * B + b) * 4 + l`` belongs to datum-position ``(b, l)`` = the row index modulo ``B * 4``, the identity ../loglike.py
uses), so with K = 0 the prediction is exactly the string a greedy decode of ``mu`` gives.

Everything stays on the device: per chunk of ``Kc`` samples one ``mvae_iw_draw`` launch (its density-ratio rows are not
used), the label decoder on the ``Kc * B`` sample-major rows (celeba19: ``AttrExperts.hidden`` and the grouped N = 1 Linear
of celeba19/loglike.py, whose [G, R] logits are read through their strides) and one ``mvae_predict_fold`` launch (K28,
csrc/predict.hip: one streaming (maximum, sum) state per (datum, class)); then one ``mvae_predict_score`` launch
(arg-max, -logp of the truth, correct flag, confusion counts)."""
import torch

from . import kernels as K
from . import loglike
from .draws import draw_chunks, eval_mode, require_gpu

KINDS = ('mnist', 'fashionmnist', 'celeba', 'celeba19', 'multimnist')
MODES = {'mnist': 'categorical', 'fashionmnist': 'categorical', 'multimnist': 'categorical', 'celeba': 'bernoulli',
         'celeba19': 'bernoulli'}
N_ATTRS = 18
TEXT_LENGTH = 4           # multimnist.model.max_length text positions per datum


def attribute_names():
    """The 18 attribute names of the CelebA models, in column order."""
    from .celeba.datasets import ATTR_IX_TO_KEEP, IX_TO_ATTR_DICT
    return tuple(IX_TO_ATTR_DICT[ATTR_IX_TO_KEEP[i]] for i in range(N_ATTRS))


def _given(kind, value, who):
    """``given`` in canonical order: 'image' and / or 'label'; celeba19: 'image' and attribute names ('attrs' or 'label'
    = all 18)."""
    if value is None:
        return ('image',)
    names = (value,) if isinstance(value, str) else tuple(value)
    if kind == 'celeba19':
        attrs = attribute_names()
        out = []
        for n in names:
            if n in ('attrs', 'label'):
                out.extend(attrs)
            elif n == 'image' or n in attrs:
                out.append(n)
            else:
                raise ValueError("%s: unknown modality %r in `given` (use 'image' and attribute names: %s)"
                                 % (who, n, ', '.join(attrs)))
        order = ('image',) + attrs
    else:
        for n in names:
            if n not in ('image', 'label'):
                raise ValueError("%s: unknown modality %r in `given` (use 'image' and / or 'label')" % (who, n))
        out, order = list(names), ('image', 'label')
    if not out:
        raise ValueError('%s: `given` must name at least one modality' % who)
    return tuple(m for m in order if m in out)


def _label_shape(kind, B):
    return {'celeba': (B, N_ATTRS), 'celeba19': (B, N_ATTRS), 'multimnist': (B, TEXT_LENGTH)}.get(kind, (B,))


def _check(who, model, image, label, given, n_samples, chunk_rows, eps, confusion, need_label):
    """Every refusal, before anything is launched."""
    kind = getattr(model, 'KIND', None)
    if kind not in KINDS:
        raise ValueError('%s: expected one of the %s MVAEs, got %r' % (who, ', '.join(KINDS), type(model).__name__))
    given = _given(kind, given, who)
    if need_label and label is None:
        raise ValueError('%s: no label was passed' % who)
    if 'image' in given and image is None:
        raise ValueError('%s: `image` is given but no image was passed' % who)
    if any(n != 'image' for n in given) and label is None:
        raise ValueError('%s: `%s` is given but no label was passed' % (who, [n for n in given if n != 'image'][0]))
    if image is None and label is None:
        raise ValueError('%s: no data was passed' % who)
    B = (image if image is not None else label).shape[0]
    if B < 1:
        raise ValueError('%s: no data (B = 0)' % who)
    if label is not None and tuple(label.shape) != _label_shape(kind, B):
        raise ValueError('%s: the label of %d %s data must be %s, got %s'
                         % (who, B, kind, _label_shape(kind, B), tuple(label.shape)))
    if int(n_samples) < 0:
        raise ValueError('%s: n_samples must be 0 (predict from the posterior mean) or positive, got %r' % (who, n_samples))
    if int(chunk_rows) < 1:
        raise ValueError('%s: chunk_rows must be at least 1 (got %r)' % (who, chunk_rows))
    if eps is not None and (int(n_samples) < 1 or tuple(eps.shape) != (int(n_samples), B, model.n_latents)):
        raise ValueError('%s: eps must be [n_samples, B, D] = %s with n_samples >= 1, got %s'
                         % (who, (int(n_samples), B, model.n_latents), tuple(eps.shape)))
    if confusion is not None:
        C = N_ATTRS if MODES[kind] == 'bernoulli' else (model.text_decoder.n_characters if kind == 'multimnist' else 10)
        want = (C, 2, 2) if MODES[kind] == 'bernoulli' else (C, C)
        if confusion.dtype != torch.int64 or tuple(confusion.shape) != want or not confusion.is_cuda:
            raise ValueError('%s: confusion must be an int64 %s tensor on the GPU' % (who, want))
    require_gpu(who, model)
    return kind, given, B


def _infer(model, kind, image, label, given):
    """``model.infer`` with exactly the modalities in ``given`` -> contiguous (mu, logvar) [B, D]."""
    if kind == 'celeba19':
        from .celeba19 import loglike as C19
        return C19.infer(model, image, label, given)
    return loglike.infer(model, kind, image, label, given)


class LabelHead(object):
    """The label decoder of ``model`` on sample-major rows: ``logits(zr)`` -> a float32 [rows, C] view for
    ``kernels.predict_fold`` (MultiMNIST: [R * 4, C], one row per text position)."""

    def __init__(self, model, kind, max_rows, device):
        self.model, self.kind = model, kind
        self.per_row = TEXT_LENGTH if kind == 'multimnist' else 1
        self.fed = []
        if kind == 'celeba19':
            from .celeba19.loglike import AttrExperts
            self.experts = AttrExperts(model, 0, N_ATTRS - 1, max_rows, device)
            self.flat = torch.empty(N_ATTRS * max_rows, dtype=torch.float32, device=device)

    def logits(self, zr):
        R = zr.shape[0]
        if self.kind == 'celeba19':
            ex = self.experts
            h = ex.hidden(zr)
            w0, w_gs, b0, b_gs = ex.layers[3]
            out = self.flat[:ex.G * R]
            K.linear_fwd_grouped(h, w0, w_gs, b0, b_gs, out.view(ex.G, R, 1), None)
            return out.view(ex.G, R).t()                       # [R, G] with strides (1, R): read in place
        if self.kind == 'multimnist':
            words = self.model.text_decoder(zr).contiguous()   # [R, 4, n_characters]; no tape under no_grad
            self.fed.append(self.model.text_decoder.last_fed)
            return words.view(R * self.per_row, -1)
        return self.model.label_decoder(zr).contiguous()


def fold_chunks(head, mode, mu, logvar, n_samples, Kc, eps=None, seed=0):
    """draw -> label decoder -> fold over chunks of ``Kc`` samples (the last may be shorter); ``n_samples`` 0: one row
    per datum at z = mu through the same launch.  Returns ``out``: [B * per_row, C] or [B, C, 2]."""
    B, D = mu.shape
    dev = mu.device
    Bd = B * head.per_row
    state = out = None

    def fold(logits, finish_k):
        nonlocal state, out
        if state is None:
            C = logits.shape[1]
            state = K.fresh_predict_state(Bd, C, mode, dev)
            out = torch.empty((Bd, C) if mode == 'categorical' else (Bd, C, 2), dtype=torch.float32, device=dev)
        K.predict_fold(logits, Bd, mode, state, out, finish_k=finish_k)

    if n_samples == 0:
        fold(head.logits(mu), 1)
        return out
    for zc, _, finish_k in draw_chunks(mu, logvar, n_samples, Kc, eps=eps, seed=seed):      # the density ratio is not used
        fold(head.logits(zc.view(-1, D)), finish_k)
    return out


class Strings(object):
    """The predicted MultiMNIST strings of ``pred`` [B, 4]; the indices stay on the device until an item is asked for."""

    def __init__(self, pred):
        self.pred, self._list = pred, None

    def _get(self):
        if self._list is None:
            from .multimnist.utils import tensor_to_string
            host = self.pred.cpu()
            self._list = [tensor_to_string(host[i]) for i in range(host.shape[0])]
        return self._list

    def __len__(self):
        return self.pred.shape[0]

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())

    def __repr__(self):
        return repr(self._get())


def _run(who, model, image, label, given, n_samples, chunk_rows, eps, seed, confusion, score):
    kind, given, B = _check(who, model, image, label, given, n_samples, chunk_rows, eps, confusion, score)
    n_samples = int(n_samples)
    mode = MODES[kind]
    dev = next(model.parameters()).device
    if image is not None and 'image' in given:
        image = image.to(dev).float().contiguous()
    if label is not None:
        label = label.to(dev)
        label = label.float().contiguous() if mode == 'bernoulli' else label.long().contiguous()
    Kc = max(1, int(chunk_rows) // B)
    with eval_mode(model):
        mu, logvar = _infer(model, kind, image, label, given)
        head = LabelHead(model, kind, B * max(1, min(Kc, n_samples)), dev)
        out = fold_chunks(head, mode, mu, logvar, n_samples, Kc, eps=eps, seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        if head.fed:
            model.text_decoder.last_fed = torch.cat(head.fed, dim=1)          # [4, K * B], sample-major like z
        shape = (out.shape[0],) if mode == 'categorical' else tuple(out.shape[:2])
        pred = torch.empty(shape, dtype=torch.int64, device=dev)
        nll = correct = None
        if score:
            nll = torch.empty(shape, dtype=torch.float32, device=dev)
            correct = torch.empty(shape, dtype=torch.uint8, device=dev)
            if confusion is None:
                C = out.shape[1]
                confusion = torch.zeros((C, C) if mode == 'categorical' else (C, 2, 2), dtype=torch.int64, device=dev)
            K.predict_score(out, mode, pred, targets=label.reshape(-1) if mode == 'categorical' else label, nll=nll,
                            correct=correct, confusion=confusion)
        else:
            K.predict_score(out, mode, pred)
    if mode == 'bernoulli':
        res = {'logp': out[..., 0], 'logp0': out[..., 1], 'pred': pred}
    elif kind == 'multimnist':
        res = {'logp': out.view(B, TEXT_LENGTH, -1), 'pred': pred.view(B, TEXT_LENGTH)}
        res['strings'] = Strings(res['pred'])
        if score:
            nll, correct = nll.view(B, TEXT_LENGTH), correct.view(B, TEXT_LENGTH)
            res['position_accuracy'] = correct.float().mean(0)
            res['exact_match'] = (res['pred'] == label).all(1).float().mean()
    else:
        res = {'logp': out, 'pred': pred}
    if score:
        res.update(nll=nll, correct=correct, confusion=confusion)
    return res


def predict(model, image=None, given=None, n_samples=0, chunk_rows=4096, eps=None, seed=0, label=None):
    """The posterior predictive of the label modality (module docstring): a dict of device tensors with ``logp`` ([B, C]
    log-probabilities; MultiMNIST [B, 4, C]; the CelebA models [B, 18] = log p(attribute = 1) and ``logp0`` = log p(0))
    and ``pred`` (int64 [B] / [B, 4] / [B, 18]); MultiMNIST also ``strings``, the predicted digit strings (converted on
    the host when first read).

    ``given`` names what the inference network sees: 'image' (the default) and / or 'label'; celeba19 takes attribute
    names beside the image ('attrs' = all 18) and still predicts all 18.  Values of a given label come from ``label``.
    ``n_samples`` K = 0 predicts from the posterior mean; K >= 1 draws K samples per datum in chunks of ``max(1,
    chunk_rows // B)``.  ``eps`` ([K, B, D], host or device) replays noise; otherwise the noise is the device Philox
    stream of ``seed`` (one launch counter, chunk c at offset c, as ``loglike.chunk_loop``).  The model is put in
    ``eval()`` for the call and every module's mode is restored afterwards."""
    return _run('predict', model, image, label, given, n_samples, chunk_rows, eps, seed, None, False)


def evaluate(model, image=None, label=None, given=None, n_samples=0, chunk_rows=4096, eps=None, seed=0, confusion=None):
    """``predict`` scored against ``label`` (int64 [B]; MultiMNIST int64 [B, 4]; the CelebA models {0, 1} [B, 18]): the
    same dict plus ``nll`` (float32, -logp of the true class), ``correct`` (uint8) -- each shaped like ``pred`` -- and
    ``confusion``, int64 [C, C] indexed (truth, prediction), for the CelebA models [18, 2, 2]: the counts of this batch
    ADDED to the table passed in (a fresh one when None), so that one table can be carried over the batches of a dataset.
    MultiMNIST also gets ``position_accuracy`` [4] and ``exact_match`` (the rate of whole strings predicted right)."""
    return _run('evaluate', model, image, label, given, n_samples, chunk_rows, eps, seed, confusion, True)


# ----------------------------------------------------------------------------- the predict.py drop-ins
def add_flags(parser):
    parser.add_argument('model_path', type=str, help='path to trained model file')
    parser.add_argument('--n-samples', type=int, default=0,
                        help='posterior samples per datum; 0 predicts from the posterior mean [default: 0]')
    parser.add_argument('--batch-size', type=int, default=64, help='data per call [default: 64]')
    parser.add_argument('--cuda', action='store_true', default=False, help='enables CUDA [default: False]')
    parser.add_argument('--synthetic', action='store_true', default=False,
                        help='evaluate on random-pixel images and random labels when no dataset is available')
    parser.add_argument('--n-data', type=int, default=None, help='with --synthetic: number of data [default: batch size]')
    parser.add_argument('--data-file', type=str, default=None, help='.npz with arrays `image` and `label`')
    parser.add_argument('--chunk-rows', type=int, default=4096, help='decoder rows per chunk [default: 4096]')
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--out-dir', type=str, default='.', help='where predict.txt is written [default: .]')


def _sem(vals):
    n = vals.numel()
    return (vals.std(unbiased=True) / n ** 0.5).item() if n > 1 else float('nan')


def report(kind, nll, correct, confusion, label, n_samples, exact=None):
    """The lines ``main`` prints and writes: host tensors ``nll`` / ``correct`` [N] or [N, heads], ``confusion`` and the
    labels of the N data."""
    lines = ['%s: N = %d data, K = %d samples, predicted from the image' % (kind, nll.shape[0], n_samples),
             'accuracy %.6f' % correct.double().mean().item()]
    per_datum = nll.double().reshape(nll.shape[0], -1).sum(1)
    lines.append('nll mean %.6f  standard error %.6f%s' % (per_datum.mean().item(), _sem(per_datum),
                                                           '' if nll.dim() == 1 else '  (per datum: the sum over its %d heads)' % nll.shape[1]))
    if MODES[kind] == 'bernoulli':
        lines.append('per attribute: accuracy, rate of the more frequent class in the data, counts [[truth 0: pred 0, pred 1], '
                     '[truth 1: pred 0, pred 1]]')
        ones = label.double().mean(0)
        for a, name in enumerate(attribute_names()):
            t = confusion[a].tolist()
            lines.append('  %-20s accuracy %.6f  majority %.6f  %s' % (name, correct[:, a].double().mean().item(),
                                                                       max(ones[a].item(), 1.0 - ones[a].item()), t))
        return lines
    if kind == 'multimnist':
        lines.append('per-position accuracy ' + ' '.join('%.6f' % v for v in correct.double().mean(0).tolist()))
        lines.append('exact match %.6f' % exact)
    lines.append('confusion (rows: truth, columns: prediction)')
    width = max(5, len(str(int(confusion.max().item()))) + 1)
    for row in confusion.tolist():
        lines.append(' '.join('%*d' % (width, v) for v in row))
    return lines


def main(kind, load_checkpoint, image_shape, argv=None):
    """``python <kind>/predict.py model_path --cuda [...]``: the accuracy of predicting the label from the image, the mean
    NLL with its standard error and the confusion matrix (the CelebA models: per named attribute the accuracy, the 2 x 2
    table and the rate of the more frequent class; MultiMNIST: per-position accuracy and the exact-match rate), printed
    and written to ``predict.txt`` under --out-dir."""
    import argparse
    import os
    parser = argparse.ArgumentParser()
    add_flags(parser)
    if kind in ('celeba', 'celeba19'):
        parser.set_defaults(batch_size=8)
    args = parser.parse_args(argv)
    args.cuda = args.cuda and torch.cuda.is_available()
    if not args.cuda:
        raise SystemExit('this drop-in predicts with HIP kernels: pass --cuda on a ROCm GPU box')
    model = load_checkpoint(args.model_path, use_cuda=True)
    model.cuda().eval()
    image, label = loglike.load_data('celeba' if kind == 'celeba19' else kind, args, image_shape)
    if image.shape[0] < 1:
        raise SystemExit('no data to evaluate')
    nll, correct, confusion, exact = [], [], None, []
    for i in range(0, image.shape[0], args.batch_size):
        lbl = label[i:i + args.batch_size]
        res = evaluate(model, image[i:i + args.batch_size], lbl, n_samples=args.n_samples, chunk_rows=args.chunk_rows,
                       seed=args.seed + i, confusion=confusion)
        confusion = res['confusion']
        nll.append(res['nll'])
        correct.append(res['correct'])
        if kind == 'multimnist':
            exact.append(res['exact_match'] * lbl.shape[0])
    exact = (torch.stack(exact).sum() / image.shape[0]).item() if exact else None
    lines = report(kind, torch.cat(nll).cpu(), torch.cat(correct).cpu(), confusion.cpu(), label, args.n_samples, exact)
    text = '\n'.join(lines)
    print(text)
    if not os.path.isdir(args.out_dir):
        os.makedirs(args.out_dir)
    with open(os.path.join(args.out_dir, 'predict.txt'), 'w') as fp:
        fp.write(text + '\n')
    return 0
