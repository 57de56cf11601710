"""What the evaluation paths built on ``mvae_iw_draw`` share (loglike.py, vision/loglike.py, celeba19/loglike.py,
celeba19/sample.py, predict.py): the eval-mode guard, the chunk schedule of the K draws and the loop that launches them,
the streaming state, the refusals with a common wording, and the line the loglike drop-ins print."""
import contextlib

import torch

from . import kernels as K


@contextlib.contextmanager
def eval_mode(model):
    """``model.eval()`` and ``no_grad`` for the body; every module's ``training`` flag is restored afterwards, also when
    the body raises."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m, mode in modes:
            m.training = mode


def fresh_state(n_states, B, device):
    """[n_states, B, 2]: (running maximum, running sum) = (-inf, 0)."""
    state = torch.zeros(n_states, B, 2, dtype=torch.float32, device=device)
    state[:, :, 0] = float('-inf')
    return state


def chunks(n_samples, Kc):
    """The K draws in chunks of ``Kc`` (the last may be shorter): ``(c, k0, n, finish_k)`` = chunk index, first sample,
    samples in the chunk, and K on the last chunk (0 before it), which is when a fold writes its result."""
    Kc = min(int(Kc), int(n_samples))
    for c, k0 in enumerate(range(0, n_samples, Kc)):
        n = min(Kc, n_samples - k0)
        yield c, k0, n, n_samples if k0 + n == n_samples else 0


def draw_chunks(mu, logvar, n_samples, Kc, eps=None, seed=0):
    """One ``kernels.iw_draw`` per chunk of ``chunks(n_samples, Kc)``; yields ``(z [n, B, D], lw [n, B], finish_k)``,
    views of two buffers that the next chunk overwrites.  ``eps`` [K, B, D] is replayed; otherwise the noise is the
    device Philox stream of ``seed``: one zeroed launch counter per call, chunk c at offset c."""
    B, D = mu.shape
    dev = mu.device
    Kc = min(int(Kc), int(n_samples))
    z = torch.empty(Kc, B, D, dtype=torch.float32, device=dev)
    lw = torch.empty(Kc, B, dtype=torch.float32, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev) if eps is None else None
    for c, k0, n, finish_k in chunks(n_samples, Kc):
        zc, lwc = z[:n], lw[:n]
        if eps is not None:
            K.iw_draw(mu, logvar, zc, lwc, eps=eps[k0:k0 + n].to(dev).float().contiguous())
        else:
            K.iw_draw(mu, logvar, zc, lwc, seed=seed, counter_dev=counter, counter_offset=c)
        yield zc, lwc, finish_k


def names(value, what, modalities, who, default=None, aliases=None, hint=None):
    """``score`` / ``given`` in the order of ``modalities``: a name or a sequence of names, ``default`` when None;
    ``aliases`` maps a shorthand to the names it stands for.  ``hint`` ends the unknown-modality message."""
    if value is None:
        value = default
    out = []
    for n in (value,) if isinstance(value, str) else tuple(value):
        if aliases and n in aliases:
            out.extend(aliases[n])
        elif n in modalities:
            out.append(n)
        else:
            raise ValueError('%s: unknown modality %r in `%s` (%s)'
                             % (who, n, what, hint or 'the modalities are %s' % ', '.join(modalities)))
    if not out:
        raise ValueError('%s: `%s` must name at least one modality' % (who, what))
    return tuple(m for m in modalities if m in out)


def check_draws(who, n_samples, chunk_rows, eps, B, D):
    if int(n_samples) < 1:
        raise ValueError('%s: n_samples must be at least 1 (got %r)' % (who, n_samples))
    if int(chunk_rows) < 1:
        raise ValueError('%s: chunk_rows must be at least 1 (got %r)' % (who, chunk_rows))
    if eps is not None and tuple(eps.shape) != (int(n_samples), B, D):
        raise ValueError('%s: eps must be [n_samples, B, D] = %s, got %s' % (who, (int(n_samples), B, D), tuple(eps.shape)))


def require_gpu(who, model):
    if not next(model.parameters()).is_cuda:
        raise RuntimeError('%s: the model must live on the GPU (model.cuda()); the HIP path has no CPU fallback' % who)


def report(name, vals, given, n_samples):
    n = vals.numel()
    sem = (vals.std(unbiased=True) / n ** 0.5).item() if n > 1 else float('nan')
    print('log p(%s | q(z|%s)): mean %.4f  standard error %.4f  (N = %d data, K = %d samples)'
          % (name, ','.join(given), vals.mean().item(), sem, n, n_samples))
