"""Float64 restatement of label prediction, written from its definition (not from csrc/predict.hip):

    categorical   logp[b, c] = logsumexp_k log_softmax(logits_kb)[c] - log K
                  pred[b] = argmax_c logp[b, c] (lowest index on a tie), nll[b] = -logp[b, y_b]
    Bernoulli     logp1[b, a] = logsumexp_k -softplus(-l_kba) - log K,  logp0 with +l
                  pred[b, a] = logp1 > logp0, nll[b, a] = -(logp1 if y = 1 else logp0)

``logits`` are sample-major: [K * B, C], row r belongs to datum r % B.  Everything is torch on the CPU in float64
(``dtype=torch.float32`` evaluates the same formulas in fp32: the yardstick of the tolerance in test_predict_gpu.py)."""
import math

import torch
import torch.nn.functional as F

FOLD_SHAPES_CAT = [(1, 1, 2), (3, 5, 10), (64, 2, 10), (65, 3, 13), (200, 2, 64)]      # (Kc, B, C)
FOLD_SHAPE_BERN = (130, 7, 18)
FOLD_SHAPE_BERN_GR = (65, 3, 18)
SCALES = (1.0, 30.0)
MARGIN = 1e-4


def fold_inputs(Kc, B, C, scale, seed=0):
    g = torch.Generator().manual_seed(7000 + 131 * seed + 17 * Kc + 5 * B + C + int(scale))
    return torch.randn(Kc * B, C, generator=g) * scale


def fold_categorical(logits, B, dtype=torch.float64):
    R, C = logits.shape
    v = torch.log_softmax(logits.to(dtype), dim=1).view(R // B, B, C)
    return torch.logsumexp(v, dim=0) - math.log(R // B)


def fold_bernoulli(logits, B, dtype=torch.float64):
    """-> [B, C, 2]: log p(1), log p(0)."""
    R, C = logits.shape
    x = logits.to(dtype).view(R // B, B, C)
    v = torch.stack((-F.softplus(-x), -F.softplus(x)), dim=3)
    return torch.logsumexp(v, dim=0) - math.log(R // B)


def fold(logits, B, mode, dtype=torch.float64):
    return (fold_categorical if mode == 'categorical' else fold_bernoulli)(logits, B, dtype)


def score_categorical(logp, y):
    """-> pred int64 [B], nll float64 [B], correct bool [B], confusion int64 [C, C] (truth, prediction).  A target outside
    0 .. C - 1 is counted nowhere: nll = +inf, correct = False."""
    B, C = logp.shape
    pred = torch.argmax(logp, dim=1)
    valid = (y >= 0) & (y < C)
    safe = torch.where(valid, y, torch.zeros_like(y))
    nll = torch.where(valid, -logp.gather(1, safe.unsqueeze(1)).squeeze(1), torch.full((B,), float('inf'), dtype=logp.dtype))
    correct = valid & (pred == y)
    confusion = torch.bincount(y[valid] * C + pred[valid], minlength=C * C).view(C, C)
    return pred, nll, correct, confusion


def score_bernoulli(logp, y):
    """``logp`` [B, C, 2], ``y`` {0, 1} [B, C] -> pred int64 [B, C], nll, correct, confusion int64 [C, 2, 2]."""
    B, C = y.shape
    l1, l0 = logp[..., 0], logp[..., 1]
    pred = (l1 > l0).long()
    valid = (y == 0) | (y == 1)
    yi = (y == 1).long()
    nll = torch.where(valid, -torch.where(yi == 1, l1, l0), torch.full((B, C), float('inf'), dtype=logp.dtype))
    correct = valid & (pred == yi)
    cell = torch.arange(C).unsqueeze(0) * 4 + yi * 2 + pred
    confusion = torch.bincount(cell[valid], minlength=C * 4).view(C, 2, 2)
    return pred, nll, correct, confusion


def margin(logp, mode):
    """Per datum (categorical) or per (datum, head): how far the prediction is from flipping."""
    if mode == 'categorical':
        if logp.shape[-1] < 2:
            return torch.full(logp.shape[:-1], float('inf'), dtype=logp.dtype)
        top = torch.topk(logp, 2, dim=-1).values
        return top[..., 0] - top[..., 1]
    return (logp[..., 0] - logp[..., 1]).abs()


# ----------------------------------------------------------------------------- inputs of the score tests
def score_case(B, mode, seed=None):
    """Logits of K = 3 samples whose reference prediction has a margin above ``MARGIN`` at every datum, and targets.
    The seeds were chosen on the CPU; ``test_predict_cpu.py`` checks the margins."""
    C = 10 if mode == 'categorical' else 18
    g = torch.Generator().manual_seed(9000 + B + C if seed is None else seed)
    logits = 3 * torch.randn(3 * B, C, generator=g)
    if mode == 'categorical':
        y = torch.randint(0, C, (B,), generator=g)
    else:
        y = torch.randint(0, 2, (B, C), generator=g).float()
    return logits, y, fold(logits, B, mode)
