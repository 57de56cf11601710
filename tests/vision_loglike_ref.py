"""Test helper (not a test): the vision importance-weighted log-likelihood (multimodal-vae-public_amd/vision/loglike.py,
csrc/loglike_multi.hip) restated in float64 on plain torch, built on tests/loglike_ref.py.

    logw[s, k, b] = ratio[k, b] + log p(x_s | z[k, b])                  s = 0 .. S-1   (the marginals)
    logw[S, k, b] = ratio[k, b] + sum_s log p(x_s | z[k, b])                           (the joint)
    L[j, b]       = logsumexp_k logw[j, k, b] - log K

``fold`` is the kernel-level restatement (given density-ratio rows and logits), ``estimates`` starts from (mu, logvar,
eps), ``vision_case`` runs the CPU model of tests/vision_ref.py in eval mode for the end-to-end cases."""
import torch

import loglike_ref as LR

# (score, given) of the end-to-end test; None = all six
E2E_CASES = ((None, None), (('image',), None), (('gray', 'edge'), ('image',)), (('mask',), ('obscured', 'watermark')))
E2E_B, E2E_K, E2E_D = 3, 5, 8


def fold(ratio, segs):
    """ratio [K, B], segs [(logits [K * B, P] or [K, B, ...], target [B, ...])] -> (logw [S + 1, K, B], L [S + 1, B])."""
    ratio = LR._d(ratio)
    K, B = ratio.shape
    logp = [LR.log_p_bernoulli(LR._d(x).reshape(K, B, -1), t) for x, t in segs]
    logw = [ratio + lp for lp in logp]
    joint = ratio
    for lp in logp:
        joint = joint + lp
    logw = torch.stack(logw + [joint])
    return logw, torch.stack([LR.estimate(w) for w in logw])


def estimates(mu, logvar, eps, segs):
    """(mu, logvar) [B, D], eps [K, B, D], segs as in ``fold`` -> (z, logw, L)."""
    z, ratio = LR.draw(mu, logvar, eps)
    logw, L = fold(ratio, segs)
    return z, logw, L


def vision_pair(seed=91):
    """(CPU restatement model in eval mode, its state_dict source for the HIP model, data dict, eps)."""
    import vision_ref as R
    from oracle import models as OM
    o = OM.fill_parameters(R.MVAE(E2E_D), seed)
    LR.randomise_running_stats([o], seed + 1)
    o.eval()
    batch = R.synthetic_batch(E2E_B, seed + 2)
    eps = torch.randn(E2E_K, E2E_B, E2E_D, generator=torch.Generator().manual_seed(seed + 3))
    return o, dict(zip(R.MODALITIES, batch)), eps


def vision_case(o, data, eps, score, given):
    """The restated {name: L [B], 'joint': L [B]} of one (score, given) case on the CPU model ``o``."""
    import vision_ref as R
    score = R.MODALITIES if score is None else tuple(m for m in R.MODALITIES if m in score)
    given = R.MODALITIES if given is None else given
    K, B, D = eps.shape
    with torch.no_grad():
        mu, lv = o.get_params([data[m] if m in given else None for m in R.MODALITIES])
        z, _ = LR.draw(mu, lv, eps)
        zr = z.float().reshape(K * B, D)
        segs = [(getattr(o, m + '_decoder')(zr).reshape(K, B, -1), data[m]) for m in score]
    _, _, L = estimates(mu, lv, eps, segs)
    res = {m: L[i] for i, m in enumerate(score)}
    res['joint'] = L[len(score)]
    return res
