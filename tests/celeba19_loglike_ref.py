"""Test helper (not a test): the CelebA-19 importance-weighted log-likelihood (multimodal-vae-public_amd/celeba19/loglike.py,
csrc/loglike_heads.hip) restated in float64 on plain torch, built on tests/loglike_ref.py.

    logit[g, r] = h[g, r, :] . w[g, :] + bias[g]                         (the one-logit heads)
    rec[g, r]   = bce_with_logits(logit[g, r], target[r % B, g])
    logw[j, k, b] = ratio[k, b] - rec[sel[j], k, b]                      j = 0 .. S-1   (the marginals)
    logw[S, k, b] = ratio[k, b] - sum_j rec[sel[j], k, b]                               (the joint)
    L[j, b]       = logsumexp_k logw[j, k, b] - log K

``heads`` and ``fold`` are the kernel-level restatements, ``estimates`` starts from (mu, logvar, eps), ``celeba19_case``
runs the CPU model of oracle/models.py in eval mode for the end-to-end cases."""
import torch

import loglike_ref as LR

ATTRIBUTES = ('Bald', 'Bangs', 'Black_Hair', 'Blond_Hair', 'Brown_Hair', 'Bushy_Eyebrows', 'Eyeglasses', 'Gray_Hair',
              'Heavy_Makeup', 'Male', 'Mouth_Slightly_Open', 'Mustache', 'Pale_Skin', 'Receding_Hairline', 'Smiling',
              'Straight_Hair', 'Wavy_Hair', 'Wearing_Hat')
MODALITIES = ('image',) + ATTRIBUTES
# (score, given) of the end-to-end test; None = all 19, 'attrs' = the 18 attributes
E2E_CASES = ((None, None), (('image',), None), ('attrs', ('image',)), (('Male', 'Smiling'), ('image', 'Eyeglasses')),
             (('Male',), ('Male',)))
E2E_B, E2E_K, E2E_D = 3, 5, 20


def expand(names):
    """None, a name, 'attrs' or a sequence of them -> the modalities named, in MODALITIES order."""
    if names is None:
        return MODALITIES
    names = (names,) if isinstance(names, str) else tuple(names)
    named = set()
    for n in names:
        named.update(ATTRIBUTES if n == 'attrs' else (n,))
    assert named <= set(MODALITIES), named
    return tuple(m for m in MODALITIES if m in named)


def heads(h, w, bias, target):
    """h [G, R, H], w [G, H], bias [G], target [T, G] (row r reads target row r % T) -> (logit, rec) [G, R], float64."""
    h, w, bias, target = LR._d(h), LR._d(w), LR._d(bias), LR._d(target)
    G, R, _ = h.shape
    logit = (h * w.unsqueeze(1)).sum(dim=2) + bias.reshape(G, 1)
    t = target[torch.arange(R) % target.shape[0]].t()                      # [G, R]
    return logit, LR.bce_with_logits(logit, t)


def fold(ratio, rec, sel=None):
    """ratio [K, B], rec [rows, K * B] loss rows (-log p), sel: the rows scored (None = all, in order) ->
    (logw [S + 1, K, B], L [S + 1, B])."""
    ratio, rec = LR._d(ratio), LR._d(rec)
    K, B = ratio.shape
    sel = list(range(rec.shape[0])) if sel is None else list(sel)
    terms = [rec[s, :K * B].reshape(K, B) for s in sel]
    logw = [ratio - t for t in terms]
    tot = torch.zeros_like(ratio)
    for t in terms:
        tot = tot + t
    logw = torch.stack(logw + [ratio - tot])
    return logw, torch.stack([LR.estimate(w) for w in logw])


def estimates(mu, logvar, eps, rec, sel=None):
    """(mu, logvar) [B, D], eps [K, B, D], rec / sel as in ``fold`` -> (z, logw, L)."""
    z, ratio = LR.draw(mu, logvar, eps)
    logw, L = fold(ratio, rec, sel)
    return z, logw, L


def celeba19_pair(seed=191):
    """(CPU oracle model in eval mode with randomised running statistics, image [B, 3, 64, 64], attrs [B, 18], eps)."""
    from oracle import models as OM
    o = OM.fill_parameters(OM.Celeba19MVAE(E2E_D), seed)
    LR.randomise_running_stats([o], seed + 1)
    o.eval()
    g = torch.Generator().manual_seed(seed + 2)
    image = torch.rand(E2E_B, 3, 64, 64, generator=g)
    attrs = torch.randint(0, 2, (E2E_B, len(ATTRIBUTES)), generator=g).float()
    eps = torch.randn(E2E_K, E2E_B, E2E_D, generator=g)
    return o, image, attrs, eps


def celeba19_case(o, image, attrs, eps, score, given):
    """The restated {name: L [B], 'joint': L [B]} of one (score, given) case on the CPU oracle ``o``: its ``infer`` and its
    decoders' logits feed the float64 formulas."""
    score, given = expand(score), expand(given)
    K, B, D = eps.shape
    with torch.no_grad():
        lst = [attrs[:, i] if n in given else None for i, n in enumerate(ATTRIBUTES)]
        mu, lv = o.infer(image=image if 'image' in given else None, attrs=lst)
        z, _ = LR.draw(mu, lv, eps)
        zr = z.float().reshape(K * B, D)
        rec = torch.zeros(len(MODALITIES), K * B, dtype=torch.float64)
        if 'image' in score:
            rec[0] = -LR.log_p_bernoulli(o.image_decoder(zr).reshape(K, B, -1), image).reshape(K * B)
        for i, n in enumerate(ATTRIBUTES):
            if n in score:
                logit = LR._d(o.attr_decoders[i](zr)).reshape(K, B)
                rec[1 + i] = LR.bce_with_logits(logit, LR._d(attrs[:, i]).reshape(1, B)).reshape(K * B)
    sel = [MODALITIES.index(n) for n in score]
    _, _, L = estimates(mu, lv, eps, rec, sel)
    res = {n: L[j] for j, n in enumerate(score)}
    res['joint'] = L[len(score)]
    return res
