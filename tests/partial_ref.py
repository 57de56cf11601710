"""Reference restatement for the weak-supervision tests (test infrastructure): the ragged product of experts and the
indexed reconstruction terms in float64, and the ragged train step as the CPU oracle evaluated on sub-batches.

The step: for each term with a non-empty row set I, ``model(image[I] or None, label[I] or None, eps=eps_t[I])`` on the
oracle module, ``oracle.functional.elbo_loss_label`` of it (a mean over |I| rows), scaled by |I| / B; the terms summed.
The stacks of mnist / fashionmnist have no BatchNorm and no Dropout, so a term on a sub-batch IS that term on those rows;
at full presence this is ``oracle.steps.bimodal_step`` term by term."""
import numpy as np
import torch

from oracle import functional as OF

POE_EPS = 1e-8
TERM_MODALITIES = ((True, True), (True, False), (False, True))      # (image, label) of joint / image-only / label-only


def poe_ragged(heads, erow, masks, slot, R, noise, variant, D):
    """float64 ragged PoE with the N(0,1) prior.  heads[e]: [n_e, 2D] double (or None); erow [E, B], slot [T, B] numpy;
    masks: T ints; noise: dense [T, B, D] double or None.  Returns mu, logvar, z [R, D] and kl [R] (rows no (t, b) owns
    stay zero), differentiable in the heads."""
    T, B = slot.shape
    rows = [None] * R
    for t in range(T):
        for b in range(B):
            s = int(slot[t, b])
            if s < 0:
                continue
            extra = POE_EPS if variant == 'A' else 0.0
            sum_t = torch.tensor(1.0 / (1.0 + POE_EPS + extra), dtype=torch.float64).expand(D)
            sum_mt = torch.zeros(D, dtype=torch.float64)
            for e in range(len(heads)):
                if not (masks[t] >> e) & 1 or erow[e, b] < 0:
                    continue
                h = heads[e][int(erow[e, b])]
                te = 1.0 / (torch.exp(h[D:]) + POE_EPS + extra)
                sum_t = sum_t + te
                sum_mt = sum_mt + h[:D] * te
            pmu, pvar = sum_mt / sum_t, 1.0 / sum_t
            plv = torch.log(pvar + POE_EPS) if variant == 'A' else torch.log(pvar)
            z = pmu if noise is None else noise[t, b] * torch.exp(0.5 * plv) + pmu
            kl = -0.5 * torch.sum(1.0 + plv - pmu * pmu - torch.exp(plv))
            rows[s] = (pmu, plv, z, kl)
    zero = torch.zeros(D, dtype=torch.float64)
    rows = [r if r is not None else (zero, zero, zero, zero.sum()) for r in rows]
    return (torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]), torch.stack([r[2] for r in rows]),
            torch.stack([r[3] for r in rows]))


def bce_rows_indexed(x, target, rowmap, coef=None):
    """float64: coef[r] * sum_p bce(x[r, p], target[rowmap[r], p]) and its gradient in x."""
    x = x.double().clone().requires_grad_(True)
    t = target.double()[torch.as_tensor(np.asarray(rowmap), dtype=torch.long)]
    rows = (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum(dim=1)
    if coef is not None:
        rows = rows * coef.double()
    rows.sum().backward()
    return rows.detach(), x.grad


def ce_rows_indexed(x, label, rowmap, coef=None):
    """float64: coef[r] * -log_softmax(x[r, :] + 1e-6)[label[rowmap[r]]] and its gradient in x."""
    x = x.double().clone().requires_grad_(True)
    y = label[torch.as_tensor(np.asarray(rowmap), dtype=torch.long)]
    rows = -torch.log_softmax(x + 1e-6, dim=1).gather(1, y.unsqueeze(1)).squeeze(1)
    if coef is not None:
        rows = rows * coef.double()
    rows.sum().backward()
    return rows.detach(), x.grad


def term_rows(present, paired):
    """Row sets of the joint / image-only / label-only term, as LongTensors."""
    present = np.asarray(present)
    paired = np.ones_like(present) if paired is None else np.asarray(paired)
    has_img, has_lbl = (present & 1) != 0, (present & 2) != 0
    return [torch.as_tensor(np.flatnonzero(a), dtype=torch.long)
            for a in (has_img & has_lbl & (paired != 0), has_img, has_lbl)]


def partial_step(oracle, image, label, present, paired, eps, lambda_image, lambda_label, annealing_factor):
    """The ragged step on the CPU oracle: (total, [joint, image, label], [image logits of the terms that have any]).
    ``eps``: [3, B, D] in term order.  Absent modalities are never indexed into a model call."""
    B = image.shape[0]
    terms, logits = [], []
    for t, rows in enumerate(term_rows(present, paired)):
        if rows.numel() == 0:
            terms.append(torch.zeros((), dtype=torch.float32))
            continue
        use_img, use_lbl = TERM_MODALITIES[t]
        img = image[rows] if use_img else None
        lbl = label[rows] if use_lbl else None
        ri, rl, mu, lv, _ = oracle(img, lbl, eps=eps[t][rows])
        e = OF.elbo_loss_label(ri if use_img else None, img, rl if use_lbl else None, lbl, mu, lv,
                               lambda_image, lambda_label, annealing_factor)
        terms.append(e * (rows.numel() / float(B)))
        if use_img:
            logits.append(ri)
    return terms[0] + terms[1] + terms[2], terms, logits
