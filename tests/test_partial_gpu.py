"""GPU: weak supervision -- the ragged product of experts (csrc/poe_ragged.hip) and the indexed reconstruction terms
(csrc/loss_ragged.hip) against their float64 restatement, ``partial.PartialStep`` against the CPU oracle on sub-batches
and against ``BimodalStep`` at full presence, absent data never read, two optimizer steps, and ``mnist/train.py
--n-paired`` end to end.  Bar: ``util.REL_TOL`` with ``util.rel_err``; every test prints the error it measured."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mvae_amd
from mvae_amd import kernels as K, partial as P
from mvae_amd.engine import BimodalStep
from mvae_amd.optim import FusedAdam
from oracle import models as OM, steps as OS
from util import REL_TOL, note_redraws, rel_err

import partial_ref as PR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = [3, 1, 1, 3, 2, 1, 3]


def check(errs, what):
    print('%s: %s' % (what, ', '.join('%s %.2e' % kv for kv in sorted(errs.items()))))
    bad = {k: v for k, v in errs.items() if not v <= REL_TOL}
    assert not bad, '%s beyond %.0e: %s' % (what, REL_TOL, bad)


def guarded(rows, cols=None, guard=2):
    """A NaN-filled buffer of ``rows + guard`` rows: the launch may only write the first ``rows``."""
    shape = (rows + guard,) if cols is None else (rows + guard, cols)
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def guard_ok(buf, rows):
    return bool(torch.isfinite(buf[:rows]).all()) and bool(torch.isnan(buf[rows:]).all())


# ----------------------------------------------------------------------------- ragged PoE
def bimodal_case(present, D):
    pl = P.plan(present)
    return dict(E=2, T=3, B=pl.B, D=D, variant='A', slot=pl.slot, erow=pl.erow, masks=list(P.TERM_MASKS), R=pl.R,
                n_rows=[r.size for r in pl.expert_rows])


def general_case(E, T, B, D, seed):
    """Random presence and term masks: expert E-1 is on no row, the last term contains it and is active on no row, and
    each other term is active on a random half of the rows that have at least ONE of its experts -- so some active (t, b)
    lack an expert of the term's mask, which then drops out of that row's product (forward and backward)."""
    rng = np.random.RandomState(seed)
    has = rng.rand(E, B) < 0.6
    has[E - 1] = False
    has[0, 0] = True
    masks = [int(rng.randint(1, 1 << (E - 1))) for _ in range(T - 1)] + [(1 << (E - 1)) | 1]
    masks[0] = 1
    erow = np.full((E, B), -1, dtype=np.int32)
    for e in range(E):
        rows = np.flatnonzero(has[e])
        erow[e, rows] = np.arange(rows.size)
    slot = np.full((T, B), -1, dtype=np.int32)
    R = 0
    lacking = 0            # active (t, b) whose row lacks an expert of the term: that expert drops out of the row's product
    for t in range(T - 1):
        for b in range(B):
            mine = [has[e, b] for e in range(E) if (masks[t] >> e) & 1]
            if any(mine) and (rng.rand() < 0.5 or (t == 0 and b == 0)):
                slot[t, b] = R
                R += 1
                lacking += not all(mine)
    assert (slot[T - 1] < 0).all() and (erow[E - 1] < 0).all() and R > 0 and lacking > 0
    # some expert row that no active term contains: its gradient row must come out zero, not stale
    idle = [(e, b) for e in range(E) for b in range(B) if has[e, b] and not any(
        slot[t, b] >= 0 and (masks[t] >> e) & 1 for t in range(T))]
    assert idle
    return dict(E=E, T=T, B=B, D=D, variant='B', slot=slot, erow=erow, masks=masks, R=R,
                n_rows=[int(h.sum()) for h in has])


POE_CASES = {'mixed': lambda: bimodal_case(MIXED, 64), 'one_row': lambda: bimodal_case([3], 5),
             'general': lambda: general_case(5, 7, 9, 70, seed=3)}


@pytest.mark.parametrize('name', sorted(POE_CASES))
def test_ragged_poe_forward_and_backward_against_float64(name):
    c = POE_CASES[name]()
    E, T, B, D, R, variant = c['E'], c['T'], c['B'], c['D'], c['R'], c['variant']
    g = torch.Generator().manual_seed(11)
    heads = [torch.cat([torch.randn(n, D, generator=g), 0.5 * torch.randn(n, D, generator=g)], dim=1) if n else None
             for n in c['n_rows']]
    noise = torch.randn(T, B, D, generator=g)
    grads_in = [torch.randn(R, D, generator=g) for _ in range(3)] + [torch.randn(R, generator=g)]     # dz, dmu, dlv, dkl
    # float64
    h64 = [None if h is None else h.double().requires_grad_(True) for h in heads]
    mu64, lv64, z64, kl64 = PR.poe_ragged(h64, c['erow'], c['masks'], c['slot'], R, noise.double(), variant, D)
    dz, dmu, dlv, dkl = [t.double() for t in grads_in]
    ((z64 * dz).sum() + (mu64 * dmu).sum() + (lv64 * dlv).sum() + (kl64 * dkl).sum()).backward()
    # device
    erow = torch.from_numpy(c['erow']).to(DEV)
    slot = torch.from_numpy(c['slot']).to(DEV)
    masks = torch.tensor(c['masks'], dtype=torch.int32, device=DEV)
    hd = [None if h is None else h.to(DEV) for h in heads]
    mus = [None if h is None else h[:, :D] for h in hd]
    lvs = [None if h is None else h[:, D:] for h in hd]
    noise_d = noise.to(DEV)

    def run():
        out = [guarded(R, D), guarded(R, D), guarded(R, D), guarded(R)]
        K.poe_ragged_fwd(mus, lvs, erow, masks, slot, R, noise_d, out[0], out[1], out[2], out[3], variant, B)
        gh = [None if h is None else torch.full_like(h, float('nan')) for h in hd]
        K.poe_ragged_bwd(mus, lvs, erow, masks, slot, R, noise_d, out[0], out[1],
                         grads_in[0].to(DEV), grads_in[1].to(DEV), grads_in[2].to(DEV), grads_in[3].to(DEV),
                         [None if t is None else t[:, :D] for t in gh], [None if t is None else t[:, D:] for t in gh],
                         variant, B)
        torch.cuda.synchronize()
        return out, gh
    out, gh = run()
    for buf, what in zip(out, ('mu', 'logvar', 'z', 'kl')):
        assert guard_ok(buf, R), '%s: a row below R is not finite, or a guard row was written' % what
    errs = dict(mu=rel_err(out[0][:R], mu64), logvar=rel_err(out[1][:R], lv64), z=rel_err(out[2][:R], z64),
                kl=rel_err(out[3][:R], kl64))
    for e, (t, h) in enumerate(zip(gh, h64)):
        if t is None:
            continue
        assert bool(torch.isfinite(t).all()), 'expert %d: a gradient element was not written' % e
        ref = h.grad if h.grad is not None else torch.zeros_like(h)
        dead = ref.abs().amax(dim=1) == 0
        assert bool((t.cpu()[dead] == 0).all()), 'expert %d: a row no active term contains is not exactly zero' % e
        errs['grad%d' % e] = rel_err(t, ref)
    check(errs, 'ragged PoE %s (E=%d T=%d B=%d D=%d %s, R=%d)' % (name, E, T, B, D, variant, R))
    out2, gh2 = run()
    for a, b in zip(out + [t for t in gh if t is not None], out2 + [t for t in gh2 if t is not None]):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), 'two runs differ'


def test_ragged_poe_draw_mode_reads_the_dense_philox_stream():
    D, seed = 64, 12345
    counter = torch.tensor([5], dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(2)
    for present in (MIXED, [3] * 7):
        pl = P.plan(present)
        tb = pl.to(DEV)
        B, R = pl.B, pl.R
        hd = [torch.cat([torch.randn(r.size, D, generator=g), 0.5 * torch.randn(r.size, D, generator=g)], 1).to(DEV)
              for r in pl.expert_rows]
        mus, lvs = [h[:, :D] for h in hd], [h[:, D:] for h in hd]
        noise = torch.full((3, B, D), float('nan'), dtype=torch.float32, device=DEV)
        mu, lv, z, kl = guarded(R, D), guarded(R, D), guarded(R, D), guarded(R)
        K.poe_ragged_fwd(mus, lvs, tb.erow, tb.masks, tb.slot, R, noise, mu, lv, z, kl, 'A', B, draw=(seed, counter, 0))
        dense = torch.empty(3, B, D, dtype=torch.float32, device=DEV)
        K.philox_fill(dense, seed, counter, 0)
        torch.cuda.synchronize()
        assert counter.item() == 5                               # not advanced
        active = torch.from_numpy(pl.slot >= 0).to(DEV)
        assert torch.equal(noise[active], dense[active]), 'the stored noise is not the dense Philox value at (t, b)'
        assert bool(torch.isnan(noise[~active]).all()), 'noise was written for an inactive (term, row)'
        for buf in (mu, lv, z, kl):
            assert guard_ok(buf, R)
        eps = dense[active]                                      # [R', D] in (t, b) order -> compact rows
        rows = torch.from_numpy(pl.slot[pl.slot >= 0].astype(np.int64)).to(DEV)
        want = eps.double() * torch.exp(0.5 * lv[rows].double()) + mu[rows].double()
        err = rel_err(z[rows], want)
        print('draw mode, present %s: z from the stored noise, rel err %.2e' % (present, err))
        assert err <= REL_TOL
        if pl.n_joint == B:
            # full presence: the same draws as the dense kernel's (term order joint, image, label in both)
            noise2 = torch.empty(3, B, D, dtype=torch.float32, device=DEV)
            mu2, lv2, z2 = (torch.empty(3, B, D, dtype=torch.float32, device=DEV) for _ in range(3))
            kl2 = torch.empty(3, B, dtype=torch.float32, device=DEV)
            K.poe_fwd_draw(mus, lvs, tb.masks, noise2, seed, counter, 0, mu2, lv2, z2, kl2, 'A')
            assert torch.equal(noise2, noise)
            order = torch.from_numpy(pl.slot.astype(np.int64)).to(DEV)            # [3, B] compact row of (t, b)
            e2 = dict(z=rel_err(z[order.reshape(-1)], z2.reshape(-1, D)), kl=rel_err(kl[order.reshape(-1)], kl2.reshape(-1)))
            check(e2, 'full presence against mvae_poe_fwd_draw')


# ----------------------------------------------------------------------------- indexed losses
ROWMAP = [2, 0, 2, 0, 2]        # R' = 5 rows over B = 3 targets: target 0 twice, target 2 three times, target 1 never


def logits_without_zero(shape, what):
    for attempt in range(6):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(40 + attempt)) * 2.0
        if not bool((x == 0).any()):
            break
    note_redraws(what, attempt)
    assert attempt <= 1
    return x


@pytest.mark.parametrize('with_coef', [False, True])
@pytest.mark.parametrize('Pn', [784, 1, 6])
def test_indexed_bce_against_float64(Pn, with_coef):
    g = torch.Generator().manual_seed(7)
    x = logits_without_zero((5, Pn), 'indexed BCE P=%d' % Pn)
    target = torch.rand(3, Pn, generator=g)
    coef = (torch.rand(5, generator=g) + 0.5) if with_coef else None
    rows64, grad64 = PR.bce_rows_indexed(x, target, ROWMAP, coef)
    poisoned = target.clone()
    poisoned[1] = float('nan')                                     # the target no row maps to must not be read
    xd, td, rm = x.to(DEV), poisoned.to(DEV), torch.tensor(ROWMAP, dtype=torch.int32, device=DEV)
    cd = None if coef is None else coef.to(DEV)
    rows, dl = guarded(5)[:5], torch.full((5, Pn), float('nan'), device=DEV)
    K.bce_rows_indexed_fwd(xd, td, rm, rows, coef=cd, dlogits=dl)
    rows_plain = torch.empty(5, device=DEV)
    K.bce_rows_indexed_fwd(xd, td, rm, rows_plain, coef=cd)
    dl2 = torch.full((5, Pn), float('nan'), device=DEV)
    K.bce_rows_indexed_bwd(xd, td, rm, cd, dl2)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_plain), 'the rows with and without the fused gradient differ'
    assert torch.equal(dl, dl2) and bool(torch.isfinite(dl).all()), 'the fused gradient and the separate backward differ'
    check(dict(rows=rel_err(rows, rows64), dlogits=rel_err(dl, grad64)), 'indexed BCE P=%d coef=%s' % (Pn, with_coef))
    # through autograd
    xa = xd.clone().requires_grad_(True)
    out = mvae_amd.functional.BceRowsIndexedFn.apply(xa, td, rm, cd)
    out.sum().backward()
    assert torch.equal(out.detach(), rows) and torch.equal(xa.grad, dl)


@pytest.mark.parametrize('with_coef', [False, True])
def test_indexed_ce_against_float64(with_coef):
    Kc = 10
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, Kc, generator=g) * 3.0
    label = torch.tensor([4, -1, 9])                               # the label no row maps to is the sentinel
    coef = (torch.rand(5, generator=g) + 0.5) if with_coef else None
    rows64, grad64 = PR.ce_rows_indexed(x, label.clamp(min=0), ROWMAP, coef)
    xd, ld, rm = x.to(DEV), label.to(DEV), torch.tensor(ROWMAP, dtype=torch.int32, device=DEV)
    cd = None if coef is None else coef.to(DEV)
    rows, dl = torch.empty(5, device=DEV), torch.full((5, Kc), float('nan'), device=DEV)
    K.ce_rows_indexed_fwd(xd, ld, rm, rows, coef=cd, dlogits=dl)
    rows_plain = torch.empty(5, device=DEV)
    K.ce_rows_indexed_fwd(xd, ld, rm, rows_plain, coef=cd)
    dl2 = torch.full((5, Kc), float('nan'), device=DEV)
    K.ce_rows_indexed_bwd(xd, ld, rm, cd, dl2)
    torch.cuda.synchronize()
    assert torch.equal(rows, rows_plain) and torch.equal(dl, dl2) and bool(torch.isfinite(dl).all())
    check(dict(rows=rel_err(rows, rows64), dlogits=rel_err(dl, grad64)), 'indexed CE coef=%s' % with_coef)
    xa = xd.clone().requires_grad_(True)
    out = mvae_amd.functional.CeRowsIndexedFn.apply(xa, ld, rm, cd)
    out.sum().backward()
    assert torch.equal(out.detach(), rows) and torch.equal(xa.grad, dl)
    # a row that maps outside the batch, or onto the sentinel, becomes NaN instead of indexing anything
    K.ce_rows_indexed_fwd(xd, ld, torch.tensor([1, 7, 0, -1, 2], dtype=torch.int32, device=DEV), rows)
    assert torch.isnan(rows).tolist() == [True, True, False, True, False]


# ----------------------------------------------------------------------------- the step
LAM_I, LAM_L, BETA = 1.0, 50.0, 0.37
PATTERNS = {
    'mixed': (MIXED, None),
    'all_paired': ([3] * 7, None),
    'image_only': ([1] * 7, None),
    'keep_unpaired': ([3] * 7, [1, 0, 0, 1, 0, 1, 0]),
}


def build_pair(kind, weight_seed):
    cls, d = OM.MODELS[kind]
    oracle = OM.fill_parameters(cls(d), weight_seed).train()
    model = getattr(mvae_amd, kind).model.MVAE(d)
    model.load_state_dict(oracle.state_dict())
    model.to(DEV).train()
    model.finalize()
    return oracle, model, d


def batch_for(kind, present, seed, poison=True):
    """A synthetic batch whose ABSENT entries are poisoned: NaN pixels, label -1."""
    image, label = OS.synthetic_batch(kind, len(present), seed)
    present = np.asarray(present)
    if poison:
        image[torch.from_numpy((present & 1) == 0)] = float('nan')
        label[torch.from_numpy((present & 2) == 0)] = -1
    return image, label


def grad_errors(model, oracle):
    """rel err of every parameter gradient against the oracle's; a parameter the oracle did not reach must be exactly 0."""
    og = dict(oracle.named_parameters())
    worst, bad = 0.0, []
    for name, p in model.named_parameters():
        assert p.grad is not None, 'no gradient for ' + name
        ref = og[name].grad
        if ref is None:
            assert bool((p.grad == 0).all()), '%s: no active term reaches it, yet its gradient is not zero' % name
            continue
        err = rel_err(p.grad, ref)
        worst = max(worst, err)
        if not err <= REL_TOL:
            bad.append('%s %.3e' % (name, err))
    assert not bad, 'gradients beyond %.0e: %s' % (REL_TOL, '; '.join(bad))
    return worst


def partial_vs_oracle(kind, present, paired, what):
    for attempt in range(6):
        oracle, model, d = build_pair(kind, weight_seed=21)
        image, label = batch_for(kind, present, seed=60 + attempt)
        eps = torch.randn(3, len(present), d, generator=torch.Generator().manual_seed(4))
        total, terms, logits = PR.partial_step(oracle, image, label, present, paired, eps, LAM_I, LAM_L, BETA)
        step = P.PartialStep(model, LAM_I, LAM_L)
        elbo = step.step(image.to(DEV), label.to(DEV), BETA, present=present, paired=paired, noise=eps)
        mine = step.last_logits[0]
        if not (any(bool((x == 0).any()) for x in logits) or (mine is not None and bool((mine == 0).any()))):
            break       # (an exactly-zero logit sits on the reference BCE's gradient jump: re-draw, and say so)
    note_redraws(what, attempt)
    assert attempt <= 1
    total.backward()
    elbo = elbo.cpu()
    errs = dict(total=rel_err(elbo[3], total.detach()))
    for t, name in enumerate(('joint', 'image', 'label')):
        if float(terms[t]) == 0.0:
            assert elbo[t].item() == 0.0, 'the empty %s term is not 0' % name
        else:
            errs[name] = rel_err(elbo[t], terms[t].detach())
    errs['worst_grad'] = grad_errors(model, oracle)
    check(errs, what)
    return model, oracle, step, elbo


@pytest.mark.parametrize('pattern', sorted(PATTERNS))
@pytest.mark.parametrize('kind', ['mnist', 'fashionmnist'])
def test_partial_step_against_the_oracle_on_sub_batches(kind, pattern):
    present, paired = PATTERNS[pattern]
    model, oracle, step, _ = partial_vs_oracle(kind, present, paired, 'PartialStep %s %s' % (kind, pattern))
    if pattern == 'image_only':
        reached = [n for n, p in oracle.named_parameters() if p.grad is not None]
        assert reached and all(n.startswith('image_') for n in reached)
        assert step.last_plan.n == [0, 7, 0] and step.last_logits[1] is None


@pytest.mark.parametrize('kind', ['mnist', 'fashionmnist'])
def test_full_presence_matches_the_fused_step(kind):
    B = 7
    oracle, model, d = build_pair(kind, weight_seed=21)
    image, label = OS.synthetic_batch(kind, B, seed=60)
    eps = torch.randn(3, B, d, generator=torch.Generator().manual_seed(4))
    noise = {'eps': [eps[0], eps[1], eps[2]], 'mask': [None] * 3}
    total, terms, _ = OS.bimodal_step(oracle, kind, image, label, noise, LAM_I, LAM_L, BETA)
    total.backward()
    ref = torch.stack([t.detach() for t in terms] + [total.detach()])
    eng = BimodalStep(model, B, LAM_I, LAM_L)
    fused = eng.terms_in_reference_order(eng.step(image.to(DEV), label.to(DEV), BETA, noise=noise)).cpu().clone()
    worst_fused = grad_errors(model, oracle)
    fused_grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    step = P.PartialStep(model, LAM_I, LAM_L)
    ragged = step.step(image.to(DEV), label.to(DEV), BETA, noise=eps).cpu()       # present=None: every label is >= 0
    assert step.last_plan.n == [B, B, B]
    worst_ragged = grad_errors(model, oracle)
    between = max(rel_err(p.grad, fused_grads[n]) for n, p in model.named_parameters())
    check(dict(fused_terms=rel_err(fused, ref), ragged_terms=rel_err(ragged, ref), ragged_vs_fused_terms=rel_err(ragged, fused),
               fused_grads=worst_fused, ragged_grads=worst_ragged, ragged_vs_fused_grads=between),
          'full presence %s' % kind)


def test_absent_data_is_not_read():
    """Absent image rows hold NaN and absent labels -1 in one run, zeros and valid labels in the other: the same bits."""
    results = []
    for poison in (True, False):
        _, model, d = build_pair('mnist', weight_seed=21)
        image, label = batch_for('mnist', MIXED, seed=60, poison=poison)
        if not poison:
            image[torch.from_numpy((np.asarray(MIXED) & 1) == 0)] = 0.0
        eps = torch.randn(3, 7, d, generator=torch.Generator().manual_seed(4))
        step = P.PartialStep(model, LAM_I, LAM_L)
        elbo = step.step(image.to(DEV), label.to(DEV), BETA, present=MIXED, noise=eps)
        results.append((elbo.clone(), model.arena.grad.clone()))
    assert bool(torch.isfinite(results[0][0]).all()) and bool(torch.isfinite(results[0][1]).all())
    assert torch.equal(results[0][0], results[1][0]), 'the ELBO terms depend on absent data'
    assert torch.equal(results[0][1], results[1][1]), 'a gradient depends on absent data'
    # the convenience default reads the flags off the -1 labels of an always-present image
    _, model, d = build_pair('mnist', weight_seed=21)
    image, label = batch_for('mnist', [3, 1, 1, 3, 1, 1, 3], seed=60)
    step = P.PartialStep(model, LAM_I, LAM_L)
    step.step(image.to(DEV), label.to(DEV), BETA)
    assert step.last_plan.present.tolist() == [3, 1, 1, 3, 1, 1, 3]
    with pytest.raises(ValueError, match='observes no modality'):
        step.step(image.to(DEV), label.to(DEV), BETA, present=[3, 1, 0, 3, 1, 1, 3])


def test_two_adam_steps_on_drawn_noise():
    _, model, d = build_pair('mnist', weight_seed=21)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    step = P.PartialStep(model, LAM_I, LAM_L, seed=3)
    image, label = batch_for('mnist', MIXED, seed=60)
    before = model.arena.flat.clone()
    losses = []
    for _ in range(2):
        losses.append(step.step(image.to(DEV), label.to(DEV), BETA, present=MIXED)[3].item())
        opt.step()
    mid = step.noise.clone()
    assert all(np.isfinite(l) for l in losses) and step.counter.item() == 2
    assert not torch.equal(before, model.arena.flat) and bool(torch.isfinite(model.arena.flat).all())
    active = torch.from_numpy(step.last_plan.slot >= 0).to(DEV)
    assert bool(torch.isfinite(mid[active]).all())
    print('two ragged Adam steps: loss %.4f -> %.4f' % tuple(losses))


@pytest.mark.parametrize('mode', ['keep', 'drop'])
def test_n_paired_on_idx_files_flags_follow_the_dataset_indices(mode, tmp_path, monkeypatch):
    """Without --synthetic: ``train_common.run`` on generated IDX files, two shuffled epochs.  Pixel (0, 0) of image i is i,
    so every step can say which examples it was handed: their flags must be the paired subset's at those indices -- in
    both epochs, whatever the shuffle -- and in drop mode exactly the unpaired rows carry label -1."""
    from mvae_amd import train_common as TC
    from mvae_amd.mnist import train as MT
    from test_loader_cpu import write_idx
    n_train, n_paired, seed = 37, 9, 5
    rng = np.random.RandomState(1)
    data = tmp_path / 'data'
    data.mkdir()
    for stem, n in (('train', n_train), ('t10k', 11)):
        images = rng.randint(0, 256, (n, 28, 28))
        images[:, 0, 0] = np.arange(n)
        write_idx(str(data / ('%s-images-idx3-ubyte' % stem)), images)
        write_idx(str(data / ('%s-labels-idx1-ubyte' % stem)), np.arange(n) % 10)
    subset = P.paired_subset(n_train, n_paired, seed)
    seen = []
    real_step = P.PartialStep.step

    def recording_step(self, image, label, annealing_factor, present=None, paired=None, noise=None):
        index = torch.round(image[:, 0, 0, 0] * 255).long().cpu().numpy()
        want_present, want_paired = P.batch_flags(subset[index], mode)
        assert np.array_equal(present, want_present) and np.array_equal(paired, want_paired)
        lab = label.cpu().numpy()
        gone = (~subset[index]) if mode == 'drop' else np.zeros(len(index), dtype=bool)
        assert np.array_equal(lab[~gone], index[~gone] % 10) and bool((lab[gone] == -1).all())
        seen.append(index)
        return real_step(self, image, label, annealing_factor, present=present, paired=paired, noise=noise)
    monkeypatch.setattr(P.PartialStep, 'step', recording_step)
    args = TC.reference_parser('mnist').parse_args([
        '--cuda', '--epochs', '2', '--batch-size', '8', '--n-latents', '16', '--annealing-epochs', '2', '--lambda-text', '50',
        '--data-dir', str(data), '--out-dir', str(tmp_path / 'out'), '--n-paired', str(n_paired), '--paired-seed', str(seed),
        '--unpaired-labels', mode])
    TC.run('mnist', MT.MVAE, MT._test_total, args, args.lambda_text, annealing_epoch_offset=0)
    assert [len(i) for i in seen] == [8, 8, 8, 8, 5] * 2
    first, second = np.concatenate(seen[:5]), np.concatenate(seen[5:])
    assert sorted(first.tolist()) == sorted(second.tolist()) == list(range(n_train))     # each epoch: every example once
    assert not np.array_equal(first, second), 'the two epochs were not shuffled differently'
    assert int(subset[first].sum()) == n_paired
    assert os.path.exists(os.path.join(str(tmp_path / 'out'), 'checkpoint.pth.tar'))


@pytest.mark.parametrize('mode', ['keep', 'drop'])
def test_mnist_cli_with_n_paired(mode, tmp_path):
    from mvae_amd.mnist import train as MT
    script = os.path.join(ROOT, 'multimodal-vae-public_amd', 'mnist', 'train.py')
    cmd = [sys.executable, script, '--cuda', '--synthetic', '--epochs', '1', '--steps-per-epoch', '3', '--batch-size', '8',
           '--n-latents', '16', '--lambda-text', '50', '--annealing-epochs', '2', '--log-interval', '1', '--n-paired', '12',
           '--paired-seed', '5', '--unpaired-labels', mode, '--out-dir', str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    losses = [float(line.split('Loss: ')[1].split()[0]) for line in out.stdout.splitlines() if 'Train Epoch' in line]
    assert len(losses) == 3 and all(l == l and abs(l) < 1e7 for l in losses) and '====> Test Loss:' in out.stdout
    model = MT.load_checkpoint(os.path.join(str(tmp_path), 'checkpoint.pth.tar'))
    assert model.n_latents == 16
    state = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    assert set(state) == {'state_dict', 'best_loss', 'n_latents', 'optimizer'}
