"""GPU: the whole-sequence TextDecoder kernels (csrc/gru_seq.hip, ``TextDecoder.whole_sequence = True``) against the
CPU oracle and against the per-cell launches they replace, forward and backward.

Six cases (B, D, H, mode): a partial row tile, exactly one tile, one row past the tile edge, three tiles with the
second latent size, eval mode (no masks), and a geometry off every alignment (H = 24, D = 5: scalar weight loads, masked
k and column tails).  Per case the oracle runs ONCE (cached) and both HIP paths run once (cached).

Bars.  Against the oracle: 1e-4 relative (util.REL_TOL), the fed-back characters exact -- which presupposes that no
tolerated error can flip an arg-max, so each case first asserts, on the oracle alone, that the smallest top-2 gap of the
logits that are fed back is at least 5e-4 x max|logit| (five times the output tolerance).  Against the per-cell path:
both sides are fp32 on the same GPU and differ only in the summation order of their products (k-ordered MFMA chains
here, the Linear kernels' tilings there), so 1e-5."""
import functools

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from mvae_amd.multimnist import model as MM
from oracle import models as OM, multimnist as OMM
from util import REL_TOL, assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PER_CELL_TOL = 1e-5

CASES = [(1, 64, 200, True), (16, 64, 200, True), (17, 64, 200, True), (37, 100, 200, True), (19, 64, 200, False),
         (33, 5, 24, True)]
IDS = ['B%d-D%d-H%d-%s' % (b, d, h, 'train' if t else 'eval') for b, d, h, t in CASES]


def _inputs(B, D, H, train):
    z = torch.randn(B, D, generator=torch.Generator().manual_seed(40 + B))
    masks = OMM.draw_decoder_masks(B, H, torch.Generator().manual_seed(50 + B)) if train else None
    w8 = torch.randn(B, OMM.MAX_LENGTH, OMM.N_CHARACTERS, generator=torch.Generator().manual_seed(60 + B))
    return z, masks, w8


@functools.lru_cache(maxsize=None)
def oracle_run(B, D, H, train):
    dec = OM.fill_parameters(OMM.TextDecoder(D, n_hiddens=H), 41).train(train)
    z, masks, w8 = _inputs(B, D, H, train)
    zo = z.clone().requires_grad_()
    words, fed = dec(zo, dropout_masks=masks)
    (words * w8).sum().backward()
    grads = {n: p.grad.clone() for n, p in dec.named_parameters()}
    return dec.state_dict(), words.detach(), fed, zo.grad.clone(), grads


@functools.lru_cache(maxsize=None)
def hip_run(B, D, H, train, whole_sequence):
    sd = oracle_run(B, D, H, train)[0]
    dec = MM.TextDecoder(D, MM.n_characters, n_hiddens=H)
    dec.load_state_dict(sd)
    dec.to(DEV).train(train)
    dec.whole_sequence = whole_sequence
    z, masks, w8 = _inputs(B, D, H, train)
    zh = z.to(DEV).requires_grad_()
    words = dec(zh, dropout_masks=masks)
    (words * w8.to(DEV)).sum().backward()
    grads = {n: p.grad.detach().cpu() for n, p in dec.named_parameters()}
    return dec, words.detach().cpu(), dec.last_fed.cpu(), zh.grad.cpu(), grads


@pytest.mark.parametrize('B,D,H,train', CASES, ids=IDS)
def test_whole_sequence_matches_oracle(B, D, H, train):
    assert K.gru_dec_seq_supported(B, H, D, MM.n_characters, MM.max_length)
    _, o_words, o_fed, o_dz, o_grads = oracle_run(B, D, H, train)
    # precondition, on the oracle alone: a tolerated error cannot flip a fed-back character
    top2 = torch.topk(o_words[:, :OMM.MAX_LENGTH - 1, :], 2, dim=2).values
    gap = (top2[..., 0] - top2[..., 1]).min().item() / o_words.abs().max().item()
    print('B=%d D=%d H=%d %s: smallest fed-back top-2 gap %.2e x max|logit|' % (B, D, H, 'train' if train else 'eval', gap))
    assert gap >= 5 * REL_TOL, 'the case does not separate its arg-max from the tolerance: %.2e' % gap

    dec, words, fed, dz, grads = hip_run(B, D, H, train, True)
    assert dec.whole_sequence is True
    assert fed.dtype == torch.int64 and torch.equal(fed, o_fed), 'greedy feedback diverged from the oracle'
    worst = assert_close(words, o_words, 'words')
    worst = max(worst, assert_close(dz, o_dz, 'd z'))
    assert set(grads) == set(o_grads)
    for name in sorted(o_grads):
        worst = max(worst, assert_close(grads[name], o_grads[name], 'grad ' + name))
    print('  whole-sequence vs oracle: worst rel err %.2e' % worst)
    # without gradient tracking nothing is taped: the same logits and characters, bit for bit
    z, masks, _ = _inputs(B, D, H, train)
    with torch.no_grad():
        again = dec(z.to(DEV), dropout_masks=masks)
    assert torch.equal(again.cpu(), words) and torch.equal(dec.last_fed.cpu(), fed)


@pytest.mark.parametrize('B,D,H,train', CASES, ids=IDS)
def test_whole_sequence_matches_per_cell_path(B, D, H, train):
    _, words, fed, dz, grads = hip_run(B, D, H, train, True)
    cell, c_words, c_fed, c_dz, c_grads = hip_run(B, D, H, train, False)
    assert cell.whole_sequence is False
    assert torch.equal(fed, c_fed), 'the two paths fed different characters'
    errs = {'words': rel_err(words, c_words), 'd z': rel_err(dz, c_dz)}
    for name in sorted(c_grads):
        errs['grad ' + name] = rel_err(grads[name], c_grads[name])
    worst = max(errs, key=errs.get)
    print('B=%d D=%d H=%d %s: whole-sequence vs per-cell worst %.2e (%s)' % (B, D, H, 'train' if train else 'eval',
                                                                           errs[worst], worst))
    for what, e in errs.items():
        assert e <= PER_CELL_TOL, '%s: relative error %.3e > %.1e against the per-cell path' % (what, e, PER_CELL_TOL)


def test_device_drawn_masks_run_on_the_whole_sequence_path(monkeypatch):
    """Training mode without explicit masks: the draws come from the device stream, fresh per call, and the call goes
    through the one-launch kernels (the per-cell launcher is never reached)."""
    dec = MM.TextDecoder(64, MM.n_characters, n_hiddens=200)
    dec.load_state_dict(oracle_run(17, 64, 200, True)[0])
    dec.to(DEV).train()
    dec.whole_sequence = True
    calls = {'seq': 0}
    real = K.gru_dec_seq_fwd

    def counting(*a, **kw):
        calls['seq'] += 1
        return real(*a, **kw)

    def refuse(*a, **kw):
        raise AssertionError('the per-cell path ran')

    monkeypatch.setattr(K, 'gru_dec_seq_fwd', counting)
    monkeypatch.setattr(K, 'gru_cell_fwd', refuse)
    z = _inputs(17, 64, 200, True)[0].to(DEV)
    a = dec(z); b = dec(z)
    assert calls['seq'] == 2
    assert a.shape == (17, MM.max_length, MM.n_characters) and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert not torch.equal(a, b), 'device dropout masks must differ between calls'
    assert dec.last_fed.shape == (MM.max_length, 17) and bool((dec.last_fed[0] == MM.SOS).all())
