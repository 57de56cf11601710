"""GPU: the whole-sequence TextEncoder kernels (csrc/gru_enc_seq.hip, ``TextEncoder.whole_sequence = True``) against
the CPU oracle and against the per-cell launches they replace, forward and backward.

Seven cases (B, n_latents, H, L, bidirectional): a partial row tile, exactly one tile, one row past the tile edge, three
tiles with the second latent size, unidirectional (null reverse parameters, five backward launches), a geometry off
every alignment (H = 24, P = 10 < 16: scalar weight loads, masked k and column tails) and L = 1 (both directions consume
the same single position; tape slot 0 is the only ``h_prev``).  Per case the oracle runs ONCE (cached) and both HIP
paths run once (cached).  The text is ``randint(0, 12)``: characters repeat across rows and positions, so the one-launch
embedding backward accumulates.

Bars.  Against the oracle: 1e-4 relative (util.REL_TOL); the reverse direction's ``weight_hh`` gradient is exactly zero
on both sides (its cell starts from h = 0) and is asserted equal to zero, no relative error is formed.  Against the
per-cell path: both sides are fp32 on the same GPU and differ only in the summation order of their products (k-ordered
MFMA chains here, the Linear kernels' tilings there), so 1e-5, the bar of test_gru_seq_gpu.py."""
import functools

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from mvae_amd.multimnist import model as MM
from oracle import models as OM, multimnist as OMM
import multimnist_ref as R
from util import REL_TOL, assert_close, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PER_CELL_TOL = 1e-5
N_CHARS = 12
ZERO_GRAD = 'gru.weight_hh_l0_reverse'

CASES = [(1, 64, 200, 4, True), (16, 64, 200, 4, True), (17, 64, 200, 4, True), (37, 100, 200, 4, True),
         (19, 64, 200, 4, False), (33, 5, 24, 3, True), (18, 64, 200, 1, True)]
IDS = ['B%d-D%d-H%d-L%d-%s' % (b, d, h, l, 'bi' if bi else 'uni') for b, d, h, l, bi in CASES]


def _inputs(B, D, L):
    text = torch.randint(0, N_CHARS, (B, L), generator=torch.Generator().manual_seed(70 + B))
    g = torch.Generator().manual_seed(80 + B)
    return text, torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)


@functools.lru_cache(maxsize=None)
def oracle_run(B, D, H, L, bidir):
    enc = OM.fill_parameters(OMM.TextEncoder(D, N_CHARS, n_hiddens=H, bidirectional=bidir), 43)
    text, a, b = _inputs(B, D, L)
    mu, logvar = enc(text)
    (mu * a + logvar * b).sum().backward()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters()}
    return enc.state_dict(), mu.detach(), logvar.detach(), grads


def _hip_encoder(B, D, H, L, bidir, whole_sequence):
    enc = MM.TextEncoder(D, N_CHARS, n_hiddens=H, bidirectional=bidir)
    enc.load_state_dict(oracle_run(B, D, H, L, bidir)[0])
    enc.to(DEV)
    enc.whole_sequence = whole_sequence
    return enc


def _fwd_bwd(enc, B, D, L, text=None):
    t0, a, b = _inputs(B, D, L)
    for p in enc.parameters():
        p.grad = None
    mu, logvar = enc((t0 if text is None else text).to(DEV))
    (mu * a.to(DEV) + logvar * b.to(DEV)).sum().backward()
    return mu.detach().cpu(), logvar.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in enc.named_parameters()}


@functools.lru_cache(maxsize=None)
def hip_run(B, D, H, L, bidir, whole_sequence):
    enc = _hip_encoder(B, D, H, L, bidir, whole_sequence)
    return (enc,) + _fwd_bwd(enc, B, D, L)


@pytest.mark.parametrize('B,D,H,L,bidir', CASES, ids=IDS)
def test_whole_sequence_matches_oracle(B, D, H, L, bidir):
    assert K.gru_enc_seq_supported(B, H, 2 * D, N_CHARS, L, bidir)
    _, o_mu, o_logvar, o_grads = oracle_run(B, D, H, L, bidir)
    enc, mu, logvar, grads = hip_run(B, D, H, L, bidir, True)
    assert enc.whole_sequence is True
    worst = assert_close(mu, o_mu, 'mu')
    worst = max(worst, assert_close(logvar, o_logvar, 'logvar'))
    assert set(grads) == set(o_grads) and (ZERO_GRAD in grads) == bidir
    for name in sorted(o_grads):
        if name == ZERO_GRAD:       # the reverse cell starts from h = 0: exactly zero on both sides, no relative error
            assert not o_grads[name].any() and not grads[name].any(), name
            continue
        worst = max(worst, assert_close(grads[name], o_grads[name], 'grad ' + name))
    print('B=%d D=%d H=%d L=%d %s: whole-sequence vs oracle worst rel err %.2e' % (B, D, H, L, 'bi' if bidir else 'uni', worst))
    # without gradient tracking nothing is taped: the same output, bit for bit
    with torch.no_grad():
        mu2, logvar2 = enc(_inputs(B, D, L)[0].to(DEV))
    assert not mu2.requires_grad
    assert torch.equal(mu2.cpu(), mu) and torch.equal(logvar2.cpu(), logvar)


@pytest.mark.parametrize('B,D,H,L,bidir', CASES, ids=IDS)
def test_whole_sequence_matches_per_cell_path(B, D, H, L, bidir):
    _, mu, logvar, grads = hip_run(B, D, H, L, bidir, True)
    cell, c_mu, c_logvar, c_grads = hip_run(B, D, H, L, bidir, False)
    assert cell.whole_sequence is False and set(grads) == set(c_grads)
    errs = {'mu': rel_err(mu, c_mu), 'logvar': rel_err(logvar, c_logvar)}
    for name in sorted(c_grads):
        if name == ZERO_GRAD:
            assert not c_grads[name].any() and not grads[name].any(), name
            continue
        errs['grad ' + name] = rel_err(grads[name], c_grads[name])
    worst = max(errs, key=errs.get)
    print('B=%d D=%d H=%d L=%d %s: whole-sequence vs per-cell worst %.2e (%s)' % (B, D, H, L, 'bi' if bidir else 'uni',
                                                                                errs[worst], worst))
    for what, e in errs.items():
        assert e <= PER_CELL_TOL, '%s: relative error %.3e > %.1e against the per-cell path' % (what, e, PER_CELL_TOL)


def test_backward_through_a_tapeless_forward_raises():
    enc = hip_run(17, 64, 200, 4, True, True)[0]
    text = _inputs(17, 64, 4)[0].to(DEV)
    with torch.no_grad():
        out = MM._TextEncoderSeqFn.apply(text, True, False, enc.embed.weight, enc.h2p.weight, enc.h2p.bias,
                                         *(MM._cell_params(enc.gru, 0) + MM._cell_params(enc.gru, 0, True)))
    assert not out.requires_grad
    out = MM._TextEncoderSeqFn.apply(text, True, False, enc.embed.weight, enc.h2p.weight, enc.h2p.bias,
                                     *(MM._cell_params(enc.gru, 0) + MM._cell_params(enc.gru, 0, True)))
    with pytest.raises(RuntimeError, match='without gradient tracking'):
        out.sum().backward()


@pytest.mark.parametrize('bidir,B', [(True, 17), (False, 19)], ids=['bi', 'uni'])
def test_the_path_is_the_path(monkeypatch, bidir, B):
    """``whole_sequence = True``: one call of each sequence wrapper and no per-cell launcher; the backward issues seven
    launches (five when unidirectional): the recurrence, the Linear weight gradients and ONE embedding backward.
    ``False``: the sequence wrappers are never reached."""
    D, H, L = 64, 200, 4
    calls = {'fwd': 0, 'bwd': 0, 'wgrad': 0, 'emb_bwd': 0}

    def counting(key, real):
        def f(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)
        return f

    def refuse(what):
        def f(*a, **kw):
            raise AssertionError(what + ' ran')
        return f

    enc = _hip_encoder(B, D, H, L, bidir, True)
    with monkeypatch.context() as m:
        m.setattr(K, 'gru_enc_seq_fwd', counting('fwd', K.gru_enc_seq_fwd))
        m.setattr(K, 'gru_enc_seq_bwd', counting('bwd', K.gru_enc_seq_bwd))
        m.setattr(K, 'linear_wgrad', counting('wgrad', K.linear_wgrad))
        m.setattr(K, 'embedding_bwd', counting('emb_bwd', K.embedding_bwd))
        for name in ('gru_cell_fwd', 'gru_cell_bwd', 'embedding_fwd', 'linear_fwd', 'linear_dgrad', 'copy2d'):
            m.setattr(K, name, refuse('K.' + name))
        mu, _, grads = _fwd_bwd(enc, B, D, L)
    assert calls == {'fwd': 1, 'bwd': 1, 'wgrad': 5 if bidir else 3, 'emb_bwd': 1}, calls
    assert torch.isfinite(mu).all() and all(torch.isfinite(g).all() for g in grads.values())

    enc.whole_sequence = False
    with monkeypatch.context() as m:
        m.setattr(K, 'gru_enc_seq_fwd', refuse('K.gru_enc_seq_fwd'))
        m.setattr(K, 'gru_enc_seq_bwd', refuse('K.gru_enc_seq_bwd'))
        mu2, _, _ = _fwd_bwd(enc, B, D, L)
    assert rel_err(mu2, mu) <= PER_CELL_TOL


def test_out_of_range_characters_are_clamped():
    """A result check on valid memory: the kernel clamps a character to [0, n_chars) before it forms any address, as
    embedding_fwd_kernel does, so -3 reads row 0 and 40 reads row 11 -- forward, and in the embedding's gradient."""
    B, D, H, L = 17, 64, 200, 4
    enc = hip_run(B, D, H, L, True, True)[0]
    text = _inputs(B, D, L)[0].clone()
    text[0, 0], text[3, 2], text[16, 3], text[5, 1] = -3, 40, -3, 40
    clamped = text.clamp(0, N_CHARS - 1)
    assert not torch.equal(text, clamped)
    mu, logvar, grads = _fwd_bwd(enc, B, D, L, text)
    c_mu, c_logvar, c_grads = _fwd_bwd(enc, B, D, L, clamped)
    assert torch.equal(mu, c_mu) and torch.equal(logvar, c_logvar)
    for name in c_grads:
        assert torch.equal(grads[name], c_grads[name]), name
    with torch.no_grad():
        mu3, _ = enc(text.to(DEV))
    assert torch.equal(mu3.cpu(), c_mu)


def test_through_the_model():
    """``model(text=text)`` in eval mode at B = 6 on two models from one state_dict, the encoder's switch set in one and
    cleared in the other: mu, logvar and the text encoder's gradients agree to 1e-5."""
    B = 6
    sd = OM.fill_parameters(R.MVAE(64), 47).state_dict()
    text = OMM.synthetic_text(B, 48).to(DEV)
    g = torch.Generator().manual_seed(49)
    a, b = torch.randn(B, 64, generator=g).to(DEV), torch.randn(B, 64, generator=g).to(DEV)
    res = []
    for whole in (True, False):
        m = MM.MVAE(64)
        m.load_state_dict(sd, strict=True)
        m.to(DEV).eval()
        m.text_encoder.whole_sequence = whole
        _, _, mu, logvar = m(text=text)
        (mu * a + logvar * b).sum().backward()
        res.append((mu.detach().cpu(), logvar.detach().cpu(),
                    {n: p.grad.detach().cpu().clone() for n, p in m.text_encoder.named_parameters()}))
    (mu, logvar, grads), (c_mu, c_logvar, c_grads) = res
    errs = {'mu': rel_err(mu, c_mu), 'logvar': rel_err(logvar, c_logvar)}
    for name in sorted(c_grads):
        if name == ZERO_GRAD:
            assert not c_grads[name].any() and not grads[name].any(), name
            continue
        errs['grad ' + name] = rel_err(grads[name], c_grads[name])
    worst = max(errs, key=errs.get)
    print('MVAE(64) text-only, B=%d: whole-sequence vs per-cell worst %.2e (%s)' % (B, errs[worst], worst))
    for what, e in errs.items():
        assert e <= PER_CELL_TOL, '%s: relative error %.3e > %.1e' % (what, e, PER_CELL_TOL)
