"""GPU: the two kernels of csrc/loglike.hip against the float64 restatement (tests/loglike_ref.py) on the same inputs, and
``mvae_amd.log_likelihood`` end to end against the restatement fed by the CPU oracle's ``infer`` and decoder logits in
eval mode (MNIST, FashionMNIST, CelebA: oracle/models.py; MultiMNIST: tests/multimnist_ref.py)."""
import os
import re
import subprocess
import sys

import pytest
import torch

import mvae_amd
from mvae_amd import kernels as K
from mvae_amd.loglike import log_likelihood
from oracle import models as OM, steps as OS
import loglike_ref as LR
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW_SHAPES = [(1, 64, 1), (3, 5, 7), (17, 100, 4), (5, 64, 33)]      # (B, D, Kc)


def close(a, b, what, tol):
    e = rel_err(a, b)
    print('%s: relative error %.3e (bound %.0e)' % (what, e, tol))
    assert e <= tol, '%s: relative error %.3e > %.1e' % (what, e, tol)


# ----------------------------------------------------------------------------- mvae_iw_draw
def draw_inputs(B, D, Kc, strided):
    g = torch.Generator().manual_seed(1000 + 7 * B + D + Kc)
    mu, lv = torch.randn(B, D, generator=g), 0.5 * torch.randn(B, D, generator=g)
    eps = torch.randn(Kc, B, D, generator=g)
    if strided:                                     # column ranges of one [B, 2D] heads buffer
        heads = torch.cat((mu, lv), dim=1).to(DEV)
        return mu, lv, eps, heads[:, :D], heads[:, D:]
    return mu, lv, eps, mu.to(DEV), lv.to(DEV)


@pytest.mark.parametrize('B,D,Kc,strided', [s + (False,) for s in DRAW_SHAPES] + [(3, 5, 7, True)])
def test_iw_draw_matches_float64(B, D, Kc, strided):
    """z within 1e-6, lw within 1e-5 of float64 (max-normalised, util.rel_err).  The reference's own fp32 evaluation of the
    same sum errs by at most 3.1e-7 over 200 seeds of each of these shapes (measured on the CPU), so the 1e-5 stands."""
    mu, lv, eps, mu_d, lv_d = draw_inputs(B, D, Kc, strided)
    assert mu_d.stride(0) == (2 * D if strided else D)
    z = torch.full((Kc, B, D), float('nan'), device=DEV)
    lw = torch.full((Kc, B), float('nan'), device=DEV)
    K.iw_draw(mu_d, lv_d, z, lw, eps=eps.to(DEV))
    z_ref, lw_ref = LR.draw(mu, lv, eps)
    close(z, z_ref, 'z', 1e-6)
    close(lw, lw_ref, 'lw', 1e-5)


@pytest.mark.parametrize('B,D,Kc', DRAW_SHAPES)
def test_iw_draw_device_noise_is_the_philox_stream(B, D, Kc):
    mu, lv, _, mu_d, lv_d = draw_inputs(B, D, Kc, False)
    seed, offset = 0x1234ABCD5678, 3
    counter = torch.tensor([5], dtype=torch.int64, device=DEV)
    z, lw, eps_out = (torch.empty(Kc, B, D, device=DEV), torch.empty(Kc, B, device=DEV), torch.empty(Kc, B, D, device=DEV))
    K.iw_draw(mu_d, lv_d, z, lw, seed=seed, counter_dev=counter, counter_offset=offset, eps_out=eps_out)
    want = torch.empty(Kc, B, D, device=DEV)
    K.philox_fill(want, seed, counter, offset)
    assert torch.equal(eps_out, want), 'eps_out is not mvae_philox_fill at the same seed, counter and offset'
    assert counter.item() == 5, 'the launch counter was advanced'
    z2, lw2 = torch.empty_like(z), torch.empty_like(lw)
    K.iw_draw(mu_d, lv_d, z2, lw2, eps=eps_out)
    assert torch.equal(z, z2) and torch.equal(lw, lw2), 'drawn and replayed noise give different bits'
    z_ref, lw_ref = LR.draw(mu, lv, eps_out)
    close(z, z_ref, 'z on device noise', 1e-6)
    close(lw, lw_ref, 'lw on device noise', 1e-5)


# ----------------------------------------------------------------------------- mvae_iw_accumulate
def fresh_state(B):
    st = torch.zeros(B, 2, device=DEV)
    st[:, 0] = float('-inf')
    return st


def accumulate(lw, terms, chunk):
    """Fold lw [K, B] (host) and its terms [(rows [K, B, rps], rps)] in chunks of ``chunk`` samples."""
    Kt, B = lw.shape
    state, out = fresh_state(B), torch.full((B,), float('nan'), device=DEV)
    for k0 in range(0, Kt, chunk):
        k1 = min(Kt, k0 + chunk)
        K.iw_accumulate(lw[k0:k1].contiguous().to(DEV),
                        [(rows[k0:k1].contiguous().reshape(-1).to(DEV), rps) for rows, rps in terms], state,
                        out, finish_k=Kt if k1 == Kt else 0)
    return out, state


@pytest.mark.parametrize('B', [1, 17])
@pytest.mark.parametrize('rps', [(1,), (4,), (1, 4), (4, 1)])
def test_iw_accumulate_one_chunk_and_ragged_chunks(B, rps):
    Kt = 67
    g = torch.Generator().manual_seed(10 * B + sum(rps) + len(rps))
    lw = -80 + 5 * torch.randn(Kt, B, generator=g)
    terms = [(20 * torch.rand(Kt, B, r, generator=g) + 3 * torch.randn(Kt, B, 1, generator=g).abs(), r) for r in rps]
    ref = LR.estimate(lw.double() - sum(rows.double().sum(2) for rows, _ in terms))
    one, _ = accumulate(lw, terms, Kt)
    ragged, _ = accumulate(lw, terms, 3)                  # 22 chunks of 3 and a last chunk of 1
    close(one, ref, 'one chunk vs float64', 1e-5)
    close(ragged, ref, 'chunks of 3 vs float64', 1e-5)
    close(ragged, one, 'chunks of 3 vs one chunk', 1e-6)


@pytest.mark.parametrize('B', [1, 17])
def test_iw_accumulate_large_negative_log_weights(B):
    """CelebA-sized log-weights: around -6000 with a spread of +-300; exp() of any of them alone is 0 in fp32."""
    Kt = 67
    g = torch.Generator().manual_seed(40 + B)
    lw = 100 * torch.randn(Kt, B, generator=g).clamp(-3, 3)
    rec = 6000 + 300 * (2 * torch.rand(Kt, B, 1, generator=g) - 1) + lw.unsqueeze(2)       # logw = lw - rec in [-6300, -5700]
    ref = LR.estimate(lw.double() - rec.double().sum(2))
    assert ref.max() < -5600 and ref.min() > -6400
    for chunk in (Kt, 3):
        out, state = accumulate(lw, [(rec, 1)], chunk)
        assert torch.isfinite(out).all() and torch.isfinite(state).all()
        close(out, ref, 'chunk %d' % chunk, 1e-5)


@pytest.mark.parametrize('B', [1, 17])
def test_iw_accumulate_equal_rows_return_that_value(B):
    Kt = 67
    vals = torch.linspace(-1234.5, -3.25, B).reshape(1, B)
    lw = vals.expand(Kt, B).contiguous()
    for chunk in (Kt, 3):
        out, _ = accumulate(lw, [], chunk)
        close(out, vals[0], 'chunk %d' % chunk, 1e-6)
    # the same through a four-row term: logw = 0 - 4 * (-v / 4)
    out, _ = accumulate(torch.zeros(Kt, B), [((-vals / 4).reshape(1, B, 1).expand(Kt, B, 4).contiguous(), 4)], 3)
    close(out, vals[0], 'through a term of four rows', 1e-6)


def test_iw_accumulate_first_chunk_from_the_empty_state_is_not_nan():
    lw = torch.tensor([[-2.0, float('-inf')], [-1.0, float('-inf')]])
    out, state = accumulate(lw, [], 1)
    assert not torch.isnan(state).any()
    close(out[:1], LR.estimate(lw[:, :1]), 'finite column', 1e-6)
    assert out[1].item() == float('-inf')                  # no mass at all: log 0, not NaN


# ----------------------------------------------------------------------------- end to end
def bimodal_pair(kind, seed):
    cls, d = OM.MODELS[kind]
    oracle = OM.fill_parameters(cls(d), seed)
    model = getattr(mvae_amd, kind).model.MVAE(d)
    model.load_state_dict(oracle.state_dict())
    model.to(DEV)
    LR.randomise_running_stats([oracle, model], seed + 1)       # no-op for the models without BatchNorm
    oracle.eval()
    model.train()                                               # log_likelihood switches to eval() itself
    return oracle, model, d


def oracle_estimate(oracle, kind, image, label, eps, score, given):
    Kt, B, D = eps.shape
    with torch.no_grad():
        mu, lv = oracle.infer(image=image if 'image' in given else None, label=label if 'label' in given else None)
        z, _ = LR.draw(mu, lv, eps)
        zr = z.float().reshape(Kt * B, D)
        img = oracle.image_decoder(zr).reshape(Kt, B, -1) if 'image' in score else None
        lbl = None
        if 'label' in score:
            dec = oracle.attrs_decoder if kind == 'celeba' else oracle.text_decoder
            lbl = dec(zr).reshape(Kt, B, -1)
    return LR.loglike(mu, lv, eps, img, image, lbl, label, 'attrs' if kind == 'celeba' else 'class')[2]


@pytest.fixture(scope='module')
def pairs():
    cache = {}

    def get(kind):
        if kind not in cache:
            oracle, model, d = bimodal_pair(kind, 83)
            image, label = OS.synthetic_batch(kind, 3, seed=84)
            eps = torch.randn(5, 3, d, generator=torch.Generator().manual_seed(85))
            cache[kind] = (oracle, model, image, label, eps)
        return cache[kind]
    return get


@pytest.mark.parametrize('kind', ['mnist', 'fashionmnist', 'celeba'])
def test_log_likelihood_matches_oracle(kind, pairs):
    oracle, model, image, label, eps = pairs(kind)
    for score, given in LR.CASES:
        got = log_likelihood(model, image=image, label=label, score=score, given=given, n_samples=5, chunk_rows=6, eps=eps)
        assert got.shape == (3,) and got.is_cuda and got.dtype == torch.float32
        ref = oracle_estimate(oracle, kind, image, label, eps, score, given)
        close(got, ref, '%s score %s given %s' % (kind, '+'.join(score), '+'.join(given)), REL_TOL)


def test_log_likelihood_multimnist_matches_restatement():
    from mvae_amd.multimnist import model as MM
    o, image, text, eps, cases = LR.multimnist_case()
    for (score, given), res in cases.items():                   # on the CPU restatement alone, before anything runs on the GPU
        if 'label' in score:
            assert res['margin'] > LR.MARGIN, 'score %s given %s: top-two margin %.3e' % (score, given, res['margin'])
    model = MM.MVAE(LR.MULTIMNIST_D)
    model.load_state_dict(o.state_dict(), strict=True)
    model.to(DEV).train()
    for (score, given), res in cases.items():
        got = log_likelihood(model, image=image, label=text, score=score, given=given, n_samples=LR.MULTIMNIST_K,
                             chunk_rows=2 * LR.MULTIMNIST_B, eps=eps)
        if 'label' in score:
            assert torch.equal(model.text_decoder.last_fed.cpu(), res['fed']), 'fed-back characters differ'
        close(got, res['L'], 'multimnist score %s given %s' % ('+'.join(score), '+'.join(given)), REL_TOL)


def test_log_likelihood_does_not_depend_on_the_chunking(pairs):
    _, model, image, label, eps = pairs('celeba')               # BatchNorm in every stack: eval mode has no batch statistics
    outs = [log_likelihood(model, image=image, label=label, score=('image', 'label'), n_samples=5, chunk_rows=rows, eps=eps)
            for rows in (3, 6, 15, 4096)]
    for o in outs[1:]:
        close(o, outs[0], 'chunk_rows', 1e-6)


def test_log_likelihood_device_noise_and_model_state(pairs):
    _, model, image, label, _ = pairs('celeba')
    model.train()
    model.image_decoder.eval()                                  # a mixed state must come back as it was
    modes = [m.training for m in model.modules()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = log_likelihood(model, image=image, label=label, n_samples=9, chunk_rows=12, seed=7)
    b = log_likelihood(model, image=image, label=label, n_samples=9, chunk_rows=12, seed=7)
    c = log_likelihood(model, image=image, label=label, n_samples=9, chunk_rows=12, seed=8)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), 'the same seed gave different bits'
    assert not torch.equal(a, c), 'different seeds gave the same estimate'
    assert [m.training for m in model.modules()] == modes and model.training
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), '%s changed' % k
    model.train()


def test_loglike_cli(tmp_path):
    model = mvae_amd.mnist.model.MVAE(16)
    path = os.path.join(str(tmp_path), 'model_best.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'n_latents': 16}, path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'multimodal-vae-public_amd', 'mnist', 'loglike.py'), path,
                          '--synthetic', '--cuda', '--n-samples', '8', '--batch-size', '4'],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    m = re.search(r'mean (-?[0-9.]+(?:e[-+]?\d+)?|nan|-?inf)', out.stdout)
    assert m, out.stdout
    mean = float(m.group(1))
    assert mean == mean and abs(mean) != float('inf') and mean < 0, out.stdout
