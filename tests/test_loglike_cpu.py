"""CPU: the float64 restatement of the importance-weighted log-likelihood checks itself; the Python wrapper and the two
C entry points refuse bad arguments before any launch; the MultiMNIST end-to-end case of tests/test_loglike_gpu.py
keeps its arg-max margins on the CPU restatement."""
import ctypes
import math

import pytest
import torch

import mvae_amd
from mvae_amd import _lib
from mvae_amd.loglike import log_likelihood
import loglike_ref as LR


# ----------------------------------------------------------------------------- the restatement
def _inputs(K, B=4, D=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g), torch.randn(K, B, D, generator=g)


def test_restatement_one_sample_is_its_log_weight():
    mu, lv, eps = _inputs(1)
    logits = torch.randn(1, 4, 10, generator=torch.Generator().manual_seed(1))
    label = torch.tensor([3, 0, 9, 5])
    z, logw, L = LR.loglike(mu, lv, eps, label_logits=logits, label=label)
    assert z.dtype == torch.float64 and z.shape == (1, 4, 6) and logw.shape == (1, 4) and L.shape == (4,)
    assert torch.allclose(L, logw[0], rtol=1e-14, atol=0)
    # the density ratio written out: log N(z; 0, 1) - log N(z; mu, exp(logvar)), the 2 pi terms cancelling
    zd, mud, lvd = z[0], mu.double(), lv.double()
    ratio = (-0.5 * zd ** 2).sum(1) - (-0.5 * lvd - 0.5 * (zd - mud) ** 2 / lvd.exp()).sum(1)
    cls = torch.log_softmax(logits[0].double() + 1e-6, dim=1)[torch.arange(4), label]
    assert torch.allclose(logw[0], ratio + cls, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('K', [2, 7, 64])
def test_restatement_identical_samples_give_the_log_weight(K):
    mu, lv, eps = _inputs(1, seed=2)
    eps = eps.expand(K, -1, -1)
    image = torch.rand(4, 1, 3, 3, generator=torch.Generator().manual_seed(3))
    logits = torch.randn(1, 4, 9, generator=torch.Generator().manual_seed(4)).expand(K, -1, -1)
    _, logw, L = LR.loglike(mu, lv, eps, image_logits=logits, image=image)
    assert torch.allclose(L, logw[0], rtol=1e-13, atol=1e-13)


def test_restatement_shift_of_all_log_weights_shifts_the_estimate():
    g = torch.Generator().manual_seed(5)
    logw = torch.randn(11, 5, generator=g).double() * 40 - 6000
    for c in (-812.5, 0.25, 3000.0):
        assert torch.allclose(LR.estimate(logw + c), LR.estimate(logw) + c, rtol=1e-13, atol=1e-10)
    # and it is a mean in the weight domain
    small = torch.randn(11, 5, generator=g).double()
    assert torch.allclose(LR.estimate(small), small.exp().mean(0).log(), rtol=1e-12, atol=1e-12)


def test_restatement_modal_terms():
    g = torch.Generator().manual_seed(6)
    x, t = torch.randn(2, 3, 18, generator=g), torch.randint(0, 2, (3, 18), generator=g).float()
    want = -torch.nn.functional.binary_cross_entropy_with_logits(x.double(), t.double().expand(2, 3, 18), reduction='none').sum(2)
    assert torch.allclose(LR.log_p_bernoulli(x, t), want, rtol=1e-12, atol=1e-12)
    words, text = torch.randn(2, 3, 4, 12, generator=g), torch.randint(0, 12, (3, 4), generator=g)
    want = sum(LR.log_p_class(words[:, :, i], text[:, i]) for i in range(4))
    assert torch.allclose(LR.log_p_text(words, text), want, rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------------------- the Python wrapper
def test_wrapper_refuses_bad_arguments_before_any_launch():
    m = mvae_amd.mnist.model.MVAE(8)
    image, label = torch.rand(2, 1, 28, 28), torch.tensor([1, 2])
    assert mvae_amd.log_likelihood is log_likelihood
    with pytest.raises(ValueError, match='no label'):
        log_likelihood(m, image=image)                                     # given defaults to image + label
    with pytest.raises(ValueError, match='no image'):
        log_likelihood(m, label=label, score=('image',), given=('label',))
    with pytest.raises(ValueError, match='unknown modality'):
        log_likelihood(m, image=image, label=label, score=('pixels',))
    with pytest.raises(ValueError, match='unknown modality'):
        log_likelihood(m, image=image, label=label, given=('image', 'text'))
    with pytest.raises(ValueError, match='at least one'):
        log_likelihood(m, image=image, label=label, score=())
    with pytest.raises(ValueError, match='n_samples'):
        log_likelihood(m, image=image, label=label, n_samples=0)
    with pytest.raises(RuntimeError, match='GPU'):
        log_likelihood(m, image=image, label=label)                        # a model on the CPU
    with pytest.raises(NotImplementedError, match='celeba19'):
        log_likelihood(mvae_amd.celeba19.model.MVAE(8), image=torch.rand(2, 3, 64, 64), label=torch.zeros(2, 18))
    assert m.training                                                      # a refused call leaves the model alone


# ----------------------------------------------------------------------------- the C entry points
def test_iw_entry_points_refuse_bad_sizes_without_a_gpu():
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ctr = ctypes.cast((ctypes.c_uint64 * 1)(), ctypes.c_void_p)

    def draw(Kc, B, D, ld=None, mu=p, eps=p, counter=ctr, z=p, lw=p):
        return lib.mvae_iw_draw(mu, p, D if ld is None else ld, eps, 0, counter, 0, None, z, lw, Kc, B, D, None)
    for Kc, B, D in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4), (2, -3, 4), (2, 2, -4)):
        assert draw(Kc, B, D) == -1, (Kc, B, D)
    assert draw(2, 2, 4, ld=3) == -1                                       # leading dimension below D
    assert draw(2, 2, 4, mu=None) == -1 and draw(2, 2, 4, z=None) == -1 and draw(2, 2, 4, lw=None) == -1
    assert draw(2, 2, 4, eps=None, counter=None) == -1                     # no noise source
    assert draw(1 << 16, 1 << 15, 4) == -1                                 # Kc * B does not fit an int

    def acc(Kc, B, finish=0, lw=p, state=p, out=p, rec_a=None, rows_a=0):
        return lib.mvae_iw_accumulate(lw, rec_a, rows_a, None, 0, state, out, Kc, B, finish, None)
    for Kc, B in ((0, 3), (3, 0), (-2, 3), (3, -1)):
        assert acc(Kc, B) == -1, (Kc, B)
    assert acc(3, 3, finish=-1) == -1
    assert acc(3, 3, lw=None) == -1 and acc(3, 3, state=None) == -1
    assert acc(3, 3, finish=3, out=None) == -1                             # finish needs somewhere to write
    assert acc(3, 3, rec_a=p, rows_a=0) == -1                              # a term of no rows


# ----------------------------------------------------------------------------- the MultiMNIST case's margins
def test_multimnist_case_keeps_its_argmax_margins_on_the_restatement():
    _, _, text, _, out = LR.multimnist_case()
    assert set(out) == set(LR.CASES)
    scored_text = 0
    for (score, given), res in out.items():
        assert torch.isfinite(res['L']).all() and res['L'].shape == (LR.MULTIMNIST_B,)
        if 'label' in score:
            scored_text += 1
            assert res['fed'].shape == (4, LR.MULTIMNIST_K * LR.MULTIMNIST_B)
            assert res['margin'] > LR.MARGIN, 'seed %d, score %s given %s: top-two margin %.3e' % (
                LR.MULTIMNIST_SEED, score, given, res['margin'])
    assert scored_text == 2
    assert math.isfinite(float(text.sum()))
