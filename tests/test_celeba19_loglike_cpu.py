"""CPU: the host side of the CelebA-19 log-likelihood -- mvae_heads_bce_rows and mvae_iw_fold_rows (K25) refuse bad
arguments before any launch, the Python wrappers refuse CPU tensors, ``celeba19.loglike.log_likelihood`` refuses every bad
call with the model left in its mode, and the float64 restatement (tests/celeba19_loglike_ref.py) reduces to
tests/loglike_ref.py for CelebA's single label term."""
import ctypes

import pytest
import torch

import mvae_amd
from mvae_amd import _lib
from mvae_amd.celeba19 import loglike as CL, model as CM
import celeba19_loglike_ref as CR
import loglike_ref as LR

ERR_ARG = -1


@pytest.fixture(scope='module')
def host():
    buf = (ctypes.c_float * 64)()
    return _lib.lib(), ctypes.cast(buf, ctypes.c_void_p), buf


# ----------------------------------------------------------------------------- the C entry points
def test_heads_bce_rows_refuses_bad_arguments_without_a_gpu(host):
    lib, p, _ = host

    def call(h=p, ldh=8, h_gs=48, w=p, w_gs=8, bias=p, b_gs=1, target=p, target_rows=2, ldt=3, rec=p, rec_gs=6,
             logits=None, logits_gs=0, G=3, R=6, H=8):
        return lib.mvae_heads_bce_rows(h, ldh, h_gs, w, w_gs, bias, b_gs, target, target_rows, ldt, rec, rec_gs, logits,
                                       logits_gs, G, R, H, None)
    for name in ('h', 'w', 'bias', 'target', 'rec'):
        assert call(**{name: None}) == ERR_ARG, name
    for G in (0, -1, 4097):
        assert call(G=G, ldt=5000) == ERR_ARG, G
    for name in ('R', 'H', 'target_rows'):
        for bad in (0, -3):
            assert call(**{name: bad}) == ERR_ARG, (name, bad)
    assert call(ldh=7) == ERR_ARG                                            # ldh < H
    assert call(ldt=2) == ERR_ARG                                            # ldt < G
    assert call(G=4096, ldt=4096, R=1 << 19) == ERR_ARG                      # G * R = 2^31
    assert call(G=2, R=1 << 30) == ERR_ARG


def test_iw_fold_rows_refuses_bad_arguments_without_a_gpu(host):
    lib, p, _ = host

    def call(rec=p, rec_ss=6, sel=None, S=2, lw=p, state=p, out=p, Kc=3, B=2, finish=0):
        arr = None if sel is None else (ctypes.c_int * len(sel))(*sel)
        return lib.mvae_iw_fold_rows(rec, rec_ss, arr, S, lw, state, out, Kc, B, finish, None)
    for name in ('rec', 'lw', 'state'):
        assert call(**{name: None}) == ERR_ARG, name
    for S in (0, -1, 65):
        assert call(S=S) == ERR_ARG, S
    assert call(sel=[0, -1]) == ERR_ARG and call(sel=[-2, 1]) == ERR_ARG     # a negative sel entry
    for Kc, B in ((0, 2), (3, 0), (-3, 2), (3, -2)):
        assert call(Kc=Kc, B=B) == ERR_ARG, (Kc, B)
    assert call(rec_ss=5) == ERR_ARG                                         # rec_ss < Kc * B
    assert call(finish=-1) == ERR_ARG
    assert call(finish=3, out=None) == ERR_ARG                               # finish needs somewhere to write
    assert call(Kc=1 << 16, B=1 << 15, rec_ss=1 << 31) == ERR_ARG            # Kc * B = 2^31
    assert _lib.IW_FOLD_MAX == 64


# ----------------------------------------------------------------------------- the Python wrappers
def test_kernel_wrappers_refuse_cpu_tensors():
    K = mvae_amd.kernels
    with pytest.raises(RuntimeError, match='GPU'):
        K.heads_bce_rows(torch.zeros(3, 6, 8), torch.zeros(8), 8, torch.zeros(1), 1, torch.zeros(2, 3), torch.zeros(3, 6))
    with pytest.raises(RuntimeError, match='GPU'):
        K.iw_fold_rows(torch.zeros(3, 2), torch.zeros(4, 6), [0, 2], torch.zeros(3, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        K.linear_fwd_grouped_shared(torch.zeros(6, 8), 3, torch.zeros(4, 8), 32, torch.zeros(4), 4, None,
                                    torch.zeros(3, 6, 4))


def _data(B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, 64, 64, generator=g), torch.randint(0, 2, (B, 18), generator=g).float()


def test_modalities_are_the_image_and_the_attribute_columns():
    from mvae_amd.celeba import datasets as CD
    assert CL.MODALITIES == ('image',) + tuple(CD.IX_TO_ATTR_DICT[CD.ATTR_IX_TO_KEEP[i]] for i in range(18))
    assert CL.MODALITIES == CR.MODALITIES and len(CL.MODALITIES) == 19
    assert CL._names('attrs', 'score', ()) == CL.ATTRIBUTES
    assert CL._names(('Smiling', 'image', 'Male'), 'score', ()) == ('image', 'Male', 'Smiling')
    assert CL.DEFAULT_PATH in CL.PATHS and CL.DEFAULT_CHUNK_ROWS >= 1


def test_wrapper_refuses_bad_arguments_before_any_launch():
    m = CM.MVAE(8)
    m.train()
    m.image_decoder.eval()
    modes = [x.training for x in m.modules()]
    image, attrs = _data()
    ll = CL.log_likelihood
    with pytest.raises(ValueError, match='expected the celeba19 MVAE'):
        ll(mvae_amd.celeba.model.MVAE(8), image, attrs)
    with pytest.raises(ValueError, match='unknown modality'):
        ll(m, image, attrs, score=('image', 'Beard'))
    with pytest.raises(ValueError, match='unknown modality'):
        ll(m, image, attrs, given=('label',))
    with pytest.raises(ValueError, match='at least one'):
        ll(m, image, attrs, score=())
    with pytest.raises(ValueError, match='at least one'):
        ll(m, image, attrs, given=())
    with pytest.raises(ValueError, match='at least one'):
        ll(m)                                                                 # both sets default to the data passed
    with pytest.raises(ValueError, match='`Male` is scored but no attrs'):
        ll(m, image, score=('Male',), given=('image',))
    with pytest.raises(ValueError, match='`image` is given but no image'):
        ll(m, attrs=attrs, score='attrs', given=('image',))
    with pytest.raises(ValueError, match='`Bald` is scored and given but no attrs'):
        ll(m, image, score=('image', 'attrs'), given=('image', 'attrs'))
    with pytest.raises(ValueError, match=r'`image` must be \[B, 3, 64, 64\]'):
        ll(m, image[:, :, :32], attrs)
    with pytest.raises(ValueError, match=r'`attrs` must be \[B, 18\]'):
        ll(m, image, attrs[:, :17])
    with pytest.raises(ValueError, match=r'`attrs` must be \[B, 18\]'):
        ll(m, image, attrs[:, 0])
    with pytest.raises(ValueError, match='holds 2 data, `attrs` 1'):
        ll(m, image, attrs[:1])
    for bad in (0, -5):
        with pytest.raises(ValueError, match='n_samples'):
            ll(m, image, attrs, n_samples=bad)
        with pytest.raises(ValueError, match='chunk_rows'):
            ll(m, image, attrs, chunk_rows=bad)
    with pytest.raises(ValueError, match='eps must be'):
        ll(m, image, attrs, n_samples=4, eps=torch.zeros(4, 2, 9))
    with pytest.raises(ValueError, match='eps must be'):
        ll(m, image, attrs, n_samples=4, eps=torch.zeros(3, 2, 8))
    with pytest.raises(ValueError, match='path must be'):
        ll(m, image, attrs, path='eager')
    for path in CL.PATHS + (None,):
        with pytest.raises(RuntimeError, match='GPU'):
            ll(m, image, attrs, n_samples=4, eps=torch.zeros(4, 2, 8), path=path)      # a model on the CPU
    assert [x.training for x in m.modules()] == modes                        # a refused call leaves the model alone


def test_cli_without_cuda_exits_with_the_house_message():
    with pytest.raises(SystemExit, match='pass --cuda on a ROCm GPU box'):
        CL.main(['no_such_model.pth.tar', '--synthetic'])


# ----------------------------------------------------------------------------- the restatement
def test_restatement_with_one_row_is_the_bimodal_restatement():
    """S = 1 on the summed 18 attribute terms = ``loglike_ref.loglike`` for CelebA's single label term."""
    g = torch.Generator().manual_seed(7)
    K, B, D, G, H = 9, 4, 6, 18, 11
    mu, lv, eps = torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g), torch.randn(K, B, D, generator=g)
    h = torch.randn(G, K * B, H, generator=g)
    w, bias = torch.randn(G, H, generator=g) / H ** 0.5, 0.1 * torch.randn(G, generator=g)
    attrs = torch.randint(0, 2, (B, G), generator=g).float()
    logit, rec = CR.heads(h, w, bias, attrs)
    assert logit.shape == (G, K * B) and rec.dtype == torch.float64
    z0, logw0, L0 = LR.loglike(mu, lv, eps, label_logits=logit.t().reshape(K, B, G), label=attrs, label_kind='attrs')
    z, logw, L = CR.estimates(mu, lv, eps, rec.sum(dim=0, keepdim=True))
    assert logw.shape == (2, K, B) and L.shape == (2, B) and L.dtype == torch.float64
    assert torch.equal(z, z0)
    for j in range(2):                          # the marginal and the joint of one row are the same number
        assert torch.allclose(logw[j], logw0, rtol=1e-13, atol=0)
        assert torch.allclose(L[j], L0, rtol=1e-13, atol=0)
    # and the joint over the 18 separate rows is that number again
    _, logw18, L18 = CR.estimates(mu, lv, eps, rec)
    assert logw18.shape == (19, K, B)
    assert torch.allclose(logw18[18], logw0, rtol=1e-13, atol=0) and torch.allclose(L18[18], L0, rtol=1e-13, atol=0)


def test_restatement_joint_is_the_fold_of_the_summed_rows():
    g = torch.Generator().manual_seed(8)
    K, B = 11, 3
    ratio = -50 + 4 * torch.randn(K, B, generator=g)
    rec = 3 * torch.rand(6, K * B + 5, generator=g)                          # rows longer than K * B
    sel = [4, 0, 2]                                                          # skips and reorders
    logw, L = CR.fold(ratio, rec, sel)
    assert logw.shape == (4, K, B)
    for j, s in enumerate(sel):
        assert torch.equal(logw[j], ratio.double() - rec[s, :K * B].double().reshape(K, B))
    summed = (rec[4].double() + rec[0].double() + rec[2].double()).unsqueeze(0)
    logw1, L1 = CR.fold(ratio, summed)
    assert torch.allclose(logw[3], logw1[0], rtol=1e-14, atol=0) and torch.allclose(L[3], L1[0], rtol=1e-14, atol=0)
    assert torch.equal(logw1[0], logw1[1]) and torch.equal(L1[0], L1[1])
    assert (L <= logw.max(dim=1).values).all()                               # every estimate is below its largest log-weight
