"""CPU: the host side of the vision log-likelihood -- mvae_iw_score_multi (K24) and its workspace query refuse bad
arguments before any launch, ``vision.loglike.log_likelihood`` refuses every bad call with the model left in its mode,
and the float64 restatement (tests/vision_loglike_ref.py) reduces to tests/loglike_ref.py for one segment."""
import ctypes

import pytest
import torch

import mvae_amd
from mvae_amd import _lib
from mvae_amd.vision import loglike as VL, model as VM
import loglike_ref as LR
import vision_loglike_ref as VR

ERR_ARG, ERR_WS = -1, -3


def _table(Ps, ptr):
    arr = (_lib.BceSeg * max(1, len(Ps)))()
    for s, P in enumerate(Ps):
        arr[s] = _lib.BceSeg(ptr, ptr, None, int(P), 1.0)
    return arr


@pytest.fixture(scope='module')
def host():
    buf = (ctypes.c_float * 64)()
    return _lib.lib(), ctypes.cast(buf, ctypes.c_void_p), buf


# ----------------------------------------------------------------------------- the C entry points
def test_ws_bytes_is_a_pure_host_function(host):
    lib, p, _ = host
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096, 12288, 5), p), 3, 6) == 6 * (1 + 3 + 1) * 4
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4097,), p), 1, 1) == 2 * 4
    # 0 for every table the launch refuses
    assert lib.mvae_iw_score_multi_ws_bytes(None, 1, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096,), p), 0, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096,) * 8, p), 9, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((0,), p), 1, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((-4,), p), 1, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096,), p), 1, 0) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096,), None), 1, 6) == 0
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096 * 3,), p), 1, (1 << 31) // 3 + 1) == 0      # R * chunks >= 2^31
    assert lib.mvae_iw_score_multi_ws_bytes(_table((4096 * 3,), p), 1, (1 << 31) // 3 - 1) == ((1 << 31) // 3 - 1) * 3 * 4


def test_score_multi_refuses_bad_arguments_without_a_gpu(host):
    lib, p, _ = host
    big = ctypes.c_size_t(1 << 40)
    ok = _table((64, 5), p)

    def call(table=ok, n=2, lw=p, state=p, out=p, Kc=3, B=2, finish=0, ws=p, ws_bytes=big):
        return lib.mvae_iw_score_multi(table, n, lw, state, out, Kc, B, finish, ws, ws_bytes, None)
    assert call(table=None) == ERR_ARG
    assert call(n=0) == ERR_ARG and call(n=-1) == ERR_ARG
    assert call(table=_table((64,) * 8, p), n=9) == ERR_ARG
    assert call(table=_table((64, 5), None)) == ERR_ARG                       # null logits and target
    half = _table((64, 5), p)
    half[1] = _lib.BceSeg(p, None, None, 5, 1.0)
    assert call(table=half) == ERR_ARG                                       # a null target alone
    half[1] = _lib.BceSeg(None, p, None, 5, 1.0)
    assert call(table=half) == ERR_ARG                                       # a null logits alone
    assert call(lw=None) == ERR_ARG and call(state=None) == ERR_ARG
    assert call(table=_table((64, 0), p)) == ERR_ARG and call(table=_table((-1, 5), p)) == ERR_ARG
    for Kc, B in ((0, 2), (3, 0), (-3, 2), (3, -2)):
        assert call(Kc=Kc, B=B) == ERR_ARG, (Kc, B)
    assert call(finish=-1) == ERR_ARG
    assert call(finish=3, out=None) == ERR_ARG                               # finish needs somewhere to write
    assert call(Kc=1 << 16, B=1 << 15) == ERR_ARG                            # Kc * B = 2^31
    assert call(table=_table((4096 * 3,), p), n=1, Kc=(1 << 31) // 3 + 1, B=1) == ERR_ARG      # R * chunks >= 2^31
    # scratch: 6 rows x 2 chunks x 4 bytes
    assert call(ws_bytes=ctypes.c_size_t(6 * 2 * 4 - 1)) == ERR_WS
    assert call(ws_bytes=ctypes.c_size_t(0)) == ERR_WS
    assert call(ws=None) == ERR_ARG


# ----------------------------------------------------------------------------- the Python wrapper
def _data(B=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {m: torch.rand(B, VM.N_CHANNELS[m], 64, 64, generator=g) for m in VM.MODALITIES}


def test_wrapper_refuses_bad_arguments_before_any_launch():
    m = VM.MVAE(8)
    m.train()
    m.image_decoder.eval()
    modes = [x.training for x in m.modules()]
    data = _data()
    ll = VL.log_likelihood
    with pytest.raises(ValueError, match='expected the vision MVAE'):
        ll(mvae_amd.mnist.model.MVAE(8), data)
    with pytest.raises(ValueError, match='unknown modality'):
        ll(m, data, score=('image', 'depth'))
    with pytest.raises(ValueError, match='unknown modality'):
        ll(m, data, given=('label',))
    with pytest.raises(ValueError, match='unknown modality'):
        ll(m, dict(data, rotated=data['image']))
    with pytest.raises(ValueError, match='at least one'):
        ll(m, data, score=())
    with pytest.raises(ValueError, match='at least one'):
        ll(m, data, given=())
    with pytest.raises(ValueError, match='at least one'):
        ll(m, {})                                                             # both sets default to the keys of data
    only = {'image': data['image']}
    with pytest.raises(ValueError, match='`gray` is scored but'):
        ll(m, only, score=('gray',), given=('image',))
    with pytest.raises(ValueError, match='`edge` is given but'):
        ll(m, only, score=('image',), given=('edge',))
    with pytest.raises(ValueError, match=r'`gray` must be \[B, 1, 64, 64\]'):
        ll(m, dict(data, gray=data['image']))
    with pytest.raises(ValueError, match=r'`image` must be \[B, 3, 64, 64\]'):
        ll(m, dict(data, image=data['image'][:, :, :32]))
    with pytest.raises(ValueError, match='holds 1 data'):
        ll(m, dict(data, watermark=data['watermark'][:1]))
    for bad in (0, -5):
        with pytest.raises(ValueError, match='n_samples'):
            ll(m, data, n_samples=bad)
        with pytest.raises(ValueError, match='chunk_rows'):
            ll(m, data, chunk_rows=bad)
    with pytest.raises(ValueError, match='eps must be'):
        ll(m, data, n_samples=4, eps=torch.zeros(4, 2, 9))
    with pytest.raises(ValueError, match='eps must be'):
        ll(m, data, n_samples=4, eps=torch.zeros(3, 2, 8))
    with pytest.raises(ValueError, match='path must be'):
        ll(m, data, path='eager')
    for path in VL.PATHS + (None,):
        with pytest.raises(RuntimeError, match='GPU'):
            ll(m, data, n_samples=4, eps=torch.zeros(4, 2, 8), path=path)     # a model on the CPU
    assert [x.training for x in m.modules()] == modes                        # a refused call leaves the model alone
    assert VL.DEFAULT_PATH in VL.PATHS and VL.DEFAULT_CHUNK_ROWS >= 1
    assert VL.BYTES_PER_ROW == 196608


def test_kernel_wrapper_refuses_cpu_tensors():
    K = mvae_amd.kernels
    lw, state = torch.zeros(3, 2), torch.zeros(2, 2, 2)
    with pytest.raises(RuntimeError, match='GPU'):
        K.iw_score_multi(lw, [(torch.zeros(6, 5), torch.zeros(2, 5))], state)


def test_cli_without_cuda_exits_with_the_house_message():
    with pytest.raises(SystemExit, match='pass --cuda on a ROCm GPU box'):
        VL.main(['no_such_model.pth.tar', '--synthetic'])


# ----------------------------------------------------------------------------- the restatement
def test_restatement_with_one_segment_is_the_bimodal_restatement():
    g = torch.Generator().manual_seed(7)
    K, B, D, P = 9, 4, 6, 37
    mu, lv, eps = torch.randn(B, D, generator=g), 0.3 * torch.randn(B, D, generator=g), torch.randn(K, B, D, generator=g)
    logits, image = 3 * torch.randn(K, B, P, generator=g), torch.rand(B, P, generator=g)
    z0, logw0, L0 = LR.loglike(mu, lv, eps, image_logits=logits, image=image)
    for shaped in (logits, logits.reshape(K * B, P)):
        z, logw, L = VR.estimates(mu, lv, eps, [(shaped, image)])
        assert logw.shape == (2, K, B) and L.shape == (2, B) and L.dtype == torch.float64
        assert torch.equal(z, z0)
        for j in range(2):                      # the marginal and the joint of one segment are the same number
            assert torch.allclose(logw[j], logw0, rtol=1e-14, atol=0)
            assert torch.allclose(L[j], L0, rtol=1e-14, atol=0)


def test_restatement_joint_is_the_sum_of_the_terms():
    g = torch.Generator().manual_seed(8)
    K, B = 11, 3
    ratio = -50 + 4 * torch.randn(K, B, generator=g)
    segs = [(torch.randn(K * B, P, generator=g), torch.rand(B, P, generator=g)) for P in (5, 64, 9)]
    logw, L = VR.fold(ratio, segs)
    assert logw.shape == (4, K, B)
    terms = [logw[s] - ratio.double() for s in range(3)]
    assert torch.allclose(logw[3], ratio.double() + terms[0] + terms[1] + terms[2], rtol=1e-14, atol=0)
    assert torch.allclose(L[3], torch.logsumexp(logw[3], 0) - torch.log(torch.tensor(float(K), dtype=torch.float64)),
                          rtol=1e-14, atol=0)
    # Jensen on the weights: no bound ties the joint to the marginals, but every estimate is below its largest log-weight
    assert (L <= logw.max(dim=1).values).all()
