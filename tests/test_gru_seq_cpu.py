"""CPU: the host side of the whole-sequence TextDecoder kernels (csrc/gru_seq.hip) -- the geometry query and the
argument checks that run before any launch.  No GPU is touched."""
import ctypes

import pytest

import mvae_amd  # noqa: F401
from mvae_amd import _lib, kernels as K
from mvae_amd.multimnist import model as MM

GEOMETRIES = [(200, 64), (200, 100), (24, 5)]      # (H, D): the model's two latent sizes and one off every alignment


@pytest.mark.parametrize('H,D', GEOMETRIES)
@pytest.mark.parametrize('B', [1, 17, 4096])
def test_supported_geometries(B, H, D):
    assert _lib.lib().mvae_gru_dec_seq_supported(B, H, D, MM.n_characters, MM.max_length) == 1
    assert K.gru_dec_seq_supported(B, H, D, MM.n_characters, MM.max_length) is True


def test_refused_geometries():
    """include/mvae_hip.h, K18: what the LDS plan does not hold is refused -- both kernels must fit the CU's 160 KiB
    (the forward needs 16 * (3 ld(H+D) + 3 ld(H)) floats: H = 1024, D = 64 is 408 KiB), the logits are one 16-column
    tile, and offsets inside a time slice are 32-bit."""
    q = _lib.lib().mvae_gru_dec_seq_supported
    assert q(100, 1024, 64, 12, 4) == 0          # LDS
    assert q(100, 200, 2048, 12, 4) == 0         # LDS through D
    assert q(100, 200, 64, 17, 4) == 0           # more than one tile of characters
    assert q(100, 200, 64, 16, 4) == 1
    assert q(0, 200, 64, 12, 4) == 0 and q(100, 0, 64, 12, 4) == 0 and q(100, 200, 0, 12, 4) == 0
    assert q(100, 200, 64, 0, 4) == 0 and q(100, 200, 64, 12, 0) == 0
    assert q(1 << 22, 200, 64, 12, 4) == 0       # B * 4H >= 2^31
    # the backward's plan (16 * (2 ld(3H) + 3H + 2D + 20) floats) is the tighter one: H = 256 still fits at D = 64
    assert q(100, 256, 64, 12, 4) == 1 and q(100, 320, 64, 12, 4) == 0


def _buf():
    b = (ctypes.c_float * 64)()
    return b, ctypes.cast(b, ctypes.c_void_p)


def test_fwd_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep, p = _buf()
    ok = [p] * 13 + [None, 1.0, p] + [None] * 7 + [None, 2, 200, 64, 12, 4, 10, None]
    assert len(ok) == len(_lib._SIGNATURES['mvae_gru_dec_seq_fwd'][1])
    for i in list(range(13)) + [15]:                           # every required pointer
        a = list(ok); a[i] = None
        assert lib.mvae_gru_dec_seq_fwd(*a) == -1, i
    for i, v in ((24, 0), (24, -3), (25, 0), (26, 0), (27, 17), (28, 0), (25, 1024)):      # B, H, D, n_chars, L
        a = list(ok); a[i] = v
        assert lib.mvae_gru_dec_seq_fwd(*a) == -1, (i, v)
    a = list(ok); a[16] = p                                    # a partial tape
    assert lib.mvae_gru_dec_seq_fwd(*a) == -1
    del keep


def test_bwd_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep, p = _buf()
    ok = [p] * 6 + [None, 1.0] + [p] * 12 + [2, 200, 64, 12, 4, None]
    assert len(ok) == len(_lib._SIGNATURES['mvae_gru_dec_seq_bwd'][1])
    for i in list(range(6)) + list(range(8, 20)):
        a = list(ok); a[i] = None
        assert lib.mvae_gru_dec_seq_bwd(*a) == -1, i
    for i, v in ((20, 0), (20, -1), (21, 0), (22, 0), (23, 17), (24, 0), (21, 1024)):
        a = list(ok); a[i] = v
        assert lib.mvae_gru_dec_seq_bwd(*a) == -1, (i, v)
    del keep


def test_decoder_has_the_switch_and_keeps_the_reference_signature():
    import inspect
    assert list(inspect.signature(MM.TextDecoder.__init__).parameters) == ['self', 'n_latents', 'n_characters', 'n_hiddens']
    dec = MM.TextDecoder(8, MM.n_characters)
    assert isinstance(dec.whole_sequence, bool)
    assert 'whole_sequence' not in dec.state_dict() and not any('whole' in k for k in dec.state_dict())
    with pytest.raises(RuntimeError, match='GPU'):
        import torch
        dec(torch.zeros(2, 8))
