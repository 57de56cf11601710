"""CPU: the host side of the whole-sequence TextEncoder kernels (csrc/gru_enc_seq.hip) -- the geometry query and the
argument checks that run before any launch.  No GPU is touched."""
import ctypes
import inspect

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib, kernels as K
from mvae_amd.multimnist import model as MM

GEOMETRIES = [(200, 128), (200, 200), (24, 10)]    # (H, P): the model's two latent sizes and one off every alignment
LDS_MAX = 160 * 1024


def ld(k):
    return ((k + 15) & ~15) + 4


def fwd_plan_bytes(H):
    """csrc/gru_enc_seq.hip, enc_lds_fwd: e, two ping-pong states and the reverse state / sum, 16 x ld(H) floats each."""
    return 4 * (4 * 16 * ld(H))


def bwd_plan_bytes(H, P):
    """enc_lds_bwd: dout 16 ld(P) | ds 16 H | carry 16 H | dgi, dgh 16 ld(3H) each (16 H is a multiple of 4)."""
    return 4 * (16 * ld(P) + 2 * 16 * H + 2 * 16 * ld(3 * H))


@pytest.mark.parametrize('H,P', GEOMETRIES)
@pytest.mark.parametrize('B', [1, 17, 4096])
@pytest.mark.parametrize('bidirectional', [0, 1])
def test_supported_geometries(B, H, P, bidirectional):
    assert _lib.lib().mvae_gru_enc_seq_supported(B, H, P, MM.n_characters, MM.max_length, bidirectional) == 1
    assert K.gru_enc_seq_supported(B, H, P, MM.n_characters, MM.max_length, bool(bidirectional)) is True


def test_documented_plan_sizes():
    """The byte counts DESIGN.md 5.10 and the unit's header quote."""
    assert fwd_plan_bytes(200) == 54272                                            # 53.0 KiB
    assert bwd_plan_bytes(200, 128) == 112384 and bwd_plan_bytes(200, 200) == 117504          # 109.8 / 114.8 KiB


def test_refused_geometries():
    """include/mvae_hip.h, K19: both kernels' LDS plans must fit the CU's 160 KiB = 40960 floats.  The backward's
    (16 ld(P) + 32 H + 32 ld(3H) floats, ld(K) = roundup16(K) + 4) is the tighter one.  At P = 128 (16 ld(P) = 2112):
    H = 298 has ld(894) = 900 -> 2112 + 9536 + 28800 = 40448 floats = 161792 bytes, the largest H that fits;
    H = 299 has ld(897) = 916 -> 2112 + 9568 + 29312 = 40992 floats = 163968 bytes, refused.  The forward's plan at
    H = 299 is 64 ld(299) floats = 78848 bytes, so the refusal is the backward's.  Offsets inside a time slice are
    32-bit: B * 4H must stay below 2^31."""
    q = _lib.lib().mvae_gru_enc_seq_supported
    assert bwd_plan_bytes(298, 128) == 161792 <= LDS_MAX < bwd_plan_bytes(299, 128) == 163968
    assert fwd_plan_bytes(299) == 78848 <= LDS_MAX
    assert all(bwd_plan_bytes(h, 128) > LDS_MAX for h in range(299, 400))          # 298 is the largest, not a gap
    for bidir in (0, 1):
        assert q(100, 298, 128, 12, 4, bidir) == 1
        assert q(100, 299, 128, 12, 4, bidir) == 0
        assert q(100, 1024, 128, 12, 4, bidir) == 0
        for bad in (0, -1):
            assert q(bad, 200, 128, 12, 4, bidir) == 0 and q(100, bad, 128, 12, 4, bidir) == 0
            assert q(100, 200, bad, 12, 4, bidir) == 0 and q(100, 200, 128, bad, 4, bidir) == 0
            assert q(100, 200, 128, 12, bad, bidir) == 0
        assert q(1 << 22, 200, 128, 12, 4, bidir) == 0                            # B * 4H >= 2^31
    # the exact edge: 4H = 1024, B = 2^21 gives exactly 2^31 (refused), one row fewer is taken (H = 256 fits both plans)
    assert bwd_plan_bytes(256, 128) <= LDS_MAX
    assert q(1 << 21, 256, 128, 12, 4, 1) == 0 and q((1 << 21) - 1, 256, 128, 12, 4, 1) == 1
    assert q(100, 200, 128, 12, 4, 2) == 0 and q(100, 200, 128, 12, 4, -1) == 0   # bidirectional is 0 or 1
    assert K.gru_enc_seq_supported(100, 299, 128, 12, 4, True) is False


def _buf():
    b = (ctypes.c_float * 64)()
    return b, ctypes.cast(b, ctypes.c_void_p)


# argument positions of mvae_gru_enc_seq_fwd: x, w_emb, w_ih, w_hh, b_ih, b_hh | w_ih_r, w_hh_r, b_ih_r, b_hh_r |
# w_h2p, b_h2p, out | e_all, h_all, gates, gates_r, s, idx_all | B, H, P, n_chars, L | stream
FWD_REQUIRED = [0, 1, 2, 3, 4, 5, 10, 11, 12]
FWD_REVERSE = [6, 7, 8, 9]
FWD_TAPE = [13, 14, 15, 17, 18]
FWD_GATES_R = 16


def _fwd_ok(p, bidirectional, tape):
    a = [p] * 6 + [p if bidirectional else None] * 4 + [p] * 3 + [None] * 6 + [2, 200, 128, 12, 4, None]
    if tape:
        for i in FWD_TAPE:
            a[i] = p
        if bidirectional:
            a[FWD_GATES_R] = p
    return a


def test_fwd_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep, p = _buf()
    for bidirectional in (False, True):
        for tape in (False, True):
            ok = _fwd_ok(p, bidirectional, tape)
            assert len(ok) == len(_lib._SIGNATURES['mvae_gru_enc_seq_fwd'][1])
            for i in FWD_REQUIRED:                                          # every required pointer
                a = list(ok); a[i] = None
                assert lib.mvae_gru_enc_seq_fwd(*a) == -1, i
            for i, v in ((19, 0), (19, -3), (20, 0), (20, -1), (21, 0), (22, 0), (23, 0), (23, -2), (20, 299), (20, 1024)):
                a = list(ok); a[i] = v                                      # B, H, P, n_chars, L
                assert lib.mvae_gru_enc_seq_fwd(*a) == -1, (i, v)
            for i in FWD_TAPE:                                              # a partial tape: one entry missing / alone
                a = list(ok); a[i] = None if tape else p
                assert lib.mvae_gru_enc_seq_fwd(*a) == -1, i
            for i in FWD_REVERSE:                                           # reverse parameters given only in part
                a = list(ok); a[i] = None if bidirectional else p
                assert lib.mvae_gru_enc_seq_fwd(*a) == -1, i
    a = _fwd_ok(p, False, True); a[FWD_GATES_R] = p                         # gates_r without reverse parameters
    assert lib.mvae_gru_enc_seq_fwd(*a) == -1
    a = _fwd_ok(p, False, False); a[FWD_GATES_R] = p
    assert lib.mvae_gru_enc_seq_fwd(*a) == -1
    a = _fwd_ok(p, True, False); a[FWD_GATES_R] = p                         # gates_r without the rest of the tape
    assert lib.mvae_gru_enc_seq_fwd(*a) == -1
    a = _fwd_ok(p, True, True); a[FWD_GATES_R] = None                       # a bidirectional tape without gates_r
    assert lib.mvae_gru_enc_seq_fwd(*a) == -1
    del keep


# mvae_gru_enc_seq_bwd: dout, w_h2p, w_ih, w_hh | w_ih_r | h_all, gates | gates_r | dgi_all, dgh_all | dgi_r, dgh_r |
# de_all | B, H, P, n_chars, L | stream
BWD_REQUIRED = [0, 1, 2, 3, 5, 6, 8, 9, 12]
BWD_REVERSE = [4, 7, 10, 11]


def test_bwd_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    keep, p = _buf()
    for bidirectional in (False, True):
        ok = [p] * 13 + [2, 200, 128, 12, 4, None]
        if not bidirectional:
            for i in BWD_REVERSE:
                ok[i] = None
        assert len(ok) == len(_lib._SIGNATURES['mvae_gru_enc_seq_bwd'][1])
        for i in BWD_REQUIRED:
            a = list(ok); a[i] = None
            assert lib.mvae_gru_enc_seq_bwd(*a) == -1, i
        for i, v in ((13, 0), (13, -1), (14, 0), (15, 0), (16, 0), (17, 0), (17, -1), (14, 299), (14, 1024)):
            a = list(ok); a[i] = v
            assert lib.mvae_gru_enc_seq_bwd(*a) == -1, (i, v)
        for i in BWD_REVERSE:                                               # the reverse set given only in part
            a = list(ok); a[i] = None if bidirectional else p               # (gates_r alone: without reverse parameters)
            assert lib.mvae_gru_enc_seq_bwd(*a) == -1, i
    del keep


def test_encoder_has_the_switch_and_keeps_the_reference_signature():
    assert list(inspect.signature(MM.TextEncoder.__init__).parameters) == ['self', 'n_latents', 'n_characters', 'n_hiddens',
                                                                           'bidirectional']
    assert isinstance(MM.TextEncoder.WHOLE_SEQUENCE_DEFAULT, bool)
    enc = MM.TextEncoder(8, MM.n_characters)
    assert isinstance(enc.whole_sequence, bool) and enc.whole_sequence is MM.TextEncoder.WHOLE_SEQUENCE_DEFAULT
    assert 'whole_sequence' not in enc.state_dict() and not any('whole' in k for k in enc.state_dict())
    assert sorted(enc.state_dict()) == sorted(MM.TextEncoder(8, MM.n_characters).state_dict())
    for whole in (True, False):
        enc.whole_sequence = whole
        with pytest.raises(RuntimeError, match='GPU'):
            enc(torch.zeros(2, 4, dtype=torch.int64))


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    """kernels.gru_enc_seq_fwd / _bwd check every tensor (GPU, dtype, contiguity, shape) before the C call."""
    H, P, B, L = 24, 10, 3, 2
    f = lambda *s: torch.zeros(*s)
    pf = (f(3 * H, H), f(3 * H, H), f(3 * H), f(3 * H))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        K.gru_enc_seq_fwd(torch.zeros(B, L, dtype=torch.int64), f(12, H), pf, None, f(P, H), f(P), f(B, P), None)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        K.gru_enc_seq_bwd(f(B, P), f(P, H), pf, None, 12, f(L + 1, B, H), f(L, B, 4 * H), None, f(L, B, 3 * H),
                          f(L, B, 3 * H), None, None, f(L, B, H))
