"""GPU: mvae_iw_score_multi (K24, csrc/loglike_multi.hip) against the float64 restatement (tests/vision_loglike_ref.py)
and against the compositions of the existing kernels it replaces, and ``vision.loglike.log_likelihood`` end to end -- both
``path``s -- against the restatement fed by the CPU model of tests/vision_ref.py in eval mode."""
import os
import re
import subprocess
import sys

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from mvae_amd.vision import loglike as VL, model as VM
import vision_loglike_ref as VR
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = 67
# one full chunk; three chunks, offset by one float (misaligned: scalar loads although P % 4 == 0); a vector tail; two
# scalar segments, one of them a chunk and one element
MIXED = (4096, 12288, 4100, 4097, 5)
MISALIGNED = 1
TABLES = {'mixed': MIXED, 'eight': (64,) * 8}


def close(a, b, what, tol):
    e = rel_err(a, b)
    print('%s: relative error %.3e (bound %.0e)' % (what, e, tol))
    assert e <= tol, '%s: relative error %.3e > %.1e' % (what, e, tol)


def close_per_state(got, ref, what, tol):
    assert got.shape == ref.shape
    for j in range(ref.shape[0]):
        close(got[j], ref[j], '%s, state %d' % (what, j), tol)


def offset_by_one_float(t):
    """The same values in storage that starts one float past an allocation: 4-byte, not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def make_case(table, B, seed):
    """lw [KT, B] and one (logits [KT * B, P], target [B, P]) per segment, on the host and on the device, with the
    float64 estimates -- computed once per (table, B) and left unchanged."""
    g = torch.Generator().manual_seed(seed)
    lw = -80 + 5 * torch.randn(KT, B, generator=g)
    segs = [(2 * torch.randn(KT * B, P, generator=g), torch.rand(B, P, generator=g)) for P in TABLES[table]]
    _, ref = VR.fold(lw, segs)
    dsegs = []
    for s, (x, t) in enumerate(segs):
        if table == 'mixed' and s == MISALIGNED:
            dsegs.append((offset_by_one_float(x), offset_by_one_float(t)))
        else:
            dsegs.append((x.to(DEV), t.to(DEV)))
    return {'B': B, 'lw': lw.to(DEV), 'segs': dsegs, 'ref': ref}


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(table, B):
        if (table, B) not in cache:
            cache[(table, B)] = make_case(table, B, 100 * len(TABLES[table]) + B)
        return cache[(table, B)]
    return get


def fold(lw, segs, chunk):
    """Fold lw [K, B] and its segments in chunks of ``chunk`` samples: (out [S + 1, B], state [S + 1, B, 2])."""
    Kt, B = lw.shape
    S = len(segs)
    state = VL.fresh_state(S + 1, B, DEV)
    out = torch.full((S + 1, B), float('nan'), device=DEV)
    for k0 in range(0, Kt, chunk):
        k1 = min(Kt, k0 + chunk)
        K.iw_score_multi(lw[k0:k1], [(x[k0 * B:k1 * B], t) for x, t in segs], state, out, finish_k=Kt if k1 == Kt else 0)
    return out, state


# ----------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('table', sorted(TABLES))
def test_score_multi_matches_float64_in_one_chunk_and_in_ragged_chunks(table, B, cases):
    c = cases(table, B)
    one, _ = fold(c['lw'], c['segs'], KT)
    ragged, _ = fold(c['lw'], c['segs'], 3)               # 22 chunks of 3 and a last chunk of 1
    assert torch.isfinite(one).all() and torch.isfinite(ragged).all()
    close_per_state(one, c['ref'], 'one chunk vs float64', 1e-5)
    close_per_state(ragged, c['ref'], 'chunks of 3 vs float64', 1e-5)
    close_per_state(ragged, one, 'chunks of 3 vs one chunk', 1e-6)


@pytest.mark.parametrize('B', [1, 3, 17])
def test_score_multi_one_segment_against_one_chunk(B, cases):
    """S = 1 in one chunk: 1e-6 of float64, and the marginal and the joint are the same bits."""
    c = cases('mixed', B)
    for s in (0, MISALIGNED, 3, 4):
        out, state = fold(c['lw'], [c['segs'][s]], KT)
        ref = c['ref'][s]
        close(out[0], ref, 'segment %d alone vs float64' % s, 1e-6)
        assert torch.equal(out[0], out[1]) and torch.equal(state[0], state[1]), 'S = 1: state 0 and state 1 differ'


# ----------------------------------------------------------------------------- the kernel against the existing kernels
def accumulate(lw, terms):
    B = lw.shape[1]
    state = VL.fresh_state(1, B, DEV)[0]
    out = torch.full((B,), float('nan'), device=DEV)
    K.iw_accumulate(lw, terms, state, out, finish_k=lw.shape[0])
    return out


@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('table', sorted(TABLES))
def test_score_multi_equals_the_compositions_it_replaces(table, B, cases):
    c = cases(table, B)
    lw, segs = c['lw'], c['segs']
    R = KT * B
    out, _ = fold(lw, segs, KT)
    rowsum = torch.empty(R, device=DEV)
    K.bce_multi_fwd([(x, t, None, 1.0) for x, t in segs], rowsum)
    close(out[len(segs)], accumulate(lw, [(rowsum, 1)]), 'joint vs bce_multi_fwd (weights 1) + iw_accumulate', 1e-6)
    for s, (x, t) in enumerate(segs):
        K.bce_multi_fwd([(x, t, None, 1.0)], rowsum)
        close(out[s], accumulate(lw, [(rowsum, 1)]), 'marginal %d vs its single-segment composition' % s, 1e-6)


# ----------------------------------------------------------------------------- edge cases
def test_score_multi_is_deterministic(cases):
    c = cases('mixed', 3)
    a, sa = fold(c['lw'], c['segs'], 3)
    b, sb = fold(c['lw'], c['segs'], 3)
    assert torch.equal(a, b) and torch.equal(sa, sb), 'two identical calls gave different bits'


def test_score_multi_first_chunk_from_the_empty_state_is_not_nan():
    g = torch.Generator().manual_seed(5)
    lw = torch.tensor([[-2.0, float('-inf')], [-1.0, float('-inf')]])
    segs = [(torch.randn(4, P, generator=g), torch.rand(2, P, generator=g)) for P in (5, 64)]
    _, ref = VR.fold(lw, segs)
    out, state = fold(lw.to(DEV), [(x.to(DEV), t.to(DEV)) for x, t in segs], 1)
    assert not torch.isnan(state).any() and not torch.isnan(out).any()
    close_per_state(out[:, :1], ref[:, :1], 'finite column', 1e-6)
    assert (out[:, 1] == float('-inf')).all()                  # no mass at all: log 0, not NaN


@pytest.mark.parametrize('B', [1, 3])
def test_score_multi_six_modality_magnitudes(B):
    """The vision shapes: six segments of 49,152 elements together, reconstruction sums near 3e4 with a spread of about
    +-300 between the samples -- exp() of any log-weight alone is 0 in fp32."""
    g = torch.Generator().manual_seed(60 + B)
    Ps = [VM.N_CHANNELS[m] * 64 * 64 for m in VM.MODALITIES]
    lw = 100 * torch.randn(KT, B, generator=g).clamp(-3, 3)
    # bce(x, t) with t ~ U(0, 1) averages softplus(x) - x / 2 ~ log 2 + x^2 / 8: about 0.70 per element, 3.4e4 per sample,
    # and a row offset c in [0, 0.33] moves a row's total by 49152 * c^2 / 8, up to ~670
    shift = 0.33 * torch.rand(KT * B, 1, generator=g)
    segs = [(0.2 * torch.randn(KT * B, P, generator=g) + shift, torch.rand(B, P, generator=g)) for P in Ps]
    logw, ref = VR.fold(lw, segs)
    rec = lw.double() - logw[len(Ps)]
    assert 2.5e4 < rec.min() and rec.max() < 4e4 and rec.max() - rec.min() > 300
    assert (torch.exp(logw.float()) == 0).all()
    dsegs = [(x.to(DEV), t.to(DEV)) for x, t in segs]
    for chunk in (KT, 3):
        out, state = fold(lw.to(DEV), dsegs, chunk)
        assert torch.isfinite(out).all() and torch.isfinite(state).all()
        close_per_state(out, ref, 'chunk %d' % chunk, 1e-5)


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def pair():
    o, data, eps = VR.vision_pair()
    model = VM.MVAE(VR.E2E_D)
    model.load_state_dict(o.state_dict(), strict=True)
    model.to(DEV)
    model.train()                                               # log_likelihood switches to eval() itself
    return o, model, data, eps


@pytest.mark.parametrize('case', range(len(VR.E2E_CASES)))
def test_log_likelihood_matches_restatement(case, pair):
    o, model, data, eps = pair
    score, given = VR.E2E_CASES[case]
    ref = VR.vision_case(o, data, eps, score, given)
    for path in VL.PATHS:
        got = VL.log_likelihood(model, data, score=score, given=given, n_samples=VR.E2E_K, chunk_rows=6, eps=eps,
                                per_modality=True, path=path)               # chunks of 2, 2 and 1 samples
        assert list(got) == list(ref), (list(got), list(ref))
        for name in ref:
            assert got[name].shape == (VR.E2E_B,) and got[name].is_cuda and got[name].dtype == torch.float32
            close(got[name], ref[name], 'case %d, path %s, %s' % (case, path, name), REL_TOL)
        joint = VL.log_likelihood(model, data, score=score, given=given, n_samples=VR.E2E_K, chunk_rows=6, eps=eps,
                                  path=path)
        assert torch.equal(joint, got['joint']), 'the default return is not the joint of per_modality=True'


@pytest.mark.parametrize('path', VL.PATHS)
def test_log_likelihood_does_not_depend_on_the_chunking(path, pair):
    _, model, data, eps = pair
    outs = [VL.log_likelihood(model, data, n_samples=VR.E2E_K, chunk_rows=rows, eps=eps, per_modality=True, path=path)
            for rows in (3, 6, 15, 4096)]
    for o in outs[1:]:
        for name in outs[0]:
            close(o[name], outs[0][name], 'chunk_rows, %s, %s' % (path, name), 1e-6)


@pytest.mark.parametrize('path', VL.PATHS)
def test_log_likelihood_device_noise_and_model_state(path, pair):
    _, model, data, _ = pair
    model.train()
    model.image_decoder.eval()                                  # a mixed state must come back as it was
    modes = [m.training for m in model.modules()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = VL.log_likelihood(model, data, n_samples=9, chunk_rows=12, seed=7, path=path)
    b = VL.log_likelihood(model, data, n_samples=9, chunk_rows=12, seed=7, path=path)
    c = VL.log_likelihood(model, data, n_samples=9, chunk_rows=12, seed=8, path=path)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), 'the same seed gave different bits'
    assert not torch.equal(a, c), 'different seeds gave the same estimate'
    assert [m.training for m in model.modules()] == modes and model.training
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), '%s changed' % k
    model.train()


def test_vision_loglike_cli(tmp_path):
    model = VM.MVAE(16)
    path = os.path.join(str(tmp_path), 'model_best.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'n_latents': 16}, path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'multimodal-vae-public_amd', 'vision', 'loglike.py'), path,
                          '--synthetic', '--cuda', '--n-samples', '4', '--batch-size', '2', '--per-modality'],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    means = re.findall(r'mean (-?[0-9.]+(?:e[-+]?\d+)?|nan|-?inf)', out.stdout)
    assert len(means) == 7, out.stdout
    for m in means:
        v = float(m)
        assert v == v and abs(v) != float('inf') and v < 0, out.stdout
