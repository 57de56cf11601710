"""GPU: mvae_heads_bce_rows and mvae_iw_fold_rows (K25, csrc/loglike_heads.hip) against the float64 restatement
(tests/celeba19_loglike_ref.py) and against the compositions of the existing kernels they replace, and
``celeba19.loglike.log_likelihood`` end to end -- both ``path``s -- against the restatement fed by the CPU oracle
(oracle/models.py) in eval mode."""
import os
import re
import subprocess
import sys

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from mvae_amd.celeba19 import loglike as CL, model as CM
from mvae_amd.vision.loglike import fresh_state
import celeba19_loglike_ref as CR
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = 67
NAN = float('nan')


def close(a, b, what, tol):
    e = rel_err(a, b)
    print('%s: relative error %.3e (bound %.0e)' % (what, e, tol))
    assert e <= tol, '%s: relative error %.3e > %.1e' % (what, e, tol)


def close_per_state(got, ref, what, tol):
    assert got.shape == ref.shape
    for j in range(ref.shape[0]):
        close(got[j], ref[j], '%s, state %d' % (what, j), tol)


# ----------------------------------------------------------------------------- heads_bce_rows
def heads_inputs(G, B, H, seed):
    """Host tensors of one shape: h [G, KT * B, H] Swish-shaped activations, w [G, H] ~ 1 / sqrt(H), bias [G], target
    {0, 1} [B, G], and the float64 (logit, rec) [G, R]."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(G, KT * B, H, generator=g)
    h = h * torch.sigmoid(h)
    w = torch.randn(G, H, generator=g) / H ** 0.5
    bias = 0.1 * torch.randn(G, generator=g)
    target = torch.randint(0, 2, (B, G), generator=g).float()
    return h, w, bias, target, CR.heads(h, w, bias, target)


@pytest.fixture(scope='module')
def heads_cases():
    cache = {}

    def get(G, B, H):
        if (G, B, H) not in cache:
            cache[(G, B, H)] = heads_inputs(G, B, H, 1000 * G + 10 * B + H)
        return cache[(G, B, H)]
    return get


def run_heads(h, w, bias, target, rows=None, target_rows=None):
    """``heads_bce_rows`` on device tensors (h [G, R, H] of any layout, w [G, 1, H]-like rows at stride w.stride(0)) into
    NaN-filled outputs: (rec, logits) [G, R]."""
    G, R = h.shape[0], h.shape[1]
    rec = torch.full((G, R), NAN, device=DEV)
    logits = torch.full((G, R), NAN, device=DEV)
    K.heads_bce_rows(h, w[0], w.stride(0), bias[:1], 1, target, rec, logits, target_rows=target_rows)
    return rec, logits


@pytest.mark.parametrize('H', [512, 516, 130, 5])
@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('G', [1, 3, 18])
def test_heads_bce_rows_matches_float64(G, B, H, heads_cases):
    """Bound 1e-5, max-normalised, the bound of the K20 / K24 kernel tests.  torch's own float32 evaluation of the same
    expression ((h * w).sum(-1) + bias, binary_cross_entropy_with_logits) against float64, on the CPU over 200 seeds of
    these shapes and this input distribution: worst 1.8e-7 for rec and 2.5e-7 for the logits -- the bound is 40x that."""
    h, w, bias, target, (logit64, rec64) = heads_cases(G, B, H)
    rec, logits = run_heads(h.to(DEV), w.to(DEV), bias.to(DEV), target.to(DEV))
    assert torch.isfinite(rec).all() and torch.isfinite(logits).all()
    close(rec, rec64, 'rec vs float64, G %d B %d H %d' % (G, B, H), 1e-5)
    close(logits, logit64, 'logits vs float64, G %d B %d H %d' % (G, B, H), 1e-5)


@pytest.mark.parametrize('variant', ['padded', 'offset', 'column_range'])
def test_heads_bce_rows_layouts(variant, heads_cases):
    """ldh = H + 4 with a padded group stride; h one float past an allocation (scalar loads although H % 4 == 0); the
    target as a column range of a wider matrix (ldt > G)."""
    G, B, H = 3, 3, 516
    h, w, bias, target, (logit64, rec64) = heads_cases(G, B, H)
    R = KT * B
    dh, dw, db, dt = h.to(DEV), w.to(DEV), bias.to(DEV), target.to(DEV)
    if variant == 'padded':
        buf = torch.full((G, R + 2, H + 4), NAN, device=DEV)
        dh = buf[:, :R, :H]
        dh.copy_(h)
        assert dh.stride() == ((R + 2) * (H + 4), H + 4, 1)
    elif variant == 'offset':
        buf = torch.empty(h.numel() + 1, device=DEV)
        dh = buf[1:].view(G, R, H)
        dh.copy_(h)
        assert dh.data_ptr() % 16 == 4
    else:
        wide = torch.full((B, 18), NAN, device=DEV)
        wide[:, 7:7 + G] = dt
        dt = wide[:, 7:7 + G]
        assert dt.stride(0) == 18
    rec, logits = run_heads(dh, dw, db, dt)
    close(rec, rec64, '%s: rec vs float64' % variant, 1e-5)
    close(logits, logit64, '%s: logits vs float64' % variant, 1e-5)


@pytest.mark.parametrize('H', [512, 130])
@pytest.mark.parametrize('G', [1, 18])
def test_heads_bce_rows_equals_the_composition_it_replaces(G, H, heads_cases):
    """The grouped N = 1 ``linear_fwd_grouped`` plus ``bce_elem_fwd``."""
    B = 3
    h, w, bias, target, _ = heads_cases(G, B, H)
    R = KT * B
    dh, dw, db, dt = h.to(DEV), w.to(DEV).view(G, 1, H), bias.to(DEV), target.to(DEV)
    rec, logits = run_heads(dh, dw, db, dt)
    pre = torch.full((G, R, 1), NAN, device=DEV)
    K.linear_fwd_grouped(dh, dw[0], H, db[:1], 1, pre, None)
    old = torch.full((G, R), NAN, device=DEV)
    K.bce_elem_fwd(pre.view(-1), dt.t().unsqueeze(1).expand(G, KT, B).reshape(-1).contiguous(), old.view(-1))
    close(logits, pre.view(G, R), 'logits vs linear_fwd_grouped', 1e-6)
    close(rec, old, 'rec vs linear_fwd_grouped + bce_elem_fwd', 1e-6)


@pytest.mark.parametrize('H', [512, 130])
def test_heads_bce_rows_is_deterministic_and_independent_of_the_row_count(H, heads_cases):
    G, B = 18, 3
    h, w, bias, target, _ = heads_cases(G, B, H)
    dh, dw, db, dt = h.to(DEV), w.to(DEV), bias.to(DEV), target.to(DEV)
    rec, logits = run_heads(dh, dw, db, dt)
    rec2, logits2 = run_heads(dh, dw, db, dt)
    assert torch.equal(rec, rec2) and torch.equal(logits, logits2), 'two identical calls gave different bits'
    few = 5 * B                                                             # the first 5 samples alone: another grid
    rec3, logits3 = run_heads(dh[:, :few], dw, db, dt)
    assert torch.equal(rec3, rec[:, :few]) and torch.equal(logits3, logits[:, :few]), 'a row depends on R'


# ----------------------------------------------------------------------------- iw_fold_rows
def fold_inputs(n_rows, B, seed):
    g = torch.Generator().manual_seed(seed)
    lw = -80 + 5 * torch.randn(KT, B, generator=g)
    rec = 0.05 + 2.95 * torch.rand(n_rows, KT * B, generator=g)
    return lw, rec


def fold(lw, rec, sel, chunk):
    """Fold lw [K, B] and the rows of rec [rows, K * B] in chunks of ``chunk`` samples (a chunk's rows are a column range
    of rec: rec_ss > Kc * B whenever there is more than one chunk): (out [S + 1, B], state [S + 1, B, 2])."""
    Kt, B = lw.shape
    S = rec.shape[0] if sel is None else len(sel)
    state = fresh_state(S + 1, B, DEV)
    out = torch.full((S + 1, B), NAN, device=DEV)
    for k0 in range(0, Kt, chunk):
        k1 = min(Kt, k0 + chunk)
        K.iw_fold_rows(lw[k0:k1], rec[:, k0 * B:k1 * B], sel, state, out, finish_k=Kt if k1 == Kt else 0)
    return out, state


@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('S', [1, 2, 19, 64])
def test_fold_rows_matches_float64_in_one_chunk_and_in_ragged_chunks(S, B):
    lw, rec = fold_inputs(S, B, 100 * S + B)
    _, ref = CR.fold(lw, rec)
    one, s_one = fold(lw.to(DEV), rec.to(DEV), None, KT)
    ragged, _ = fold(lw.to(DEV), rec.to(DEV), None, 3)                    # 22 chunks of 3 and a last chunk of 1
    assert torch.isfinite(one).all() and torch.isfinite(ragged).all()
    close_per_state(one, ref, 'one chunk vs float64', 1e-5)
    close_per_state(ragged, ref, 'chunks of 3 vs float64', 1e-5)
    close_per_state(ragged, one, 'chunks of 3 vs one chunk', 1e-6)
    if S == 1:
        assert torch.equal(one[0], one[1]) and torch.equal(s_one[0], s_one[1]), 'S = 1: state 0 and state 1 differ'


@pytest.mark.parametrize('B', [1, 3, 17])
def test_fold_rows_with_a_selection_that_skips_and_reorders(B):
    lw, rec = fold_inputs(8, B, 800 + B)
    sel = [5, 0, 3]
    _, ref = CR.fold(lw, rec, sel)
    for chunk in (KT, 3):
        out, _ = fold(lw.to(DEV), rec.to(DEV), sel, chunk)
        close_per_state(out, ref, 'sel %s, chunk %d vs float64' % (sel, chunk), 1e-5)
    # one selected row alone: the marginal and the joint are the same bits
    out, state = fold(lw.to(DEV), rec.to(DEV), [6], KT)
    assert torch.equal(out[0], out[1]) and torch.equal(state[0], state[1])
    close(out[0], CR.fold(lw, rec, [6])[1][0], 'sel [6] vs float64', 1e-5)


def accumulate(lw, terms):
    B = lw.shape[1]
    state = fresh_state(1, B, DEV)[0]
    out = torch.full((B,), NAN, device=DEV)
    K.iw_accumulate(lw, terms, state, out, finish_k=lw.shape[0])
    return out


@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('S', [1, 2, 19, 64])
def test_fold_rows_equals_iw_accumulate_on_the_same_rows(S, B):
    lw, rec = fold_inputs(S, B, 100 * S + B)
    lw, rec = lw.to(DEV), rec.to(DEV)
    out, _ = fold(lw, rec, None, KT)
    for s in range(S):
        close(out[s], accumulate(lw, [(rec[s], 1)]), 'state %d vs iw_accumulate' % s, 1e-6)
    close(out[S], accumulate(lw, [(rec.t().contiguous(), S)]), 'joint vs iw_accumulate on the [R, S] copy', 1e-6)


def test_fold_rows_first_chunk_from_the_empty_state_is_not_nan():
    g = torch.Generator().manual_seed(5)
    lw = torch.tensor([[-2.0, float('-inf')], [-1.0, float('-inf')]])
    rec = 3 * torch.rand(3, 4, generator=g)
    _, ref = CR.fold(lw, rec)
    out, state = fold(lw.to(DEV), rec.to(DEV), None, 1)
    assert not torch.isnan(state).any() and not torch.isnan(out).any()
    close_per_state(out[:, :1], ref[:, :1], 'finite column', 1e-6)
    assert (out[:, 1] == float('-inf')).all()                  # no mass at all: log 0, not NaN


@pytest.mark.parametrize('B', [1, 3])
def test_fold_rows_celeba19_magnitudes(B):
    """The CelebA-19 shapes: an image row near 7000 +- 300, 18 attribute rows in [0.05, 3], density ratios spread by
    +-300 (around -500: the attribute marginals' log-weights are the ratio less a term below 3) -- exp() of any
    log-weight alone is 0 in fp32."""
    g = torch.Generator().manual_seed(190 + B)
    lw = -500 + 100 * torch.randn(KT, B, generator=g).clamp(-3, 3)
    rec = torch.cat([7000 + 300 * (2 * torch.rand(1, KT * B, generator=g) - 1),
                     0.05 + 2.95 * torch.rand(18, KT * B, generator=g)])
    logw, ref = CR.fold(lw, rec)
    assert 6700 <= rec[0].min() and rec[0].max() <= 7300 and rec[0].max() - rec[0].min() > 300
    assert lw.max() - lw.min() > 300 and (torch.exp(logw.float()) == 0).all()
    for chunk in (KT, 3):
        out, state = fold(lw.to(DEV), rec.to(DEV), None, chunk)
        assert torch.isfinite(out).all() and torch.isfinite(state).all()
        close_per_state(out, ref, 'chunk %d' % chunk, 1e-5)


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def pair():
    o, image, attrs, eps = CR.celeba19_pair()
    model = CM.MVAE(CR.E2E_D)
    model.load_state_dict(o.state_dict(), strict=True)
    model.to(DEV)
    model.train()                                               # log_likelihood switches to eval() itself
    refs = {}

    def ref(case):
        if case not in refs:
            refs[case] = CR.celeba19_case(o, image, attrs, eps, *CR.E2E_CASES[case])
        return refs[case]
    return model, image, attrs, eps, ref


def call(model, image, attrs, eps, case, **kw):
    """``log_likelihood`` for E2E case ``case``, handed only the data the case uses."""
    score, given = CR.E2E_CASES[case]
    used = CR.expand(score) + CR.expand(given)
    return CL.log_likelihood(model, image if 'image' in used else None, attrs if len(set(used) - {'image'}) else None,
                             score=score, given=given, n_samples=CR.E2E_K, eps=eps, **kw)


@pytest.mark.parametrize('case', range(len(CR.E2E_CASES)))
def test_log_likelihood_matches_restatement(case, pair):
    model, image, attrs, eps, ref = pair
    want = ref(case)
    score = CR.expand(CR.E2E_CASES[case][0])
    assert list(want) == list(score) + ['joint']
    for path in CL.PATHS:
        got = call(model, image, attrs, eps, case, chunk_rows=6, per_modality=True, path=path)   # chunks of 2, 2, 1
        assert list(got) == list(want), (list(got), list(want))
        for name in want:
            assert got[name].shape == (CR.E2E_B,) and got[name].is_cuda and got[name].dtype == torch.float32
            close(got[name], want[name], 'case %d, path %s, %s' % (case, path, name), REL_TOL)
        joint = call(model, image, attrs, eps, case, chunk_rows=6, path=path)
        assert torch.equal(joint, got['joint']), 'the default return is not the joint of per_modality=True'


@pytest.mark.parametrize('path', CL.PATHS)
def test_log_likelihood_does_not_depend_on_the_chunking(path, pair):
    model, image, attrs, eps, _ = pair
    outs = [call(model, image, attrs, eps, 0, chunk_rows=rows, per_modality=True, path=path) for rows in (3, 6, 15, 4096)]
    for o in outs[1:]:
        for name in outs[0]:
            close(o[name], outs[0][name], 'chunk_rows, %s, %s' % (path, name), 1e-6)


@pytest.mark.parametrize('case', [0, 3])
def test_log_likelihood_fused_equals_rows(case, pair):
    model, image, attrs, eps, _ = pair
    a = call(model, image, attrs, eps, case, chunk_rows=6, per_modality=True, path='fused')
    b = call(model, image, attrs, eps, case, chunk_rows=6, per_modality=True, path='rows')
    for name in b:
        close(a[name], b[name], 'fused vs rows, case %d, %s' % (case, name), 1e-5)


@pytest.mark.parametrize('path', CL.PATHS)
def test_log_likelihood_device_noise_and_model_state(path, pair):
    model, image, attrs, _, _ = pair
    model.train()
    model.image_decoder.eval()                                  # a mixed state must come back as it was
    modes = [m.training for m in model.modules()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = CL.log_likelihood(model, image, attrs, n_samples=9, chunk_rows=12, seed=7, path=path)
    b = CL.log_likelihood(model, image, attrs, n_samples=9, chunk_rows=12, seed=7, path=path)
    c = CL.log_likelihood(model, image, attrs, n_samples=9, chunk_rows=12, seed=8, path=path)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), 'the same seed gave different bits'
    assert not torch.equal(a, c), 'different seeds gave the same estimate'
    assert [m.training for m in model.modules()] == modes and model.training
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), '%s changed' % k
    model.train()


@pytest.mark.parametrize('path', CL.PATHS)
def test_log_likelihood_of_one_attribute_does_not_run_the_image_decoder(path, pair):
    model, image, attrs, eps, ref = pair
    calls = {'decoder': 0, 'encoder': 0}
    hooks = [model.image_decoder.register_forward_hook(lambda *a: calls.__setitem__('decoder', calls['decoder'] + 1)),
             model.image_encoder.register_forward_hook(lambda *a: calls.__setitem__('encoder', calls['encoder'] + 1))]
    try:
        got = call(model, image, attrs, eps, 4, chunk_rows=6, per_modality=True, path=path)
        assert calls == {'decoder': 0, 'encoder': 0}, calls
        call(model, image, attrs, eps, 1, chunk_rows=6, path=path)          # the hook does count: 3 chunks of the image
        assert calls['decoder'] == 3, calls
    finally:
        for h in hooks:
            h.remove()
    assert list(got) == ['Male', 'joint'] and torch.equal(got['Male'], got['joint'])      # S = 1


def test_celeba19_loglike_cli(tmp_path):
    model = CM.MVAE(16)
    path = os.path.join(str(tmp_path), 'model_best.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'n_latents': 16}, path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'multimodal-vae-public_amd', 'celeba19', 'loglike.py'), path,
                          '--synthetic', '--cuda', '--n-samples', '4', '--batch-size', '2', '--per-modality'],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    names = re.findall(r'log p\(([^ ]+) \|', out.stdout)
    assert names[:19] == list(CL.MODALITIES) and len(names) == 20, out.stdout
    means = re.findall(r'mean (-?[0-9.]+(?:e[-+]?\d+)?|nan|-?inf)', out.stdout)
    assert len(means) == 20, out.stdout
    for m in means:
        v = float(m)
        assert v == v and abs(v) != float('inf') and v < 0, out.stdout
