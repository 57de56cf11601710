"""GPU: the two kernels of csrc/predict.hip against the float64 restatement (tests/predict_ref.py) on the same inputs, and
``predict`` / ``evaluate`` end to end for the five kinds against the restatement run on the logits of plain module calls
on the same z; the command-line drop-ins against ``evaluate``."""
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

import mvae_amd
from mvae_amd import kernels as K
import predict_ref as PR
from util import REL_TOL, rel_err

P = importlib.import_module('mvae_amd.predict')
pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The fold's bound (see test_fold_matches_float64): 1e-5 where it is at least ten times the fp32 error of the reference's
# own evaluation, ten times that error otherwise.
FOLD_TOL = {'categorical': 1e-5, 'bernoulli': 1.023e-5}


def close(a, b, what, tol):
    e = rel_err(a, b)
    print('%s: relative error %.3e (bound %.3e)' % (what, e, tol))
    assert e <= tol, '%s: relative error %.3e > %.3e' % (what, e, tol)


# ----------------------------------------------------------------------------- mvae_predict_fold
def run_fold(logits, B, mode, chunk=None, gr_layout=False):
    """Fold host ``logits`` [Kt * B, C] in chunks of ``chunk`` samples (default: one chunk) -> (out, state) on the
    device.  ``gr_layout`` stores each chunk as [C, R] and passes its transpose: row stride 1, column stride R."""
    R, C = logits.shape
    Kt = R // B
    chunk = chunk or Kt
    state = K.fresh_predict_state(B, C, mode, DEV)
    out = torch.full((B, C) if mode == 'categorical' else (B, C, 2), float('nan'), device=DEV)
    for k0 in range(0, Kt, chunk):
        k1 = min(Kt, k0 + chunk)
        part = logits[k0 * B:k1 * B].to(DEV)
        if gr_layout:
            part = part.t().contiguous().t()
            assert part.stride() == (1, (k1 - k0) * B) or C == 1
        else:
            part = part.contiguous()
        K.predict_fold(part, B, mode, state, out, finish_k=Kt if k1 == Kt else 0)
    return out, state


FOLD_CASES = [('categorical', s, False) for s in PR.FOLD_SHAPES_CAT] + [('bernoulli', PR.FOLD_SHAPE_BERN, False),
                                                                        ('bernoulli', PR.FOLD_SHAPE_BERN_GR, True)]


@pytest.mark.parametrize('scale', PR.SCALES)
@pytest.mark.parametrize('mode,shape,gr', FOLD_CASES)
def test_fold_matches_float64(mode, shape, gr, scale):
    """Against float64 with util.rel_err.  The reference's own fp32 evaluation of the same formulas (predict_ref with
    dtype=float32, on the CPU) errs over 200 seeds of each of these shapes, at both scales, by at most 1.9e-7 in
    categorical mode -- the 1e-5 of test_loglike_gpu.py's streaming merge stands -- and by at most 1.023e-6 in Bernoulli
    mode (torch's fp32 softplus), of which 1e-5 is not ten times: that mode's bound is ten times the figure, 1.023e-5.
    Chunks of 3 samples (ragged) agree with one chunk to 1e-6, and two runs give the same bits."""
    Kc, B, C = shape
    logits = PR.fold_inputs(Kc, B, C, scale)
    ref = PR.fold(logits, B, mode)
    one, state = run_fold(logits, B, mode, gr_layout=gr)
    again, state2 = run_fold(logits, B, mode, gr_layout=gr)
    ragged, _ = run_fold(logits, B, mode, chunk=3, gr_layout=gr)
    assert torch.isfinite(one).all() and torch.isfinite(state).all()
    close(one, ref, 'one chunk vs float64', FOLD_TOL[mode])
    close(ragged, ref, 'chunks of 3 vs float64', FOLD_TOL[mode])
    close(ragged, one, 'chunks of 3 vs one chunk', 1e-6)
    assert torch.equal(one, again) and torch.equal(state, state2), 'two runs gave different bits'
    if mode == 'categorical':
        close(one.double().exp().sum(1), torch.ones(B, dtype=torch.float64), 'rows of exp(logp)', 1e-5)


@pytest.mark.parametrize('mode', ['categorical', 'bernoulli'])
def test_fold_of_one_sample_is_the_log_probability_itself(mode):
    x = PR.fold_inputs(1, 5, 13, 30.0)
    out, _ = run_fold(x, 5, mode)
    if mode == 'categorical':
        want = torch.log_softmax(x.double(), dim=1)
    else:
        want = torch.stack((-torch.nn.functional.softplus(-x.double()), -torch.nn.functional.softplus(x.double())), dim=2)
    close(out, want, 'Kc = 1, finish_k = 1', 1e-6)


def test_fold_value_of_a_datum_does_not_depend_on_the_batch():
    logits = PR.fold_inputs(65, 3, 13, 1.0)
    full, _ = run_fold(logits, 3, 'categorical')
    alone, _ = run_fold(logits.view(65, 3, 13)[:, 1].contiguous(), 1, 'categorical')
    assert torch.equal(full[1], alone[0])


@pytest.mark.parametrize('mode', ['categorical', 'bernoulli'])
def test_fold_edge_cases(mode):
    """A column of -inf logits gives -inf (log 0) and no NaN anywhere; a logit of +80 in one column stays finite."""
    Kc, B, C = 5, 3, 6
    x = PR.fold_inputs(Kc, B, C, 1.0)
    x[:, 2] = float('-inf')
    for chunk in (Kc, 2):
        out, state = run_fold(x, B, mode, chunk=chunk)
        assert not torch.isnan(out).any() and not torch.isnan(state).any()
        if mode == 'categorical':
            assert (out[:, 2] == float('-inf')).all()
            keep = [0, 1, 3, 4, 5]
            close(out[:, keep], PR.fold_categorical(x[:, keep], B), 'the finite columns', 1e-5)
        else:
            assert (out[:, 2, 0] == float('-inf')).all() and (out[:, 2, 1] == 0).all()
            close(out[:, [0, 1, 3]], PR.fold_bernoulli(x[:, [0, 1, 3]], B), 'the finite columns', FOLD_TOL[mode])
    y = PR.fold_inputs(Kc, B, C, 1.0)
    y[:, 4] = 80.0
    out, state = run_fold(y, B, mode, chunk=2)
    assert torch.isfinite(out).all() and torch.isfinite(state).all()
    close(out, PR.fold(y, B, mode), 'a logit of +80', FOLD_TOL[mode])


# ----------------------------------------------------------------------------- mvae_predict_score
def run_score(logp, mode, y, confusion=None):
    shape = (logp.shape[0],) if mode == 'categorical' else tuple(logp.shape[:2])
    pred = torch.full(shape, -7, dtype=torch.int64, device=DEV)
    nll = torch.full(shape, float('nan'), device=DEV)
    correct = torch.full(shape, 9, dtype=torch.uint8, device=DEV)
    K.predict_score(logp, mode, pred, targets=y, nll=nll, correct=correct, confusion=confusion)
    return pred, nll, correct


@pytest.mark.parametrize('B,mode', [(1, 'categorical'), (7, 'categorical'), (300, 'categorical'), (7, 'bernoulli'),
                                    (300, 'bernoulli')])
def test_score_matches_restatement(B, mode):
    logits, y, ref_logp = PR.score_case(B, mode)
    assert PR.margin(ref_logp, mode).min().item() > PR.MARGIN
    C = logits.shape[1]
    logp, _ = run_fold(logits, B, mode)
    score = PR.score_categorical if mode == 'categorical' else PR.score_bernoulli
    r_pred, r_nll, r_correct, r_conf = score(ref_logp, y if mode == 'categorical' else y.double())
    conf = torch.zeros((C, C) if mode == 'categorical' else (C, 2, 2), dtype=torch.int64, device=DEV)
    if mode == 'categorical':
        y_dev = y.to(DEV)
    else:                                               # a column range of a wider matrix: row stride C + 5
        wide = torch.full((B, C + 5), 0.5, device=DEV)
        wide[:, 2:2 + C] = y.to(DEV)
        y_dev = wide[:, 2:2 + C]
        assert y_dev.stride(0) == C + 5
    pred, nll, correct = run_score(logp, mode, y_dev, conf)
    assert torch.equal(pred.cpu(), r_pred) and torch.equal(correct.cpu().bool(), r_correct)
    assert torch.equal(conf.cpu(), r_conf) and conf.sum().item() == B * (1 if mode == 'categorical' else C)
    close(nll, r_nll, 'nll', 1e-6)
    run_score(logp, mode, y_dev, conf)                  # a second call into the same table: the sum of the two
    assert torch.equal(conf.cpu(), 2 * r_conf)
    only = torch.full_like(pred, -7)
    K.predict_score(logp, mode, only)                   # predictions alone
    assert torch.equal(only, pred)


def test_score_counts_an_out_of_range_target_nowhere():
    logits, y, ref_logp = PR.score_case(7, 'categorical')
    y = y.clone()
    y[1], y[4], y[6] = 10, -1, 1 << 40
    logp, _ = run_fold(logits, 7, 'categorical')
    guard = torch.zeros(3, 10, 10, dtype=torch.int64, device=DEV)       # the table in the middle of two guard tables
    pred, nll, correct = run_score(logp, 'categorical', y.to(DEV), guard[1])
    r_pred, r_nll, r_correct, r_conf = PR.score_categorical(ref_logp, y)
    assert torch.equal(guard[1].cpu(), r_conf) and guard[1].sum().item() == 4
    assert guard[0].sum().item() == 0 and guard[2].sum().item() == 0
    assert torch.equal(pred.cpu(), r_pred) and torch.equal(correct.cpu().bool(), r_correct)
    assert torch.isinf(nll[[1, 4, 6]]).all() and (nll[[1, 4, 6]] > 0).all() and (correct[[1, 4, 6]] == 0).all()
    close(nll[[0, 2, 3, 5]], r_nll[[0, 2, 3, 5]], 'nll of the valid targets', 1e-6)
    logits, yb, ref_b = PR.score_case(7, 'bernoulli')
    yb = yb.clone()
    yb[2, 3], yb[5, 17] = 2.0, -1.0
    logp, _ = run_fold(logits, 7, 'bernoulli')
    guard = torch.zeros(3, 18, 2, 2, dtype=torch.int64, device=DEV)
    pred, nll, correct = run_score(logp, 'bernoulli', yb.to(DEV), guard[1])
    r_pred, r_nll, r_correct, r_conf = PR.score_bernoulli(ref_b, yb.double())
    assert torch.equal(guard[1].cpu(), r_conf) and guard[1].sum().item() == 7 * 18 - 2
    assert guard[0].sum().item() == 0 and guard[2].sum().item() == 0
    assert torch.isinf(nll[2, 3]) and torch.isinf(nll[5, 17]) and correct[2, 3] == 0 and correct[5, 17] == 0
    assert torch.equal(correct.cpu().bool(), r_correct)


# ----------------------------------------------------------------------------- end to end
KINDS = ['mnist', 'fashionmnist', 'celeba', 'celeba19', 'multimnist']
N_LATENTS = {'mnist': 64, 'fashionmnist': 64, 'multimnist': 64, 'celeba': 100, 'celeba19': 100}
K_SAMPLES = 7


def last_label_weights(model, kind):
    """The weight of the last Linear of every label decoder."""
    if kind == 'multimnist':
        return [model.text_decoder.h2o.weight]
    decoders = list(model.attr_decoders) if kind == 'celeba19' else [model.label_decoder]
    return [[m.weight for m in d.modules() if getattr(m, 'weight', None) is not None and m.weight.dim() == 2][-1]
            for d in decoders]


def make_case(kind):
    """A default-size model at its random initialisation with the label decoder's last weight times 20 (the logits
    spread), B data and replayed noise."""
    torch.manual_seed(410 + KINDS.index(kind))
    mod = importlib.import_module('mvae_amd.%s.model' % kind)
    model = mod.MVAE(N_LATENTS[kind])
    with torch.no_grad():
        for w in last_label_weights(model, kind):
            w.mul_(20.0)
    model.to(DEV).train()
    B = 3 if kind in ('multimnist', 'celeba19') else 5
    from mvae_amd.loglike import synthetic_data
    image, label = synthetic_data('celeba' if kind == 'celeba19' else kind, B, seed=77)
    eps = torch.randn(K_SAMPLES, B, N_LATENTS[kind], generator=torch.Generator().manual_seed(78))
    return model, image, label, eps


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = make_case(kind)
        return cache[kind]
    return get


def module_logits(model, kind, zr):
    """The label logits of plain module calls on the rows ``zr`` -> host [rows (x 4), C]."""
    if kind == 'celeba19':
        return torch.cat([d(zr) for d in model.attr_decoders], dim=1).cpu()
    if kind == 'multimnist':
        words = model.text_decoder(zr)
        return words.reshape(zr.shape[0] * 4, -1).cpu()
    return model.label_decoder(zr).cpu()


def restate(model, kind, image, label, eps, n_samples, chunk, given=('image',)):
    """The restatement on the logits of plain module calls on the same z, chunk by chunk as ``predict`` cuts them."""
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            img = image.to(DEV) if 'image' in given else None
            if kind == 'celeba19':
                from mvae_amd.celeba19 import loglike as C19
                mu, lv = C19.infer(model, img, label.to(DEV).float() if label is not None else None, given)
            else:
                mu, lv = model.infer(img)
            mu, lv = mu.contiguous(), lv.contiguous()
            B, D = mu.shape
            if n_samples == 0:
                logits = module_logits(model, kind, mu)
            else:
                z = torch.empty(n_samples, B, D, device=DEV)
                K.iw_draw(mu, lv, z, torch.empty(n_samples, B, device=DEV), eps=eps.to(DEV).contiguous())
                parts = [module_logits(model, kind, z[k0:k0 + chunk].reshape(-1, D)) for k0 in range(0, n_samples, chunk)]
                logits = torch.cat(parts)
    finally:
        for m, t in modes:
            m.training = t
    per = 4 if kind == 'multimnist' else 1
    return PR.fold(logits, B * per, P.MODES[kind]), mu


@pytest.mark.parametrize('n_samples', [0, K_SAMPLES])
@pytest.mark.parametrize('kind', KINDS)
def test_evaluate_matches_restatement(kind, n_samples, cases):
    model, image, label, eps = cases(kind)
    B = image.shape[0]
    mode = P.MODES[kind]
    before = [m.training for m in model.modules()]
    kw = dict(n_samples=n_samples, chunk_rows=2 * B, eps=eps if n_samples else None)    # chunks of 2, 2, 2 and 1 samples
    res = P.evaluate(model, image, label, **kw)
    fed = model.text_decoder.last_fed.cpu() if kind == 'multimnist' else None
    assert [m.training for m in model.modules()] == before and model.training
    only = P.predict(model, image, **kw)
    assert torch.equal(only['logp'], res['logp']) and torch.equal(only['pred'], res['pred'])
    ref, mu = restate(model, kind, image, label, eps, n_samples, 2)
    if mode == 'bernoulli':
        got = torch.stack((res['logp'], res['logp0']), dim=2)
        y = label.double()
        r_pred, r_nll, r_correct, r_conf = PR.score_bernoulli(ref, y)
    else:
        got = res['logp'].reshape(ref.shape)
        y = label.reshape(-1)
        r_pred, r_nll, r_correct, r_conf = PR.score_categorical(ref, y)
    assert all(v.is_cuda for v in res.values() if torch.is_tensor(v))
    close(got, ref, '%s K = %d logp' % (kind, n_samples), REL_TOL)
    safe = PR.margin(ref, mode) > PR.MARGIN
    assert safe.double().mean().item() >= 0.9, 'more than 10%% of the data have a margin below %.0e' % PR.MARGIN
    pred, correct = res['pred'].cpu().reshape(r_pred.shape), res['correct'].cpu().reshape(r_pred.shape).bool()
    assert torch.equal(pred[safe], r_pred[safe]) and torch.equal(correct[safe], r_correct[safe])
    close(res['nll'].reshape(r_nll.shape), r_nll, '%s nll' % kind, REL_TOL)
    if safe.all():
        assert torch.equal(res['confusion'].cpu(), r_conf)
    assert res['confusion'].sum().item() == r_pred.numel()
    if kind == 'mnist' and n_samples == 0:
        model.eval()
        with torch.no_grad():
            want = torch.log_softmax(model.text_decoder(mu), dim=1)
        model.train()
        close(res['logp'], want, 'log_softmax(text_decoder(mu))', 1e-6)
    if kind == 'multimnist':
        assert res['logp'].shape == (B, 4, 12) and res['pred'].shape == (B, 4) and len(res['strings']) == B
        from mvae_amd.multimnist.utils import tensor_to_string
        assert list(res['strings']) == [tensor_to_string(res['pred'][i].cpu()) for i in range(B)]
        hit = (res['pred'].cpu() == label)
        assert torch.equal(res['position_accuracy'].cpu(), hit.float().mean(0))
        assert res['exact_match'].item() == hit.all(1).float().mean().item()
        if n_samples == 0:                              # the characters the greedy decoder fed back: SOS, then its arg-max
            assert fed.shape == (4, B) and torch.equal(res['pred'].cpu()[:, :3], fed[1:].t())


def test_celeba19_given_image_and_an_attribute(cases):
    model, image, label, eps = cases('celeba19')
    given = ('image', 'Male')
    res = P.evaluate(model, image, label, given=given, n_samples=K_SAMPLES, chunk_rows=2 * image.shape[0], eps=eps)
    ref, _ = restate(model, 'celeba19', image, label, eps, K_SAMPLES, 2, given=given)
    close(torch.stack((res['logp'], res['logp0']), dim=2), ref, 'celeba19 given image + Male', REL_TOL)
    plain = P.predict(model, image, n_samples=K_SAMPLES, chunk_rows=2 * image.shape[0], eps=eps)
    assert not torch.equal(plain['logp'], res['logp']), 'the given attribute changed nothing'
    assert res['pred'].shape == (image.shape[0], 18)


def test_device_noise(cases):
    model, image, _, _ = cases('mnist')
    a = P.predict(model, image, n_samples=9, chunk_rows=10, seed=7)
    b = P.predict(model, image, n_samples=9, chunk_rows=10, seed=7)
    c = P.predict(model, image, n_samples=9, chunk_rows=10, seed=8)
    assert torch.isfinite(a['logp']).all()
    assert torch.equal(a['logp'], b['logp']), 'the same seed gave different bits'
    assert not torch.equal(a['logp'], c['logp']), 'different seeds gave the same bits'


# ----------------------------------------------------------------------------- the command line
@pytest.mark.parametrize('kind', ['mnist', 'celeba19'])
def test_predict_cli(kind, tmp_path):
    d = 16
    torch.manual_seed(5)
    model = importlib.import_module('mvae_amd.%s.model' % kind).MVAE(d)
    path = os.path.join(str(tmp_path), 'model_best.pth.tar')
    torch.save({'state_dict': model.state_dict(), 'n_latents': d}, path)
    n = 6
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'multimodal-vae-public_amd', kind, 'predict.py'), path,
                          '--synthetic', '--cuda', '--n-samples', '4', '--batch-size', str(n), '--n-data', str(n),
                          '--seed', '3', '--out-dir', os.path.join(str(tmp_path), 'out')],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    text = open(os.path.join(str(tmp_path), 'out', 'predict.txt')).read()
    assert text.strip() in out.stdout
    m = re.search(r'^accuracy ([0-9.]+)$', text, flags=re.M)
    assert m, text
    from mvae_amd.loglike import synthetic_data
    image, label = synthetic_data('celeba' if kind == 'celeba19' else kind, n, 3)
    model.to(DEV)
    res = P.evaluate(model, image, label, n_samples=4, seed=3)
    assert abs(float(m.group(1)) - res['correct'].double().mean().item()) < 5e-7, text
    if kind == 'celeba19':
        assert len(re.findall(r'accuracy [0-9.]+  majority [0-9.]+', text)) == 18 and 'Male' in text
    else:
        assert 'confusion' in text and 'nll mean' in text
