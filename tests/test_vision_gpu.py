"""GPU parity of the vision experiment (vision/model.py, vision/train.py): the HIP stacks, the eager seven-call
``train_step`` and the batched ``fused_step`` against the live plain-torch restatement (tests/vision_ref.py, whose stacks
the golden generator proves equal to the reference's text) and against tests/golden/vision_b4.npz, forward and backward,
with every noise draw replayed.  Bar: util.REL_TOL (1e-4 of max |ref|) on outputs, terms, every gradient and the
BatchNorm running statistics; ``num_batches_tracked`` exact."""
import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd.vision import model as VM, train as VT
from oracle import models as OM
import vision_ref as R
from util import assert_close, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
D = 16


def pair(ref_cls, hip_cls, seed, n_latents=D, channels=3, train=True):
    o = OM.fill_parameters(ref_cls(n_latents, channels), seed)
    m = hip_cls(n_latents, channels)
    m.load_state_dict(o.state_dict(), strict=True)
    m.to(DEV)
    o.train(train); m.train(train)
    return o, m


def compare_params_and_buffers(o, m, what):
    worst = 0.0
    for (name, q), (n2, p) in zip(o.named_parameters(), m.named_parameters()):
        assert name == n2
        worst = max(worst, assert_close(p.grad, q.grad, '%s grad %s' % (what, name)))
    for (name, b), (n2, b2) in zip(o.state_dict().items(), m.state_dict().items()):
        assert name == n2
        if name.endswith('num_batches_tracked'):
            assert int(b) == int(b2), '%s %s: %d vs %d' % (what, name, int(b2), int(b))
        elif 'running_' in name:
            assert_close(b2, b, '%s buffer %s' % (what, name))
    return worst


def encoder_case(channels, batch, n_latents=D):
    o, m = pair(R.ImageEncoder, VM.ImageEncoder, 51, n_latents, channels)
    g = torch.Generator().manual_seed(52 + batch + channels)
    x = torch.rand(batch, channels, 64, 64, generator=g)
    mask = torch.empty(batch, 512).bernoulli_(0.9, generator=g)
    w = torch.randn(batch, 2 * n_latents, generator=g)
    mu, lv = o(x, mask)
    (torch.cat((mu, lv), dim=1) * w).sum().backward()
    hmu, hlv = m(x.to(DEV), mask.to(DEV))
    (torch.cat((hmu, hlv), dim=1) * w.to(DEV)).sum().backward()
    assert_close(hmu, mu.detach(), 'mu'); assert_close(hlv, lv.detach(), 'logvar')
    return compare_params_and_buffers(o, m, 'encoder')


def decoder_case(channels, batch, n_latents=D):
    o, m = pair(R.ImageDecoder, VM.ImageDecoder, 53, n_latents, channels)
    g = torch.Generator().manual_seed(54 + batch + channels)
    z = torch.randn(batch, n_latents, generator=g)
    w = torch.randn(batch, channels, 64, 64, generator=g)
    zo = z.clone().requires_grad_()
    out = o(zo)
    (out * w).sum().backward()
    zh = z.to(DEV).requires_grad_()
    got = m(zh)
    assert got.shape == (batch, channels, 64, 64)
    (got * w.to(DEV)).sum().backward()
    assert_close(got, out.detach(), 'logits'); assert_close(zh.grad, zo.grad, 'd z')
    return compare_params_and_buffers(o, m, 'decoder')


@pytest.mark.parametrize('batch', [1, 5])
@pytest.mark.parametrize('channels', [1, 3])
def test_image_stacks_training_match_restatement(channels, batch):
    print('C=%d B=%d: worst gradient rel err encoder %.2e, decoder %.2e' % (
        channels, batch, encoder_case(channels, batch), decoder_case(channels, batch)))


def test_gray_stacks_at_the_default_latent_size():
    """D = 250: the K = 250 Linear routes are the scalar-loader ones (250 % 4 != 0)."""
    print('C=1 B=2 D=250: worst gradient rel err encoder %.2e, decoder %.2e' % (
        encoder_case(1, 2, 250), decoder_case(1, 2, 250)))


@pytest.mark.parametrize('channels', [1, 3])
def test_image_stacks_eval_mode_after_one_training_pass(channels):
    g = torch.Generator().manual_seed(55 + channels)
    oe, me = pair(R.ImageEncoder, VM.ImageEncoder, 51, D, channels)
    od, md = pair(R.ImageDecoder, VM.ImageDecoder, 53, D, channels)
    x = torch.rand(3, channels, 64, 64, generator=g)
    mask, z = torch.empty(3, 512).bernoulli_(0.9, generator=g), torch.randn(3, D, generator=g)
    with torch.no_grad():
        oe(x, mask); me(x.to(DEV), mask.to(DEV)); od(z); md(z.to(DEV))      # advance the running statistics
        for mod in (oe, me, od, md):
            mod.eval()
        mu, lv = oe(x)
        hmu, hlv = me(x.to(DEV))
        assert_close(hmu, mu, 'eval mu'); assert_close(hlv, lv, 'eval logvar')
        assert_close(md(z.to(DEV)), od(z), 'eval logits')


# ----------------------------------------------------------------------------- the seven-term step
def models(seed, train=True):
    o = OM.fill_parameters(R.MVAE(D), seed)
    m = VM.MVAE(D)
    m.load_state_dict(o.state_dict(), strict=True)
    m.to(DEV)
    o.train(train); m.train(train)
    return o, m


def to_dev(noise):
    return [{'eps': n['eps'].to(DEV), 'masks': [None if k is None else k.to(DEV) for k in n['masks']]} for n in noise]


def snapshot(m, total, terms):
    sd = m.state_dict()             # flushes the BatchNorm counters
    return {'total': float(total), 'terms': terms.detach().double().cpu(),
            'grads': {n: p.grad.detach().clone() for n, p in m.named_parameters()},
            'buffers': {k: v.detach().clone() for k, v in sd.items() if 'running_' in k or k.endswith('num_batches_tracked')}}


@pytest.fixture(scope='module')
def step3():
    """One step at B = 3 on the same weights, batch and noise, three ways: restatement (CPU), eager, fused."""
    B, beta = 3, 0.5
    o, m_eager = models(61)
    _, m_fused = models(61)
    batch6 = R.synthetic_batch(B, 62)
    noise = R.draw_step_noise(B, D, torch.Generator().manual_seed(63))
    o_total, o_terms, _ = R.seven_term_step(o, batch6, noise, beta)
    o_total.backward()
    dev6 = tuple(x.to(DEV) for x in batch6)
    eager = snapshot(m_eager, *VT.train_step(m_eager, None, dev6, beta, noise=to_dev(noise)))
    fused = snapshot(m_fused, *VT.fused_step(m_fused, None, dev6, beta, noise=to_dev(noise)))
    return {'oracle': o, 'o_total': o_total.detach(), 'o_terms': torch.stack([t.detach() for t in o_terms]),
            'eager': eager, 'fused': fused}


def test_train_step_matches_live_restatement(step3):
    o, got = step3['oracle'], step3['eager']
    assert_close(got['total'], step3['o_total'], 'total')
    assert_close(got['terms'], step3['o_terms'], 'terms')
    worst = 0.0
    for name, q in o.named_parameters():
        worst = max(worst, assert_close(got['grads'][name], q.grad, 'grad ' + name))
    for name, b in o.state_dict().items():
        if name.endswith('num_batches_tracked'):
            assert int(got['buffers'][name]) == int(b) == (2 if '_encoder.' in name else 7), name
        elif 'running_' in name:
            assert_close(got['buffers'][name], b, 'buffer ' + name)
    print('train_step B=3: worst gradient rel err %.2e' % worst)


def test_fused_step_matches_train_step(step3):
    eager, fused = step3['eager'], step3['fused']
    assert_close(fused['total'], eager['total'], 'total')
    assert_close(fused['terms'], eager['terms'], 'terms')
    worst = 0.0
    for name, g in eager['grads'].items():
        worst = max(worst, assert_close(fused['grads'][name], g, 'grad ' + name))
    for name, b in eager['buffers'].items():
        if name.endswith('num_batches_tracked'):
            assert int(fused['buffers'][name]) == int(b) == (2 if '_encoder.' in name else 7), name
        else:
            assert_close(fused['buffers'][name], b, 'buffer ' + name)
    print('fused_step vs train_step B=3: worst gradient rel err %.2e' % worst)


@pytest.mark.parametrize('step', ['train_step', 'fused_step'])
def test_step_matches_golden(golden_dir, step):
    fx, meta = load_golden(golden_dir, 'vision_b4')
    assert meta['n_latents'] == D
    _, m = models(meta['model_seed'])
    batch6 = tuple(x.to(DEV) for x in R.synthetic_batch(meta['batch'], meta['batch_seed']))
    noise = R.draw_step_noise(meta['batch'], D, torch.Generator().manual_seed(meta['noise_seed']))
    total, terms = getattr(VT, step)(m, None, batch6, meta['annealing_factor'], noise=to_dev(noise))
    assert_close(total.item(), fx['total'], 'total')
    assert_close(terms, fx['terms'], 'terms')
    for name, p in m.named_parameters():
        g = p.grad.detach().reshape(-1).cpu()
        ref_norm = float(fx['gnorm/' + name])
        assert abs(g.double().norm().item() - ref_norm) <= 1e-4 * max(ref_norm, 1e-30), 'grad norm ' + name
        ref = fx['ghead/' + name]
        scale = max(float(np.abs(ref).max()), ref_norm / max(g.numel(), 1) ** 0.5, 1e-30)
        assert np.abs(g[:8].numpy() - ref).max() <= 1e-4 * scale, 'grad head ' + name
    for name, b in m.state_dict().items():
        if name.endswith('num_batches_tracked'):
            assert int(b) == int(fx['nbt/' + name]), name
        elif 'running_' in name:
            assert_close(b, fx['buf/' + name], 'buffer ' + name)


def test_gray_term_kl_gradient_reaches_the_joint_logvar():
    """vision/train.py:242 takes the gray term's KL on (gray_mu, joint_logvar): d term / d joint_logvar is the KL's
    own derivative beta / B * 0.5 * (exp(logvar) - 1), and nothing else of the gray term depends on it."""
    B, beta = 3, 0.7
    _, m = models(64)
    batch6 = tuple(x.to(DEV) for x in R.synthetic_batch(B, 65))
    joint = m(*batch6)
    gray = m(gray=batch6[1])
    pairs = [v for p in zip(gray[:6], batch6) for v in p]
    term = VT.elbo_loss(*pairs, gray[6], joint[7], annealing_factor=beta)
    g_joint, = torch.autograd.grad(term, joint[7], retain_graph=True)
    assert_close(g_joint, beta / B * 0.5 * (joint[7].detach().exp() - 1), 'd gray term / d joint logvar')
    assert float(g_joint.abs().max()) > 0


def test_subset_call_in_eval_mode_returns_the_mean():
    o, m = models(66, train=False)
    x = R.synthetic_batch(4, 67)[1]
    with torch.no_grad():
        out = m(gray=x.to(DEV))
        ref = o([None, x, None, None, None, None])
    assert len(out) == 8 and torch.equal(m.last_z, out[6]), 'eval mode: z = mu'
    assert torch.equal(m.reparametrize(out[6], out[7]), out[6])
    assert_close(out[6], ref[6], 'mu'); assert_close(out[7], ref[7], 'logvar')
    for i, c in enumerate(R.N_CHANNELS):
        assert out[i].shape == (4, c, 64, 64)
        assert_close(out[i], ref[i], 'eval logits %s' % R.MODALITIES[i])
    mu, lv = m.infer(gray=x.to(DEV))
    assert torch.equal(mu, out[6]) and torch.equal(lv, out[7])
    with pytest.raises(ValueError):
        m()
