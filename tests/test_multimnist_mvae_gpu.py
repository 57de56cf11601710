"""GPU parity of the MultiMNIST image stacks and MVAE (multimnist/model.py, multimnist/train.py): the HIP modules
against the golden captured from the unmodified reference (tests/golden/multimnist_mvae_b6.npz) and against the live
plain-torch restatement (tests/multimnist_ref.py, which the golden generator proves equal to the reference), forward and
backward, with every noise draw replayed.  Bar: util.REL_TOL (1e-4 of max |ref|) on outputs, terms, every gradient and
the BatchNorm running statistics; the fed-back characters bit-exact.

The text decoder feeds back arg-max characters: the live cases first check, on the CPU side, that the top two logits
of every fed-back position differ by >= 1e-3 x max|logit| (as the golden generator does) and skip a seed that does not
-- the seeds below were chosen on the CPU so that none does."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd.multimnist import model as MM, train as MT
from oracle import models as OM, multimnist as OMM
import multimnist_ref as R
from util import assert_close, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-3


def pair(ref_cls, hip_cls, seed, train=True):
    o = OM.fill_parameters(ref_cls(64), seed)
    m = hip_cls(64)
    m.load_state_dict(o.state_dict(), strict=True)
    m.to(DEV)
    o.train(train); m.train(train)
    return o, m


def compare_params_and_buffers(o, m, what):
    worst = 0.0
    for (name, q), (n2, p) in zip(o.named_parameters(), m.named_parameters()):
        assert name == n2
        worst = max(worst, assert_close(p.grad, q.grad, '%s grad %s' % (what, name)))
    for (name, b), (n2, b2) in zip(o.named_buffers(), m.named_buffers()):
        assert name == n2
        if not name.endswith('num_batches_tracked'):
            assert_close(b2, b, '%s buffer %s' % (what, name))
    return worst


@pytest.mark.parametrize('batch', [1, 5, 37])
def test_image_encoder_training_matches_restatement(batch):
    o, m = pair(R.ImageEncoder, MM.ImageEncoder, 51)
    g = torch.Generator().manual_seed(52 + batch)
    x = torch.rand(batch, 1, 50, 50, generator=g)
    mask = torch.empty(batch, 512).bernoulli_(0.9, generator=g)
    w8 = torch.randn(batch, 128, generator=g)
    mu, lv = o(x, mask)
    (torch.cat((mu, lv), dim=1) * w8).sum().backward()
    hmu, hlv = m(x.to(DEV), mask.to(DEV))
    (torch.cat((hmu, hlv), dim=1) * w8.to(DEV)).sum().backward()
    assert_close(hmu, mu.detach(), 'mu'); assert_close(hlv, lv.detach(), 'logvar')
    print('image encoder B=%d: worst gradient rel err %.2e' % (batch, compare_params_and_buffers(o, m, 'encoder')))


@pytest.mark.parametrize('batch', [1, 5, 37])
def test_image_decoder_training_matches_restatement(batch):
    o, m = pair(R.ImageDecoder, MM.ImageDecoder, 53)
    g = torch.Generator().manual_seed(54 + batch)
    z = torch.randn(batch, 64, generator=g)
    w8 = torch.randn(batch, 1, 50, 50, generator=g)
    zo = z.clone().requires_grad_()
    out = o(zo)
    (out * w8).sum().backward()
    zh = z.to(DEV).requires_grad_()
    got = m(zh)
    assert got.shape == (batch, 1, 50, 50)
    (got * w8.to(DEV)).sum().backward()
    assert_close(got, out.detach(), 'logits'); assert_close(zh.grad, zo.grad, 'd z')
    print('image decoder B=%d: worst gradient rel err %.2e' % (batch, compare_params_and_buffers(o, m, 'decoder')))


def test_image_stacks_eval_mode_after_one_training_pass():
    g = torch.Generator().manual_seed(55)
    oe, me = pair(R.ImageEncoder, MM.ImageEncoder, 51)
    od, md = pair(R.ImageDecoder, MM.ImageDecoder, 53)
    x, mask, z = torch.rand(3, 1, 50, 50, generator=g), torch.empty(3, 512).bernoulli_(0.9, generator=g), torch.randn(3, 64, generator=g)
    with torch.no_grad():
        oe(x, mask); me(x.to(DEV), mask.to(DEV)); od(z); md(z.to(DEV))      # advance the running statistics
        for mod in (oe, me, od, md):
            mod.eval()
        mu, lv = oe(x)
        hmu, hlv = me(x.to(DEV))
        assert_close(hmu, mu, 'eval mu'); assert_close(hlv, lv, 'eval logvar')
        assert_close(md(z.to(DEV)), od(z), 'eval logits')


def models(seed, train=True):
    o = OM.fill_parameters(R.MVAE(64), seed)
    m = MM.MVAE(64)
    m.load_state_dict(o.state_dict(), strict=True)
    m.to(DEV)
    o.train(train); m.train(train)
    return o, m


def to_dev(noise):
    return [{'mask': None if n['mask'] is None else n['mask'].to(DEV), 'eps': n['eps'].to(DEV), 'gru': n['gru']} for n in noise]


def hip_step(m, image, text, noise, li, lt, beta):
    """The three-call step on the HIP modules; returns total, terms, outs, and per call (z, fed-back characters)."""
    extra = []

    def call(*a, **kw):
        out = m(*a, **kw)
        extra.append((m.last_z.clone(), m.text_decoder.last_fed.clone()))
        return out
    total, terms, outs = R.three_call_step(call, image.to(DEV), text.to(DEV), to_dev(noise), li, lt, beta, elbo=MT.elbo_loss)
    return total, terms, outs, extra


def test_mvae_step_matches_reference_golden(golden_dir):
    fx, meta = load_golden(golden_dir, 'multimnist_mvae_b6')
    _, m = models(meta['model_seed'])
    image, text = torch.from_numpy(fx['image']), torch.from_numpy(fx['text'])
    noise = []
    for c, (wi, _) in enumerate(R.CALLS):
        noise.append({'mask': torch.from_numpy(fx['mask%d' % c]).float() if wi else None, 'eps': torch.from_numpy(fx['eps%d' % c]),
                      'gru': [torch.from_numpy(fx['gru%d_%d' % (c, i)]).float() for i in range(4)]})
    total, terms, outs, extra = hip_step(m, image, text, noise, meta['lambda_image'], meta['lambda_text'], meta['annealing_factor'])
    total.backward()
    assert_close(total.item(), fx['total'], 'total')
    for c in range(3):
        assert_close(terms[c].item(), fx['terms'][c], 'term %d' % c)
        assert_close(outs[c][2], fx['mu%d' % c], 'mu %d' % c); assert_close(outs[c][3], fx['logvar%d' % c], 'logvar %d' % c)
        assert_close(extra[c][0], fx['z%d' % c], 'z %d' % c)
        assert outs[c][0].shape == (meta['batch'], 1, 50, 50)
        # the head of sample 0's image logits, against the scale of the recorded slice
        assert_close(outs[c][0].reshape(meta['batch'], -1)[0, :64], fx['img_head%d' % c], 'image logits %d' % c)
    for c in (0, 2):
        assert_close(outs[c][1], fx['words%d' % c], 'text logits %d' % c)
        assert np.array_equal(extra[c][1].cpu().numpy(), fx['fed%d' % c]), 'fed-back characters of call %d' % c
    for name, p in m.named_parameters():
        g = p.grad.detach().reshape(-1).cpu()
        ref_norm = float(fx['gnorm/' + name])
        assert abs(g.double().norm().item() - ref_norm) <= 1e-4 * max(ref_norm, 1e-30), 'grad norm ' + name
        ref = fx['ghead/' + name]
        scale = max(float(np.abs(ref).max()), ref_norm / max(g.numel(), 1) ** 0.5, 1e-30)
        assert np.abs(g[:8].numpy() - ref).max() <= 1e-4 * scale, 'grad head ' + name
    for name, b in m.named_buffers():
        if name.endswith('running_mean') or name.endswith('running_var'):
            assert_close(b, fx['buf/' + name], 'buffer ' + name)


@pytest.mark.parametrize('batch,model_seed,seed', [(100, 61, 230), (7, 62, 62)])
def test_mvae_step_matches_live_restatement(batch, model_seed, seed):
    o, m = models(model_seed)
    g = torch.Generator().manual_seed(seed + 100)
    image = torch.rand(batch, 1, 50, 50, generator=g)
    text = OMM.synthetic_text(batch, seed + 200)
    noise = [R.draw_call_noise(batch, 64, wi, generator=g) for wi, _ in R.CALLS]
    o_total, o_terms, o_outs = R.three_call_step(o, image, text, noise, 1.0, 10.0, 0.5)
    margins = [R.argmax_margin(out[1]) for out in o_outs]
    if min(margins) < MARGIN:
        pytest.skip('seed %d: arg-max margin %.2e < %.0e on the CPU side' % (seed, min(margins), MARGIN))
    fed = []
    o_total.backward()
    total, terms, outs, extra = hip_step(m, image, text, noise, 1.0, 10.0, 0.5)
    total.backward()
    assert_close(total, o_total.detach(), 'total')
    for c in range(3):
        assert_close(terms[c], o_terms[c].detach(), 'term %d' % c)
        for i, what in ((0, 'image logits'), (1, 'text logits'), (2, 'mu'), (3, 'logvar')):
            assert_close(outs[c][i], o_outs[c][i].detach(), '%s %d' % (what, c))
        assert_close(extra[c][0], o_outs[c][4].detach(), 'z %d' % c)
        fed.append(extra[c][1])
    assert torch.equal(fed[2].cpu(), o.last_fed), 'greedy feedback diverged'
    print('MVAE B=%d: worst gradient rel err %.2e, margins %s' % (
        batch, compare_params_and_buffers(o, m, 'mvae'), ['%.1e' % x for x in margins]))


def test_infer_eval_forward_and_state_dict_round_trip():
    o, m = models(63, train=False)
    g = torch.Generator().manual_seed(64)
    image, text = torch.rand(5, 1, 50, 50, generator=g), OMM.synthetic_text(5, 65)
    with torch.no_grad():
        for im, tx in ((image, None), (None, text), (image, text)):
            mu, lv = o.infer(im, tx)
            hmu, hlv = m.infer(None if im is None else im.to(DEV), None if tx is None else tx.to(DEV))
            assert_close(hmu, mu, 'infer mu'); assert_close(hlv, lv, 'infer logvar')
        img, words, mu, lv, z = o(image, text)
        himg, hwords, hmu, hlv = m(image.to(DEV), text.to(DEV))
        assert torch.equal(m.last_z, hmu), 'eval mode: z = mu'
        assert torch.equal(m.reparametrize(hmu, hlv), hmu)
        assert_close(himg, img, 'eval image logits'); assert_close(hwords, words, 'eval text logits')
    with pytest.raises(ValueError):
        m()
    m2 = MM.MVAE(64)
    m2.load_state_dict(o.state_dict(), strict=True)
    o.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)


def test_train_cli_runs_and_writes_a_loadable_checkpoint(tmp_path):
    cmd = ['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'multimodal-vae-public_amd', 'multimnist', 'train.py'),
           '--cuda', '--synthetic', '--epochs', '1', '--steps-per-epoch', '3', '--batch-size', '8', '--out-dir', str(tmp_path)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('====> Epoch: 1')]
    assert line, r.stdout[-3000:]
    assert np.isfinite(float(line[0].split('Loss:')[1]))
    test_line = [ln for ln in r.stdout.splitlines() if ln.startswith('====> Test Loss:')]
    assert test_line and np.isfinite(float(test_line[0].split(':')[1]))
    ckpt = torch.load(os.path.join(str(tmp_path), 'checkpoint.pth.tar'), map_location='cpu', weights_only=False)
    assert sorted(ckpt) == ['best_loss', 'n_latents', 'optimizer', 'state_dict'] and ckpt['n_latents'] == 64
    model = MT.load_checkpoint(os.path.join(str(tmp_path), 'checkpoint.pth.tar'))
    assert isinstance(model, MM.MVAE) and all(torch.isfinite(v).all() for v in model.state_dict().values())
    assert os.path.exists(os.path.join(str(tmp_path), 'model_best.pth.tar'))
