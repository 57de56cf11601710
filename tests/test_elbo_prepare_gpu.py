"""GPU: the ELBO bookkeeping launch that also carries Adam's counter launch (mvae_elbo_reduce_prepare) is
mvae_elbo_reduce + mvae_adam_prepare, bit for bit; a captured step that uses it equals one that keeps the two launches."""
import pytest
import torch

import mvae_amd
from mvae_amd import kernels as K
from mvae_amd.engine import BimodalStep
from mvae_amd.optim import FusedAdam
from oracle import models as OM, steps as OS

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def g(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize('with_zero', [False, True])
def test_elbo_reduce_prepare_is_the_two_launches(with_zero):
    """3 parts of 4 rows per group: elbo and the cleared buffer against elbo_reduce, counter and the two
    bias-correction factors against adam_prepare -- equal bits, at several counter values."""
    T, R = 3, 4
    kl, ri, rl = g(T * R, seed=1), g(2 * R, seed=2), g(1 * R, seed=3)
    ck, ci, cl = torch.rand(T).to(DEV), torch.rand(2).to(DEV), torch.rand(1).to(DEV)
    parts = [(kl, ck, None, 0, T, R), (ri, ci, None, 0, 2, R), (rl, cl, None, 2, 1, R)]
    lr, b1, b2 = 1e-3, 0.9, 0.999
    for start in (0, 1, 999, 123456):
        want = torch.full((T + 1,), float('nan'), device=DEV)
        got = torch.full((T + 1,), float('nan'), device=DEV)
        zero_w = torch.full((4099,), 3.0, device=DEV) if with_zero else None
        zero_g = torch.full((4099,), 3.0, device=DEV) if with_zero else None
        ctr_w = torch.full((1,), 5, dtype=torch.int64, device=DEV)
        ctr_g = ctr_w.clone()
        step_w = torch.full((1,), start, dtype=torch.int64, device=DEV)
        step_g = step_w.clone()
        coef_w = torch.full((2,), float('nan'), device=DEV)
        coef_g = torch.full((2,), float('nan'), device=DEV)
        K.elbo_reduce(parts, want, T, zero=zero_w, counter_dev=ctr_w, counter_inc=2)
        K.adam_prepare(step_w, 1, lr, b1, b2, coef_w)
        K.elbo_reduce_prepare(parts, got, T, step_g, 1, lr, b1, b2, coef_g, zero=zero_g, counter_dev=ctr_g,
                              counter_inc=2)
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want)) and not torch.isnan(got).any()
        assert ctr_g.item() == 7 and ctr_w.item() == 7
        assert step_g.item() == start + 1 and step_w.item() == start + 1
        assert torch.equal(bits(coef_g), bits(coef_w)) and not torch.isnan(coef_g).any()
        if with_zero:
            assert torch.equal(bits(zero_g), bits(zero_w)) and zero_g.abs().max().item() == 0
    ref = (kl.double().reshape(T, R).sum(1) * ck.double())
    ref[:2] += ri.double().reshape(2, R).sum(1) * ci.double()
    ref[2:] += rl.double().reshape(1, R).sum(1) * cl.double()
    assert (got[:T].double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    with pytest.raises(RuntimeError):
        K.elbo_reduce_prepare([(kl, ck, None, 1, T, R)], got, T, step_g, 1, lr, b1, b2, coef_g)   # terms 1..3: T = 3
    assert step_g.item() == start + 1          # a refused call launches nothing


def _captured_run(monkeypatch, switch, kind, batch, lam, split_dz='1'):
    monkeypatch.setenv('MVAE_ELBO_PREPARE', switch)
    monkeypatch.setenv('MVAE_SPLIT_DZ', split_dz)
    cls, d = OM.MODELS[kind]
    oracle = OM.fill_parameters(cls(d), 37)
    model = getattr(mvae_amd, kind).model.MVAE(d)
    model.load_state_dict(oracle.state_dict())
    model.to(DEV).train()
    model.finalize()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    eng = BimodalStep(model, batch, 1.0, lam, seed=11)
    assert eng.elbo_prepare == (switch == '1')
    image, label = OS.synthetic_batch(kind, batch, seed=800)
    # the eager step() has no optimizer and keeps mvae_elbo_reduce under either setting
    eager_elbo = eng.step(image.to(DEV), label.to(DEV), 0.5).clone()
    eager_grad = model.arena.grad.clone()
    eng.capture(opt, image.shape[1:], label)
    elbos = []
    for step in range(3):
        image, label = OS.synthetic_batch(kind, batch, seed=810 + step)
        elbos.append(eng.replay(image.to(DEV), label.to(DEV), 0.5).clone())
    torch.cuda.synchronize()
    assert opt._step_dev.item() == 3
    return (torch.stack(elbos), model.arena.grad.clone(), model.arena.flat.clone(), opt._m.clone(), opt._v.clone(),
            opt._coef.clone(), eng.counter.clone(), eager_elbo, eager_grad)


@pytest.mark.parametrize('kind,batch,lam,split_dz', [('mnist', 64, 50.0, '1'), ('mnist', 64, 50.0, '0'),
                                                     ('celeba', 6, 10.0, '1')])
def test_captured_step_is_the_same_with_the_counter_launch_folded(kind, batch, lam, split_dz, monkeypatch):
    """MVAE_ELBO_PREPARE=1 (default) against =0: one eager step() (ELBO, gradients), then capture() + 3 replays: ELBO of
    every step, gradients, parameters and moments after FusedAdam, the bias-correction factors and the Philox counter --
    equal bits."""
    on = _captured_run(monkeypatch, '1', kind, batch, lam, split_dz)
    off = _captured_run(monkeypatch, '0', kind, batch, lam, split_dz)
    names = ('elbo', 'gradients', 'parameters', 'exp_avg', 'exp_avg_sq', 'coef2', 'philox counter', 'eager elbo',
             'eager gradients')
    assert len(on) == len(off) == len(names)
    for a, b, what in zip(on, off, names):
        assert torch.equal(bits(a), bits(b)), what
    assert torch.isfinite(on[0]).all() and torch.isfinite(on[7]).all() and on[6].item() == off[6].item() != 0
