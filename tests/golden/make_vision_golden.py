#!/usr/bin/env python
"""Golden fixture of the vision MVAE (vision/model.py, vision/train.py) -> tests/golden/vision_b4.npz.

Run in the build container only (needs the reference checkout, which never travels):

    python tests/golden/make_vision_golden.py [path to the reference's vision/ folder]

The reference's vision/ text does not run as a whole (see multimodal-vae-public_amd/vision/train.py for the defects), so
this generator pins every part that CAN be pinned to the reference's own text and records the rest from the restatement:

  * it EXECUTES vision/model.py:103-218 (get_batch_size, ImageEncoder, ImageDecoder, ProductOfExperts, Swish,
    prior_expert, with the imports of :1-10) and vision/train.py:61-73 (binary_cross_entropy_with_logits), unmodified,
    and asserts that the restated stacks of tests/vision_ref.py equal the reference's for C = 1 and C = 3 on the CPU in
    training mode -- outputs, input gradients, parameter gradients, BatchNorm buffers -- and the same for the PoE
    (against oracle.functional.poe variant 'A') and the elementwise BCE;
  * from the reference it records the stacks' state_dict key names and shapes, the twelve
    ``self.<name> = Image{En,De}coder(n_latents, C)`` attribute / channel pairs of vision/model.py:16-28 (by regular
    expression), the parser defaults of vision/train.py:114-127 (by ast) and the parameter count at n_latents = 250;
  * it then records the restated seven-term step (tests/vision_ref.py seven_term_step) at B = 4, D = 16: the total, the
    seven terms, a norm and the first eight values of every parameter gradient, the BatchNorm running statistics and
    num_batches_tracked.

The fixture holds digests only: weights come from ``oracle.models.fill_parameters``, inputs and noise from seeded
``torch.Generator``s, and none of them is stored."""
import ast
import os
import re
import sys
import textwrap
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import functional as OF, models as OM  # noqa: E402
import vision_ref as R  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), 'reference', 'vision')
N_LATENTS, BATCH = 16, 4
MODEL_SEED, BATCH_SEED, NOISE_SEED, ANNEAL = 71, 72, 73, 0.5


def lines(path, first, last):
    return ''.join(open(path).read().splitlines(True)[first - 1:last])


def execute_reference():
    """The parts of the reference text that run, executed as they stand."""
    model_py, train_py = os.path.join(REF, 'model.py'), os.path.join(REF, 'train.py')
    ns = {'__name__': 'vision_reference_model'}
    exec(compile(lines(model_py, 1, 10) + '\n' * 92 + lines(model_py, 103, 218), model_py, 'exec'), ns)
    ns_t = {'torch': torch, '__name__': 'vision_reference_train'}
    exec(compile('\n' * 60 + lines(train_py, 61, 73), train_py, 'exec'), ns_t)
    return ns, ns_t


def close(a, b, what, tol=2e-5):
    err = (a.detach() - b.detach()).abs().max().item() / max(b.detach().abs().max().item(), 1e-30)
    assert err <= tol, '%s: restatement vs reference %.3e' % (what, err)


def check_stacks(ns):
    """Restated stacks == reference stacks, C in {1, 3}: outputs, input / parameter gradients, BatchNorm buffers."""
    for c in (1, 3):
        g = torch.Generator().manual_seed(80 + c)
        ref_e = OM.fill_parameters(ns['ImageEncoder'](N_LATENTS, c), 81).train()
        my_e = R.ImageEncoder(N_LATENTS, c)
        my_e.load_state_dict(ref_e.state_dict(), strict=True)
        my_e.train()
        x = torch.rand(3, c, 64, 64, generator=g)
        w = torch.randn(3, 2 * N_LATENTS, generator=g)
        seen = {}
        ref_e.classifier[2].register_forward_hook(lambda m, i, o: seen.update(mask=(o != 0).float()))
        xr = x.clone().requires_grad_()
        mu, lv = ref_e(xr)
        (torch.cat((mu, lv), dim=1) * w).sum().backward()
        xm = x.clone().requires_grad_()
        mmu, mlv = my_e(xm, seen['mask'])
        (torch.cat((mmu, mlv), dim=1) * w).sum().backward()
        close(mmu, mu, 'encoder C=%d mu' % c); close(mlv, lv, 'encoder C=%d logvar' % c)
        close(xm.grad, xr.grad, 'encoder C=%d input gradient' % c, tol=1e-4)
        ref_d = OM.fill_parameters(ns['ImageDecoder'](N_LATENTS, c), 82).train()
        my_d = R.ImageDecoder(N_LATENTS, c)
        my_d.load_state_dict(ref_d.state_dict(), strict=True)
        my_d.train()
        z = torch.randn(3, N_LATENTS, generator=g)
        wd = torch.randn(3, c, 64, 64, generator=g)
        zr, zm = z.clone().requires_grad_(), z.clone().requires_grad_()
        out = ref_d(zr)
        (out * wd).sum().backward()
        mine = my_d(zm)
        (mine * wd).sum().backward()
        close(mine, out, 'decoder C=%d logits' % c); close(zm.grad, zr.grad, 'decoder C=%d input gradient' % c, tol=1e-4)
        for ref, my, what in ((ref_e, my_e, 'encoder'), (ref_d, my_d, 'decoder')):
            for (n, p), (n2, q) in zip(ref.named_parameters(), my.named_parameters()):
                assert n == n2
                close(q.grad, p.grad, '%s C=%d grad %s' % (what, c, n), tol=1e-4)
            for (n, b), (n2, b2) in zip(ref.named_buffers(), my.named_buffers()):
                assert n == n2
                close(b2.double(), b.double(), '%s C=%d buffer %s' % (what, c, n))


def check_poe_and_bce(ns, ns_t):
    g = torch.Generator().manual_seed(83)
    mu = torch.randn(4, 5, N_LATENTS, generator=g).requires_grad_()
    lv = torch.randn(4, 5, N_LATENTS, generator=g).requires_grad_()
    w = torch.randn(2, 5, N_LATENTS, generator=g)
    rm, rl = ns['ProductOfExperts']()(mu, lv)
    gr = torch.autograd.grad((rm * w[0] + rl * w[1]).sum(), (mu, lv))
    om, ol = OF.poe(mu, lv, 'A')
    go = torch.autograd.grad((om * w[0] + ol * w[1]).sum(), (mu, lv))
    close(om, rm, 'PoE mu'); close(ol, rl, 'PoE logvar')
    close(go[0], gr[0], 'PoE d mu'); close(go[1], gr[1], 'PoE d logvar')
    pm, pl = ns['prior_expert']((1, 5, N_LATENTS))
    assert float(pm.abs().sum() + pl.abs().sum()) == 0.0
    assert ns['get_batch_size'](None, torch.zeros(7, 2), None) == 7
    x = (4 * torch.randn(6, 33, generator=g)).requires_grad_()
    t = torch.rand(6, 33, generator=g)
    rb = ns_t['binary_cross_entropy_with_logits'](x, t)
    ob = OF.binary_cross_entropy_with_logits(x, t)
    close(ob, rb, 'BCE')
    close(torch.autograd.grad(ob.sum(), x)[0], torch.autograd.grad(rb.sum(), x)[0], 'BCE gradient')
    sx = torch.randn(9, generator=g)
    close(R.Swish()(sx), ns['Swish']()(sx), 'Swish')


def reference_facts(ns):
    model_py, train_py = os.path.join(REF, 'model.py'), os.path.join(REF, 'train.py')
    pairs = re.findall(r'self\.(\w+)\s*=\s*Image(En|De)coder\(n_latents,\s*(\d)\)', lines(model_py, 16, 28))
    assert len(pairs) == 12, pairs
    stack_keys, count, full_keys = [], 0, []
    stacks = {}
    for kind in ('En', 'De'):
        for c in (1, 3):
            sd = ns['Image%scoder' % kind](250, c).state_dict()
            stacks[(kind, c)] = sd
            stack_keys += ['%s%d %s %s' % (kind, c, k, 'x'.join(str(d) for d in v.shape)) for k, v in sd.items()]
    for name, kind, c in pairs:
        sd = stacks[(kind, int(c))]
        count += sum(v.numel() for k, v in sd.items() if not (k.endswith('running_mean') or k.endswith('running_var')
                                                              or k.endswith('num_batches_tracked')))
        full_keys += ['%s.%s %s' % (name, k, 'x'.join(str(d) for d in v.shape)) for k, v in sd.items()]
    defaults = []
    for node in ast.walk(ast.parse(textwrap.dedent(lines(train_py, 114, 127)))):
        if isinstance(node, ast.Call) and getattr(node.func, 'attr', '') == 'add_argument':
            default = [ast.literal_eval(k.value) for k in node.keywords if k.arg == 'default'][0]
            defaults.append('%s %r' % (node.args[0].value, default))
    return {'stack_keys': np.array(stack_keys), 'state_keys': np.array(full_keys),
            'attr_pairs': np.array(['%s %scoder %s' % p for p in pairs]), 'n_params_250': np.int64(count),
            'parser_defaults': np.array(defaults)}


def restated_step():
    model = OM.fill_parameters(R.MVAE(N_LATENTS), MODEL_SEED).train()
    batch6 = R.synthetic_batch(BATCH, BATCH_SEED)
    noise = R.draw_step_noise(BATCH, N_LATENTS, torch.Generator().manual_seed(NOISE_SEED))
    total, terms, _ = R.seven_term_step(model, batch6, noise, ANNEAL)
    total.backward()
    return model, total, terms


def step_digests(model, total, terms):
    fx = {'total': np.float64(total.item()), 'terms': np.array([t.item() for t in terms], dtype=np.float64)}
    for name, p in model.named_parameters():
        g = p.grad.detach().reshape(-1)
        fx['gnorm/' + name] = np.float64(g.double().norm().item())
        fx['ghead/' + name] = g[:8].numpy().copy()
    for name, b in model.named_buffers():
        if name.endswith('running_mean') or name.endswith('running_var'):
            fx['buf/' + name] = b.numpy().copy()
        elif name.endswith('num_batches_tracked'):
            fx['nbt/' + name] = np.int64(b.item())
    return fx


def main():
    warnings.simplefilter('ignore')
    ns, ns_t = execute_reference()
    check_stacks(ns)
    check_poe_and_bce(ns, ns_t)
    fx = reference_facts(ns)
    fx.update(step_digests(*restated_step()))
    fx['meta'] = np.array(repr({'n_latents': N_LATENTS, 'batch': BATCH, 'model_seed': MODEL_SEED, 'batch_seed': BATCH_SEED,
                                'noise_seed': NOISE_SEED, 'annealing_factor': ANNEAL, 'torch': torch.__version__}))
    path = os.path.join(HERE, 'vision_b4.npz')
    np.savez_compressed(path, **fx)
    print('wrote %s (%d arrays, %d bytes); total %.6f, n_params(250) %d' % (
        path, len(fx), os.path.getsize(path), fx['total'], fx['n_params_250']))


if __name__ == '__main__':
    main()
