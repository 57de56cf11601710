#!/usr/bin/env python
"""Golden fixture of the whole MultiMNIST MVAE train step from the UNMODIFIED reference (multimnist/model.py,
multimnist/train.py:22-68,207-228).

Run in the build container only (needs the reference checkout that make_multimnist_golden.py imports, which never travels):

    python tests/golden/make_multimnist_mvae_golden.py

Imports the reference with the import-time shims of make_multimnist_golden.py, fills ``MVAE(64)`` with the deterministic
weights of ``oracle.models.fill_parameters``, and runs the reference's loop body -- three ``model()`` calls, three
``elbo_loss`` (lambda_image 1, lambda_text 10, annealing factor 0.5), ``backward()`` -- in TRAINING mode under
``torch.manual_seed``.  The generator is then replayed to recover the noise in draw order (per call: the image encoder's
Bernoulli(0.9) mask when an image is given, eps, the four GRU masks), and the plain-torch restatement
``tests/multimnist_ref.py`` must reproduce every recorded value on that noise before anything is written.

A condition on the seeds, not a tolerance: greedy arg-max feedback makes the text decoder discontinuous, so the script
refuses to write a fixture in which the reference's top-1 and top-2 logits at a fed-back position differ by less than
1e-3 x max|logit| -- pick another seed.  The fixture is data (npz): inputs, noise, terms, latents, digests of logits and
gradients, BatchNorm running statistics, the state_dict key / shape list and the reference parser's defaults."""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)

from oracle import models as OM, multimnist as OMM  # noqa: E402
import multimnist_ref as R  # noqa: E402
from make_multimnist_golden import REF, import_reference  # noqa: E402

N_LATENTS, BATCH = 64, 6
MODEL_SEED, IMAGE_SEED, TEXT_SEED, NOISE_SEED = 41, 42, 43, 44
LAMBDA_IMAGE, LAMBDA_TEXT, ANNEAL = 1.0, 10.0, 0.5
MARGIN = 1e-3


def reference_parser_defaults(train_path):
    """(flag, default) of every add_argument call in the reference's __main__ block, read from its text with ast
    (the block builds data loaders when executed)."""
    import ast
    tree = ast.parse(open(train_path).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, 'attr', '') == 'add_argument':
            flag = node.args[0].value
            default = [ast.literal_eval(k.value) for k in node.keywords if k.arg == 'default'][0]
            out.append((flag, default))
    return out


def main():
    warnings.simplefilter('ignore')
    M, T, U = import_reference()
    ref = OM.fill_parameters(M.MVAE(N_LATENTS), MODEL_SEED).train()
    image = torch.rand(BATCH, 1, 50, 50, generator=torch.Generator().manual_seed(IMAGE_SEED))
    text = OMM.synthetic_text(BATCH, TEXT_SEED)

    torch.manual_seed(NOISE_SEED)
    outs = [ref(image, text), ref(image), ref(text=text)]
    terms = [T.elbo_loss(outs[0][0], image, outs[0][1], text, outs[0][2], outs[0][3], LAMBDA_IMAGE, LAMBDA_TEXT, ANNEAL),
             T.elbo_loss(outs[1][0], image, None, None, outs[1][2], outs[1][3], LAMBDA_IMAGE, LAMBDA_TEXT, ANNEAL),
             T.elbo_loss(None, None, outs[2][1], text, outs[2][2], outs[2][3], LAMBDA_IMAGE, LAMBDA_TEXT, ANNEAL)]
    total = terms[0] + terms[1] + terms[2]
    total.backward()
    for c, o in enumerate(outs):
        m = R.argmax_margin(o[1])
        assert m >= MARGIN, 'call %d: arg-max margin %.2e < %.0e -- pick another seed' % (c, m, MARGIN)

    # the restatement on the replayed noise
    mine = R.MVAE(N_LATENTS)
    sd0 = OM.fill_parameters(M.MVAE(N_LATENTS), MODEL_SEED).state_dict()
    mine.load_state_dict(sd0, strict=True)
    mine.train()
    torch.manual_seed(NOISE_SEED)
    noise = [R.draw_call_noise(BATCH, N_LATENTS, wi) for wi, _ in R.CALLS]
    o_total, o_terms, o_outs = R.three_call_step(mine, image, text, noise, LAMBDA_IMAGE, LAMBDA_TEXT, ANNEAL)
    o_total.backward()

    def close(a, b, what, tol=2e-5):
        err = (a.detach() - b.detach()).abs().max().item() / max(b.detach().abs().max().item(), 1e-30)
        assert err <= tol, '%s: restatement vs reference %.3e' % (what, err)
    close(o_total, total, 'total')
    for c in range(3):
        close(o_terms[c], terms[c], 'term %d' % c)
        close(o_outs[c][0], outs[c][0], 'image logits %d' % c); close(o_outs[c][1], outs[c][1], 'text logits %d' % c)
        close(o_outs[c][2], outs[c][2], 'mu %d' % c); close(o_outs[c][3], outs[c][3], 'logvar %d' % c)
    for (n, p), (n2, q) in zip(ref.named_parameters(), mine.named_parameters()):
        assert n == n2
        close(q.grad, p.grad, 'grad ' + n, tol=1e-4)
    for (n, b), (n2, b2) in zip(ref.named_buffers(), mine.named_buffers()):
        assert n == n2
        close(b2.double(), b.double(), 'buffer ' + n)

    fx = {'image': image.numpy(), 'text': text.numpy(), 'total': np.float64(total.item()),
          'terms': np.array([t.item() for t in terms], dtype=np.float64)}
    for c, (nz, o, oo) in enumerate(zip(noise, outs, o_outs)):
        if nz['mask'] is not None:
            fx['mask%d' % c] = nz['mask'].numpy().astype(np.uint8)
        fx['eps%d' % c] = nz['eps'].numpy()
        for i, m in enumerate(nz['gru']):
            fx['gru%d_%d' % (c, i)] = m.numpy().astype(np.uint8)
        fx['mu%d' % c] = o[2].detach().numpy(); fx['logvar%d' % c] = o[3].detach().numpy()
        fx['z%d' % c] = oo[4].detach().numpy()          # the reference does not return z: the restatement's, on its noise
        fx['img_head%d' % c] = o[0].detach().reshape(BATCH, -1)[0, :64].numpy().copy()
    for c in (0, 2):
        fx['words%d' % c] = outs[c][1].detach().numpy()
        fx['fed%d' % c] = torch.stack([torch.full((BATCH,), OMM.SOS, dtype=torch.long)] +
                                      [outs[c][1][:, i].argmax(dim=1) for i in range(OMM.MAX_LENGTH - 1)]).numpy()
    for name, p in ref.named_parameters():
        g = p.grad.detach().reshape(-1)
        fx['gnorm/' + name] = np.float64(g.double().norm().item())
        fx['ghead/' + name] = g[:8].numpy().copy()
    for name, b in ref.named_buffers():
        if name.endswith('running_mean') or name.endswith('running_var'):
            fx['buf/' + name] = b.numpy().copy()
    fx['state_keys'] = np.array(['%s %s' % (k, 'x'.join(str(d) for d in v.shape)) for k, v in ref.state_dict().items()])
    fx['parser_defaults'] = np.array(['%s %r' % fd for fd in reference_parser_defaults(os.path.join(REF, 'train.py'))])
    fx['meta'] = np.array(repr({'n_latents': N_LATENTS, 'batch': BATCH, 'model_seed': MODEL_SEED, 'image_seed': IMAGE_SEED,
                                'text_seed': TEXT_SEED, 'noise_seed': NOISE_SEED, 'lambda_image': LAMBDA_IMAGE,
                                'lambda_text': LAMBDA_TEXT, 'annealing_factor': ANNEAL, 'torch': torch.__version__}))
    path = os.path.join(HERE, 'multimnist_mvae_b6.npz')
    np.savez_compressed(path, **fx)
    print('wrote %s (%d arrays, %d bytes); total %.6f, margins %s' % (
        path, len(fx), os.path.getsize(path), total.item(), ['%.2e' % R.argmax_margin(o[1]) for o in outs]))


if __name__ == '__main__':
    main()
