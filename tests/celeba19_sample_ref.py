"""Not a test: the restatement the celeba19 sample.py tests compare against.

``poe_table``   the table product of experts and the draw of csrc/poe_table.hip in float64 torch: PoE variant B
                (celeba19/model.py:219-226) with the N(0, 1) prior, experts added in the order ``infer`` stacks them.
``generate``    ``celeba19.sample.generate`` on the CPU oracle (oracle/models.py) in eval mode: the oracle's own encoders
                give the expert table and the image heads, ``poe_table`` the posteriors and draws, the oracle's decoders
                and torch.sigmoid the probabilities.
``fixture_model`` / ``fixture_conditions``   the inputs of tests/golden/celeba19_sample.npz, regenerated from its seeds.
"""
import numpy as np
import torch

from oracle import models as OM, steps as OS

N_ATTRS = 18
POE_EPS = 1e-8


def poe_table(table, state, img_heads=None, img_row=None, eps=None):
    """table [A, 2, 2D], state [C, A] in {-1, 0, 1}, img_heads [rows, 2D], img_row [C] (-1: none), eps [n, C, D] or None
    -> float64 (mu [C, D], logvar [C, D], z [n, C, D] or None)."""
    table = torch.as_tensor(table).double()
    state = torch.as_tensor(state).long()
    A, D = table.shape[0], table.shape[2] // 2
    C = state.shape[0]
    assert state.shape == (C, A) and int(state.min()) >= -1 and int(state.max()) <= 1
    mu = torch.zeros(C, D, dtype=torch.float64)
    logvar = torch.zeros(C, D, dtype=torch.float64)
    for c in range(C):
        experts = [torch.zeros(2 * D, dtype=torch.float64)]                       # the prior: mu = 0, logvar = 0
        if img_row is not None and int(img_row[c]) >= 0:
            experts.append(torch.as_tensor(img_heads[int(img_row[c])]).double())
        for a in range(A):
            if int(state[c, a]) >= 0:
                experts.append(table[a, int(state[c, a])])
        sum_t = torch.zeros(D, dtype=torch.float64)
        sum_mt = torch.zeros(D, dtype=torch.float64)
        for h in experts:
            t = 1.0 / (torch.exp(h[D:]) + POE_EPS)
            sum_mt = sum_mt + h[:D] * t
            sum_t = sum_t + t
        mu[c] = sum_mt / sum_t
        logvar[c] = torch.log(1.0 / sum_t)
    z = None
    if eps is not None:
        z = mu.unsqueeze(0) + torch.exp(0.5 * logvar).unsqueeze(0) * torch.as_tensor(eps).double()
    return mu, logvar, z


def oracle_table(oracle):
    """[18, 2, 2D] float32: the oracle's attribute encoders on the inputs 0 and 1."""
    values = torch.tensor([0, 1])
    with torch.no_grad():
        return torch.stack([torch.cat(enc(values), dim=1) for enc in oracle.attr_encoders])


def generate(oracle, image=None, img_row=None, state=None, eps=None):
    """The dict of ``celeba19.sample.generate`` from the eval-mode oracle; without ``eps`` the mean is decoded (z = mu,
    leading dimension 1).  mu, logvar and z are float64, the decoded probabilities float32."""
    assert not oracle.training
    with torch.no_grad():
        heads = torch.cat(oracle.image_encoder(image), dim=1) if image is not None else None
        mu, logvar, z = poe_table(oracle_table(oracle), state, heads, img_row, eps)
        if z is None:
            z = mu.unsqueeze(0)
        n, C, D = z.shape
        zr = z.reshape(n * C, D).float()
        probs_image = torch.sigmoid(oracle.image_decoder(zr))
        probs_attrs = torch.sigmoid(torch.cat([dec(zr) for dec in oracle.attr_decoders], dim=1))
    return {'mu': mu, 'logvar': logvar, 'z': z, 'image': probs_image.view(n, C, 3, 64, 64),
            'attrs': probs_attrs.view(n, C, N_ATTRS)}


def fixture_model(fx, meta):
    """The eval-mode oracle the fixture was written from: ``fill_parameters(weight_seed)`` with the recorded BatchNorm
    statistics."""
    cls, d = OM.MODELS['celeba19']
    oracle = OM.fill_parameters(cls(d), meta['weight_seed'])
    sd = oracle.state_dict()
    for k in list(sd):
        if 'running_' in k or 'num_batches' in k:
            sd[k] = torch.from_numpy(np.asarray(fx['bn/' + k])).to(sd[k].dtype)
    oracle.load_state_dict(sd)
    return oracle.eval()


def fixture_conditions(fx, meta):
    """(image [rows, 3, 64, 64], img_row [C], state [C, 18], eps [n, C, D]) of the fixture: the images regenerated from
    their seed, the conditions and the noise as recorded."""
    image, _ = OS.synthetic_batch('celeba19', meta['rows'], meta['input_seed'])
    return (image, torch.from_numpy(fx['img_row'].astype(np.int64)), torch.from_numpy(fx['state'].astype(np.int64)),
            torch.from_numpy(fx['eps']))
