"""GPU: ``mvae_poe_table_draw`` (K27, csrc/poe_table.hip) against the float64 restatement (tests/celeba19_sample_ref.py),
against the surface it extends (``model.infer`` on a batch of 1 per condition row, i.e. poe.hip) and against
``philox_fill`` for the device draw; ``celeba19.sample.generate`` against the fixture written from the reference
(tests/golden/celeba19_sample.npz) and against the model's own eval-mode forward; and the sample.py command line.

Tolerance: the project's 1e-4 relative in fp32 (``util.assert_close``, max-normalised), as the other kernel tests use it."""
import os
import struct
import subprocess
import sys

import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from mvae_amd.celeba19 import model as CM, sample as CS
import celeba19_sample_ref as SR
from util import assert_close, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


# ----------------------------------------------------------------------------- the kernel on synthetic tables
def kernel_inputs(D, C, A, img, seed):
    """Host tensors: table [A, 2, 2D], state [C, A] (row 0 a random mix, then nothing present, all at 0, all at 1, then
    random mixes), and per ``img`` mode the image heads and rows: 'none'; 'per_row' (one image row per condition);
    'shared' (fewer image rows than conditions: rows are shared, and some conditions have no image)."""
    g = torch.Generator().manual_seed(seed)
    table = 0.5 * torch.randn(A, 2, 2 * D, generator=g)
    state = torch.randint(-1, 2, (C, A), generator=g)
    state[0, 0] = int(state[0, 0]) % 2                    # row 0 has an expert: no output tensor is all prior (all zero)
    for c, v in ((1, -1), (2, 0), (3, 1)):
        if c < C:
            state[c] = v
    heads = img_row = None
    if img == 'per_row':
        heads = 0.5 * torch.randn(C, 2 * D, generator=g)
        img_row = torch.arange(C)
    elif img == 'shared':
        rows = max(1, C // 2)
        heads = 0.5 * torch.randn(rows, 2 * D, generator=g)
        img_row = torch.arange(C) % rows
        img_row[1::5] = -1                                # the nothing-present row among them
    eps = torch.randn(3, C, D, generator=g)
    return table, state, heads, img_row, eps


def run_kernel(table, state, heads, img_row, n, eps=None, **draw):
    """``poe_table_draw`` into NaN-filled outputs -> (mu, logvar, z or None)."""
    C, D = state.shape[0], table.shape[2] // 2
    mu = torch.full((C, D), NAN, device=DEV)
    logvar = torch.full((C, D), NAN, device=DEV)
    z = torch.full((n, C, D), NAN, device=DEV) if n else None
    K.poe_table_draw(table.to(DEV), state, mu, logvar, z, img_heads=heads.to(DEV) if heads is not None else None,
                     img_row=img_row, eps=eps.to(DEV) if eps is not None else None, **draw)
    return mu, logvar, z


@pytest.mark.parametrize('img', ['none', 'per_row', 'shared'])
@pytest.mark.parametrize('A', [1, 18])
@pytest.mark.parametrize('C', [1, 2, 3, 67])
@pytest.mark.parametrize('D', [20, 64, 100, 130])
def test_kernel_matches_float64(D, C, A, img):
    """D below a wave, exactly a wave, ragged second and third passes; n = 0, 1, 3 with eps replayed."""
    table, state, heads, img_row, eps = kernel_inputs(D, C, A, img, 7 + D + 1000 * C + A)
    mu64, lv64, z64 = SR.poe_table(table, state, heads, img_row, eps)
    for n in (0, 1, 3):
        mu, logvar, z = run_kernel(table, state, heads, img_row, n, eps=eps[:n] if n else None)
        tag = 'D %d C %d A %d img %s n %d' % (D, C, A, img, n)
        assert torch.isfinite(mu).all() and torch.isfinite(logvar).all()
        assert_close(mu, mu64, tag + ': mu')
        assert_close(logvar, lv64, tag + ': logvar')
        if n:
            assert torch.isfinite(z).all()
            assert_close(z, z64[:n], tag + ': z')
        else:
            assert z is None


def test_kernel_prior_rows_are_exact():
    """Nothing present: the only expert is the N(0, 1) prior, T = 1 / (exp(0) + 1e-8) and 1 + 1e-8 is 1 in fp32, so
    mu = 0 / 1 and logvar = log(1 / 1) are exactly 0 (derived, not measured) and z is eps, bit for bit."""
    D = 130
    table, state, heads, _, eps = kernel_inputs(D, 5, 18, 'shared', 3)
    state[3] = -1
    img_row = torch.tensor([0, -1, 1, -1, 1])
    mu, logvar, z = run_kernel(table, state, heads, img_row, 3, eps=eps)
    for c in (1, 3):
        assert bool((mu[c] == 0).all()) and bool((logvar[c] == 0).all())
        assert torch.equal(z[:, c].cpu(), eps[:, c])
    assert float(mu[0].abs().max()) > 0 and float(mu[2].abs().max()) > 0 and float(mu[4].abs().max()) > 0


def test_kernel_device_draw_is_the_philox_stream():
    """n = 19 draws (three slices of the grid, the last ragged) at D = 130: ``eps_out`` equals what ``philox_fill`` writes
    for [n, C, D] with the same seed, counter and offset, bit for bit; z is the replay of that noise, bit for bit; two
    calls with the same seed give the same bits; the counter is not advanced."""
    n, C, D, seed, offset = 19, 3, 130, 0x1234567, 2
    table, state, heads, img_row, _ = kernel_inputs(D, C, 18, 'per_row', 5)
    counter = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    want = torch.empty(n, C, D, device=DEV)
    K.philox_fill(want, seed, counter, offset)
    outs = []
    for _ in range(2):
        eps_out = torch.full((n, C, D), NAN, device=DEV)
        mu, logvar, z = run_kernel(table, state, heads, img_row, n, seed=seed, counter_dev=counter, counter_offset=offset,
                                   eps_out=eps_out)
        outs.append((mu, logvar, z, eps_out))
    assert int(counter.item()) == 5
    assert torch.equal(outs[0][3], want)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    mu_r, lv_r, z_r = run_kernel(table, state, heads, img_row, n, eps=want.cpu())
    assert torch.equal(mu_r, outs[0][0]) and torch.equal(lv_r, outs[0][1]) and torch.equal(z_r, outs[0][2])
    other = run_kernel(table, state, heads, img_row, n, seed=seed + 1, counter_dev=counter, counter_offset=offset)[2]
    assert not torch.equal(other, outs[0][2])


# ----------------------------------------------------------------------------- on the model
@pytest.fixture(scope='module')
def fixture(golden_dir):
    return load_golden(golden_dir, 'celeba19_sample')


@pytest.fixture(scope='module')
def pair(fixture):
    """(oracle, model): the eval-mode CPU oracle of the fixture and the HIP model on its weights, built once."""
    fx, meta = fixture
    oracle = SR.fixture_model(fx, meta)
    model = CM.MVAE(meta['n_latents'])
    model.load_state_dict(oracle.state_dict())
    model.to(DEV).train()
    model.finalize()
    model.eval()
    return oracle, model


def test_expert_table_matches_the_oracle_encoders(pair):
    oracle, model = pair
    table = CS.expert_table(model)
    assert tuple(table.shape) == (18, 2, 2 * model.n_latents)
    assert_close(table, SR.oracle_table(oracle), 'expert table')


def test_kernel_matches_model_infer_per_condition(pair, fixture):
    """For every condition row, ``model.infer`` on a batch of 1 with that row's modalities (the existing surface: the
    encoders' own launches and poe.hip) against the one table launch."""
    fx, meta = fixture
    _, model = pair
    image, img_row, state, _ = SR.fixture_conditions(fx, meta)
    state = torch.cat([state, CS.sweep_states()[1:6].long()])
    img_row = torch.cat([img_row, torch.tensor([-1, 1, -1, 0, -1])])
    with torch.no_grad():
        table = CS.expert_table(model)
        heads = model.image_encoder.heads(image.to(DEV))
        C, D = state.shape[0], model.n_latents
        mu = torch.empty(C, D, device=DEV)
        logvar = torch.empty(C, D, device=DEV)
        K.poe_table_draw(table, state, mu, logvar, None, img_heads=heads, img_row=img_row)
        for c in range(C):
            img = image[int(img_row[c]):int(img_row[c]) + 1].to(DEV) if int(img_row[c]) >= 0 else None
            lst = [state[c, a].reshape(1).float().to(DEV) if int(state[c, a]) >= 0 else None for a in range(18)]
            mu_i, lv_i = model.infer(image=img, attrs=lst if any(t is not None for t in lst) else None)
            assert_close(mu[c], mu_i[0], 'mu vs infer, condition %d' % c)
            assert_close(logvar[c], lv_i[0], 'logvar vs infer, condition %d' % c)


def test_generate_matches_the_reference_fixture(pair, fixture):
    fx, meta = fixture
    _, model = pair
    image, img_row, state, eps = SR.fixture_conditions(fx, meta)
    n, C = eps.shape[0], state.shape[0]
    modes = [m.training for m in model.modules()]
    model.train()
    try:
        out = CS.generate(model, image=image, img_row=img_row, state=state, n_samples=n, eps=eps)
        assert all(m.training for m in model.modules())          # modes restored
    finally:
        for m, mode in zip(model.modules(), modes):
            m.training = mode
    assert tuple(out['image'].shape) == (n, C, 3, 64, 64) and tuple(out['attrs'].shape) == (n, C, 18)
    for c in range(C):
        assert_close(out['mu'][c], fx['mu'][c], 'mu, condition %d' % c)
        assert_close(out['logvar'][c], fx['logvar'][c], 'logvar, condition %d' % c)
        assert_close(out['z'][:, c], fx['z'][:, c], 'z, condition %d' % c)
        assert_close(out['image'].reshape(n, C, -1)[:, c, :256], fx['image256'][:, c], 'image slice, condition %d' % c)
        assert_close(out['attrs'][:, c], fx['attrs'][:, c], 'attribute probabilities, condition %d' % c)


def test_generate_device_draw_and_prior(pair):
    """No conditions: one row, the prior; the device draw is reproducible from its seed and decodes to probabilities."""
    _, model = pair
    a = CS.generate(model, n_samples=3, seed=11)
    b = CS.generate(model, n_samples=3, seed=11)
    c = CS.generate(model, n_samples=3, seed=12)
    assert tuple(a['z'].shape) == (3, 1, model.n_latents) and tuple(a['image'].shape) == (3, 1, 3, 64, 64)
    assert bool((a['mu'] == 0).all()) and bool((a['logvar'] == 0).all())
    assert torch.equal(a['z'], b['z']) and torch.equal(a['image'], b['image']) and not torch.equal(a['z'], c['z'])
    for t in (a['image'], a['attrs']):
        assert torch.isfinite(t).all() and float(t.min()) >= 0 and float(t.max()) <= 1


def test_generate_mean_matches_the_eval_forward(pair):
    """``n_samples=0`` decodes z = mu; on a batch whose rows all share one subset that is the model's own eval-mode
    forward: sigmoid(model(image, attrs))."""
    from oracle import steps as OS
    _, model = pair
    B = 3
    image, label = OS.synthetic_batch('celeba19', B, seed=31)
    subset = (2, 9, 14)
    state = torch.full((B, 18), -1, dtype=torch.int64)
    for a in subset:
        state[:, a] = label[:, a].long()
    out = CS.generate(model, image=image, state=state, n_samples=0)
    assert tuple(out['z'].shape) == (1, B, model.n_latents) and torch.equal(out['z'][0], out['mu'])
    assert tuple(out['image'].shape) == (1, B, 3, 64, 64) and tuple(out['attrs'].shape) == (1, B, 18)
    with torch.no_grad():
        lst = [label[:, a].to(DEV) if a in subset else None for a in range(18)]
        img_logits, attr_logits, mu, logvar = model(image.to(DEV), lst)
    assert_close(out['mu'], mu, 'mean mode: mu')
    assert_close(out['logvar'], logvar, 'mean mode: logvar')
    assert_close(out['attrs'][0], torch.sigmoid(torch.stack(attr_logits, dim=1)), 'mean mode: attribute probabilities')
    assert_close(out['image'][0], torch.sigmoid(img_logits), 'mean mode: image probabilities')


# ----------------------------------------------------------------------------- the command line
@pytest.fixture(scope='module')
def checkpoint(fixture, tmp_path_factory):
    fx, meta = fixture
    oracle = SR.fixture_model(fx, meta)
    path = str(tmp_path_factory.mktemp('celeba19_sample') / 'model_best.pth.tar')
    torch.save({'state_dict': oracle.state_dict(), 'n_latents': meta['n_latents']}, path)
    return path


def run_cli(args, timeout=300):
    script = os.path.join(ROOT, 'multimodal-vae-public_amd', 'celeba19', 'sample.py')
    return subprocess.run([sys.executable, script] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def png_size(path):
    with open(path, 'rb') as f:
        head = f.read(24)
    assert head[:8] == b'\x89PNG\r\n\x1a\n'
    return struct.unpack('>II', head[16:24])          # (width, height)


def test_cli_condition_on_attrs(checkpoint, tmp_path):
    out = run_cli([checkpoint, '--cuda', '--condition-on-attrs', 'Male=1,Eyeglasses=0', '--n-samples', '4', '--out-dir',
                   str(tmp_path)])
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert png_size(os.path.join(str(tmp_path), 'sample_image.png')) == (4 * 66 + 2, 66 + 2)
    lines = open(os.path.join(str(tmp_path), 'sample_attrs.txt')).read().split('\n')
    assert len(lines) == 5 and lines[4] == ''
    for line in lines[:4]:
        assert all(name in CS.ATTRIBUTES for name in line.split(',') if name)
    assert not os.path.exists(os.path.join(str(tmp_path), 'sweep_attrs.txt'))


def test_cli_sweep(checkpoint, tmp_path):
    out = run_cli([checkpoint, '--cuda', '--sweep', '--n-samples', '2', '--out-dir', str(tmp_path)])
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert png_size(os.path.join(str(tmp_path), 'sample_image.png')) == (2 * 66 + 2, 37 * 66 + 2)       # one grid row per condition
    assert len(open(os.path.join(str(tmp_path), 'sample_attrs.txt')).read().splitlines()) == 37 * 2
    lines = open(os.path.join(str(tmp_path), 'sweep_attrs.txt')).read().splitlines()
    assert len(lines) == 37
    assert [ln.split()[0] for ln in lines] == CS.sweep_labels()
    for ln in lines:
        probs = [float(v) for v in ln.split()[1:]]
        assert len(probs) == 18 and all(0.0 <= p <= 1.0 for p in probs)


def test_cli_without_cuda_names_the_flag(checkpoint, tmp_path):
    out = run_cli([checkpoint, '--n-samples', '2', '--out-dir', str(tmp_path)])
    assert out.returncode != 0 and '--cuda' in out.stderr
    assert not os.listdir(str(tmp_path))
