"""CPU: the host side of celeba19/sample.py -- the float64 restatement (tests/celeba19_sample_ref.py) against the fixture
written from the reference (tests/golden/make_celeba19_sample_golden.py), ``parse_conditions`` / ``sweep_states``, and
every refusal of ``parse_conditions``, of ``generate``'s host checks and of ``kernels.poe_table_check``: all of them are
raised before a device is needed."""
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib, kernels as K
from mvae_amd.celeba19 import model as CM, sample as CS
import celeba19_sample_ref as SR
from util import assert_close, load_golden

D = 100


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return load_golden(golden_dir, 'celeba19_sample')


def test_restatement_reproduces_the_reference_fixture(fixture):
    """Six conditions, each run by the reference as a batch of 1 through ``infer``; the restatement runs them as one
    batch of condition rows on the oracle."""
    fx, meta = fixture
    oracle = SR.fixture_model(fx, meta)
    image, img_row, state, eps = SR.fixture_conditions(fx, meta)
    assert tuple(state.shape) == (6, 18) and tuple(eps.shape) == (meta['n_draws'], 6, D) and image.shape[0] == meta['rows']
    # the six kinds of condition the fixture promises
    present = (state >= 0).sum(1).tolist()
    assert present[0] == 0 and img_row[0] >= 0                                   # image only
    assert present[1] == 1 and int(state[1].max()) == 0 and img_row[1] < 0       # one attribute at 0
    assert present[2] == 1 and int(state[2].max()) == 1 and img_row[2] < 0       # one attribute at 1
    assert present[3] == 18 and img_row[3] >= 0                                  # image plus all 18
    assert 1 < present[4] < 18 and img_row[4] < 0 and 1 < present[5] < 18 and img_row[5] >= 0
    assert int(img_row[5]) == int(img_row[0])                                    # two conditions share an image row
    out = SR.generate(oracle, image, img_row, state, eps)
    n, C = eps.shape[0], 6
    for c in range(C):
        assert_close(out['mu'][c], fx['mu'][c], 'mu, condition %d' % c)
        assert_close(out['logvar'][c], fx['logvar'][c], 'logvar, condition %d' % c)
        assert_close(out['z'][:, c], fx['z'][:, c], 'z, condition %d' % c)
        assert_close(out['image'].reshape(n, C, -1)[:, c, :256], fx['image256'][:, c], 'image slice, condition %d' % c)
        assert_close(out['attrs'][:, c], fx['attrs'][:, c], 'attribute probabilities, condition %d' % c)


def test_restatement_prior_row_is_the_standard_normal():
    """Nothing present: T = 1 / (1 + 1e-8), mu = 0 and logvar = log(1 + 1e-8) = 1e-8 in float64."""
    table = torch.randn(18, 2, 2 * D, generator=torch.Generator().manual_seed(1))
    eps = torch.randn(3, 1, D, generator=torch.Generator().manual_seed(2))
    mu, logvar, z = SR.poe_table(table, torch.full((1, 18), -1), eps=eps)
    assert float(mu.abs().max()) == 0.0
    assert float((logvar - 1e-8).abs().max()) < 1e-15
    assert float((z - eps.double()).abs().max()) < 1e-7


def test_restatement_matches_the_oracle_infer():
    """``poe_table`` on the oracle's table equals ``oracle.infer`` with the same modalities (float32, CPU)."""
    from oracle import models as OM, steps as OS
    oracle = OM.fill_parameters(OM.Celeba19MVAE(D), 11).eval()
    image, label = OS.synthetic_batch('celeba19', 1, seed=5)
    state = torch.full((1, 18), -1, dtype=torch.int64)
    for a in (2, 9, 13):
        state[0, a] = int(label[0, a])
    with torch.no_grad():
        heads = torch.cat(oracle.image_encoder(image), dim=1)
        mu_o, lv_o = oracle.infer(image, [label[:, a] if state[0, a] >= 0 else None for a in range(18)])
    mu, logvar, _ = SR.poe_table(SR.oracle_table(oracle), state, heads, torch.tensor([0]))
    assert_close(mu, mu_o, 'mu vs oracle.infer')
    assert_close(logvar, lv_o, 'logvar vs oracle.infer')


# ----------------------------------------------------------------------------- parse_conditions / sweep_states
def test_parse_conditions():
    names = CS.ATTRIBUTES
    assert len(names) == 18 and 'Male' in names and 'Eyeglasses' in names
    row = CS.parse_conditions('Male=1,Eyeglasses=0')
    assert len(row) == 18 and row[names.index('Male')] == 1 and row[names.index('Eyeglasses')] == 0
    assert sum(v != -1 for v in row) == 2
    assert CS.parse_conditions('Smiling') == CS.parse_conditions('Smiling=1') == CS.parse_conditions(' %d = 1 ' % names.index('Smiling'))
    assert CS.parse_conditions('0=0,17')[0] == 0 and CS.parse_conditions('0=0,17')[17] == 1
    assert CS.parse_conditions('') == CS.parse_conditions(None) == [-1] * 18


@pytest.mark.parametrize('spec,what', [('Male=1,Male=0', 'twice'), ('Male,9', 'twice'), ('Beard=1', 'unknown attribute'),
                                       ('18=1', 'unknown attribute'), ('-1=1', 'unknown attribute'),
                                       ('Male=2', 'must be 0 or 1'), ('Male=', 'must be 0 or 1'),
                                       ('Male=yes', 'must be 0 or 1'), ('Male=-1', 'must be 0 or 1')])
def test_parse_conditions_refusals(spec, what):
    with pytest.raises(ValueError, match=what) as err:
        CS.parse_conditions(spec)
    for name in CS.ATTRIBUTES:                     # every refusal lists the 18 names
        assert name in str(err.value)


def test_sweep_states():
    state = CS.sweep_states()
    assert tuple(state.shape) == (37, 18) and state.dtype == torch.int8
    assert bool((state[0] == -1).all())
    for r in range(1, 37):
        a, v = divmod(r - 1, 2)
        assert int((state[r] != -1).sum()) == 1 and int(state[r, a]) == v
    labels = CS.sweep_labels()
    assert len(labels) == 37 and labels[0] == 'prior' and labels[1] == CS.ATTRIBUTES[0] + '=0' and labels[36] == CS.ATTRIBUTES[17] + '=1'


# ----------------------------------------------------------------------------- generate: host checks
@pytest.fixture(scope='module')
def cpu_model():
    return CM.MVAE(D)


def _img(rows):
    return torch.zeros(rows, 3, 64, 64)


@pytest.mark.parametrize('kw,what', [
    (dict(state=torch.zeros(2, 17, dtype=torch.int64)), r'`state` must be \[C >= 1, 18\]'),
    (dict(state=torch.zeros(18, dtype=torch.int64)), r'`state` must be'),
    (dict(state=torch.zeros(0, 18, dtype=torch.int64)), r'`state` must be'),
    (dict(state=torch.full((2, 18), 2)), 'outside'),
    (dict(state=torch.full((2, 18), -2)), 'outside'),
    (dict(state=torch.full((2, 18), 0.5)), 'outside'),
    (dict(state=torch.zeros(2, 18, dtype=torch.bool)), 'outside'),
    (dict(image=torch.zeros(1, 3, 32, 32)), r'`image` must be'),
    (dict(image=torch.zeros(3, 64, 64)), r'`image` must be'),
    (dict(image=_img(1), state=torch.zeros(2, 18, dtype=torch.int64)), 'pass `img_row`'),
    (dict(image=_img(2), img_row=torch.tensor([0, 2]), state=torch.zeros(2, 18, dtype=torch.int64)), r'must lie in \[-1, 2\)'),
    (dict(image=_img(2), img_row=torch.tensor([0, -2]), state=torch.zeros(2, 18, dtype=torch.int64)), r'must lie in'),
    (dict(image=_img(2), img_row=torch.tensor([0]), state=torch.zeros(2, 18, dtype=torch.int64)), 'holds 1 entries for 2'),
    (dict(image=_img(2), img_row=torch.tensor([0.0, 1.0]), state=torch.zeros(2, 18, dtype=torch.int64)), 'integer vector'),
    (dict(img_row=torch.tensor([0, -1]), state=torch.zeros(2, 18, dtype=torch.int64)), 'no `image` was passed'),
    (dict(n_samples=-1), 'n_samples must be at least 0'),
    (dict(n_samples=2, eps=torch.zeros(2, 1, D + 1)), 'eps must be'),
    (dict(n_samples=2, eps=torch.zeros(3, 1, D)), 'eps must be'),
    (dict(n_samples=0, eps=torch.zeros(0, 1, D)), 'eps must be'),
])
def test_generate_refuses_on_the_host(cpu_model, kw, what):
    with pytest.raises(ValueError, match=what):
        CS.generate(cpu_model, **kw)


def test_generate_refuses_other_models_and_a_model_off_the_gpu(cpu_model):
    with pytest.raises(ValueError, match='expected the celeba19 MVAE'):
        CS.generate(mvae_amd.celeba.model.MVAE(D))
    # the last check: everything else about the call is in order
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        CS.generate(cpu_model, image=_img(1), img_row=torch.tensor([0, 0, -1]), state=CS.sweep_states()[:3], n_samples=2)
    modes = [m.training for m in cpu_model.modules()]
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        CS.generate(cpu_model)
    assert modes == [m.training for m in cpu_model.modules()]


# ----------------------------------------------------------------------------- poe_table_draw: host checks
def _table(A=18, d=20):
    return torch.zeros(A, 2, 2 * d)


@pytest.mark.parametrize('args,what', [
    ((_table(), torch.full((3, 18), 2, dtype=torch.int8)), r'state\[0, 0\] = 2 is outside'),
    ((_table(), torch.tensor([[-1] * 18, [0] * 17 + [-2]])), r'state\[1, 17\] = -2 is outside'),
    ((_table(), torch.zeros(3, 17, dtype=torch.int8)), 'state must be an integer tensor'),
    ((_table(), torch.zeros(3, 18)), 'state must be an integer tensor'),
    ((_table(A=_lib.POE_TABLE_MAX_A + 1), torch.zeros(3, _lib.POE_TABLE_MAX_A + 1, dtype=torch.int8)), 'supports 1 to 32 experts'),
    ((torch.zeros(18, 2, 41), torch.zeros(3, 18, dtype=torch.int8)), 'table must be float32'),
    ((torch.zeros(18, 3, 40), torch.zeros(3, 18, dtype=torch.int8)), 'table must be float32'),
    ((_table().double(), torch.zeros(3, 18, dtype=torch.int8)), 'table must be float32'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), None, torch.tensor([0, -1, -1])), 'img_heads is None'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), torch.zeros(2, 40), torch.tensor([0, 2, -1])), r'outside \[-1, 2\)'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), torch.zeros(2, 40), torch.tensor([0, -2, -1])), r'outside \[-1, 2\)'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), torch.zeros(2, 40), torch.tensor([0, 1])), r'HOST integer tensor \[3\]'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), torch.zeros(2, 40), None), 'without img_row'),
    ((_table(), torch.zeros(3, 18, dtype=torch.int8), torch.zeros(2, 44), torch.tensor([0, 1, -1])), 'img_heads must be float32'),
])
def test_poe_table_check_refuses(args, what):
    with pytest.raises(ValueError, match=what):
        K.poe_table_check(*args)


def test_poe_table_check_accepts_and_converts():
    state, img_row = K.poe_table_check(_table(), torch.tensor([[-1] * 18, [1] * 18]), torch.zeros(2, 40), torch.tensor([1, -1]))
    assert state.dtype == torch.int8 and img_row.dtype == torch.int32 and state.tolist()[1] == [1] * 18
    state, img_row = K.poe_table_check(_table(), torch.tensor([[-1] * 18]), None, torch.tensor([-1]))
    assert img_row.tolist() == [-1]


def test_poe_table_draw_refuses_shapes_before_any_launch():
    """Shape mismatches of the outputs and the noise are ValueErrors raised with host tensors: nothing was launched."""
    t, s = _table(), torch.zeros(3, 18, dtype=torch.int8)
    mu = torch.zeros(3, 20)
    with pytest.raises(ValueError, match='mu and logvar must be'):
        K.poe_table_draw(t, s, torch.zeros(3, 21), mu)
    with pytest.raises(ValueError, match=r'z must be \[n >= 1, 3, 20\]'):
        K.poe_table_draw(t, s, mu, mu.clone(), torch.zeros(2, 4, 20))
    with pytest.raises(ValueError, match='eps must have the shape of z'):
        K.poe_table_draw(t, s, mu, mu.clone(), torch.zeros(2, 3, 20), eps=torch.zeros(1, 3, 20))
    with pytest.raises(ValueError, match='eps must have the shape of z'):
        K.poe_table_draw(t, s, mu, mu.clone(), None, eps=torch.zeros(1, 3, 20))
    with pytest.raises(ValueError, match='launch counter'):
        K.poe_table_draw(t, s, mu, mu.clone(), torch.zeros(2, 3, 20))
    with pytest.raises(RuntimeError, match='GPU'):                           # all in order, but host tensors: no fallback
        K.poe_table_draw(t, s, mu, mu.clone(), torch.zeros(2, 3, 20), eps=torch.zeros(2, 3, 20))


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    import ctypes
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(table=p, A=2, state=p, img=None, ld=0, rows=0, img_row=None, eps=p, seed=0, ctr=None, off=0, eps_out=None,
              mu=p, logvar=p, z=p, n=1, C=1, D=4, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mvae_poe_table_draw(*[a[k] for k in ('table', 'A', 'state', 'img', 'ld', 'rows', 'img_row', 'eps', 'seed',
                                                        'ctr', 'off', 'eps_out', 'mu', 'logvar', 'z', 'n', 'C', 'D', 'stream')])
    for bad in (dict(table=None), dict(state=None), dict(mu=None), dict(logvar=None), dict(A=0), dict(A=33), dict(C=0),
                dict(D=0), dict(n=-1), dict(z=None), dict(eps=None), dict(n=8 * 65535 + 1),
                dict(img=p, img_row=None, rows=1, ld=8), dict(img=p, img_row=p, rows=0, ld=8),
                dict(img=p, img_row=p, rows=1, ld=7)):
        assert call(**bad) == -1, bad
