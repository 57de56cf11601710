"""CPU: label prediction (predict.py, K28).  The new symbols are exported with the declared arity and the ABI version did
not move; the two C entry points and ``predict`` / ``evaluate`` refuse bad arguments before any launch; the float64
restatement (tests/predict_ref.py) checks itself against closed forms; the score cases of tests/test_predict_gpu.py keep
their arg-max margins."""
import ctypes
import importlib
import math
import os
import re

import pytest
import torch

import mvae_amd
from mvae_amd import _lib, kernels as K
import predict_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = importlib.import_module('mvae_amd.predict')
CAT, BERN = 0, 1


# ----------------------------------------------------------------------------- the ABI
def test_symbols_are_exported_with_the_declared_arity():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read(), flags=re.S)
    for name, arity in (('mvae_predict_fold', 11), ('mvae_predict_score', 11)):
        assert hasattr(handle, name), '%s is not exported' % name
        m = re.search(r'\bint\s+%s\s*\(([^;{]*?)\)\s*;' % name, text, flags=re.S)
        assert m, '%s is not declared in include/mvae_hip.h' % name
        assert m.group(1).count(',') + 1 == arity == len(_lib._SIGNATURES[name][1])
    assert handle.mvae_abi_version() == 6
    header = open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read()
    assert int(re.search(r'#define\s+MVAE_PREDICT_MAX_C\s+(\d+)', header).group(1)) == _lib.PREDICT_MAX_C == 64
    assert int(re.search(r'#define\s+MVAE_PREDICT_CATEGORICAL\s+(\d+)', header).group(1)) == _lib.PREDICT_CATEGORICAL == CAT
    assert int(re.search(r'#define\s+MVAE_PREDICT_BERNOULLI\s+(\d+)', header).group(1)) == _lib.PREDICT_BERNOULLI == BERN
    assert callable(K.predict_fold) and callable(K.predict_score) and callable(K.fresh_predict_state)
    assert mvae_amd.predict is P and mvae_amd.predict_label is P.predict and mvae_amd.evaluate is P.evaluate


def test_predict_fold_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)

    def fold(R=6, B=3, C=4, rs=None, cs=1, mode=CAT, logits=p, state=p, out=p, finish=0):
        return lib.mvae_predict_fold(logits, C * cs if rs is None else rs, cs, R, B, C, mode, state, out, finish, None)
    assert fold(logits=None) == -1 and fold(state=None) == -1                       # null pointers
    for R, B, C in ((0, 3, 4), (6, 0, 4), (6, 3, 0), (-6, 3, 4), (6, -3, 4), (6, 3, -4)):
        assert fold(R=R, B=B, C=C) == -1, (R, B, C)
    assert fold(R=7, B=3) == -1                                                      # R % B != 0
    assert fold(C=65) == -1                                                          # above MVAE_PREDICT_MAX_C
    assert fold(mode=2) == -1 and fold(mode=-1) == -1
    assert fold(rs=3, cs=1) == -1                                                    # rows overlap: 4 columns in a stride of 3
    assert fold(rs=1, cs=5) == -1                                                    # [C, R] layout with 6 rows in a stride of 5
    assert fold(rs=0) == -1 and fold(cs=0) == -1 and fold(rs=-4) == -1 and fold(cs=-1) == -1
    assert fold(rs=2, cs=2) == -1
    assert fold(finish=-1) == -1
    assert fold(finish=2, out=None) == -1                                            # finish needs somewhere to write
    assert fold(R=1 << 26, B=1 << 10, C=32) == -1                                    # R * C = 2^31
    for mode in (CAT, BERN):                                                         # the same for the Bernoulli mode
        assert fold(mode=mode, R=7, B=3) == -1 and fold(mode=mode, logits=None) == -1


def test_predict_score_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)

    def score(B=3, C=4, mode=CAT, logp=p, targets=p, ldt=4, pred=p, nll=p, correct=p, confusion=p):
        return lib.mvae_predict_score(logp, mode, targets, ldt, B, C, pred, nll, correct, confusion, None)
    assert score(logp=None) == -1 and score(pred=None) == -1
    assert score(nll=None) == -1 and score(correct=None) == -1                       # targets want both
    assert score(targets=None) == -1                                                 # outputs of a score without targets
    assert score(targets=None, nll=None, correct=None) == -1                         # ... the table included
    for B, C in ((0, 4), (3, 0), (-3, 4), (3, -4), (3, 65)):
        assert score(B=B, C=C) == -1, (B, C)
    assert score(mode=2) == -1
    assert score(mode=BERN, ldt=3) == -1                                             # a target row shorter than C
    assert score(B=1 << 26, C=32) == -1                                              # B * C = 2^31


# ----------------------------------------------------------------------------- the Python surface
def test_predict_and_evaluate_refuse_before_any_launch():
    m = mvae_amd.mnist.model.MVAE(8)
    image, label = torch.rand(2, 1, 28, 28), torch.tensor([1, 2])
    with pytest.raises(ValueError, match='expected one of'):
        P.predict(torch.nn.Linear(2, 2), image)                                      # unknown kind
    with pytest.raises(RuntimeError, match='GPU'):
        P.predict(m, image)                                                          # a model on the CPU
    with pytest.raises(RuntimeError, match='GPU'):
        P.evaluate(m, image, label)
    with pytest.raises(ValueError, match='n_samples'):
        P.predict(m, image, n_samples=-1)
    with pytest.raises(ValueError, match='eps'):
        P.predict(m, image, n_samples=3, eps=torch.zeros(3, 2, 9))
    with pytest.raises(ValueError, match='eps'):
        P.predict(m, image, n_samples=0, eps=torch.zeros(0, 2, 8))
    with pytest.raises(ValueError, match='no label'):
        P.evaluate(m, image)
    with pytest.raises(ValueError, match='no label'):
        P.predict(m, image, given=('image', 'label'))
    with pytest.raises(ValueError, match='unknown modality'):
        P.predict(m, image, given=('pixels',))
    with pytest.raises(ValueError, match='at least one'):
        P.predict(m, image, given=())
    with pytest.raises(ValueError, match='chunk_rows'):
        P.predict(m, image, chunk_rows=0)
    with pytest.raises(ValueError, match='label of 2 mnist data'):
        P.evaluate(m, image, torch.zeros(2, 18))
    with pytest.raises(ValueError, match='confusion'):
        P.evaluate(m, image, label, confusion=torch.zeros(10, 10))
    c19 = mvae_amd.celeba19.model.MVAE(8)
    with pytest.raises(ValueError, match='unknown modality'):
        P.predict(c19, torch.rand(2, 3, 64, 64), given=('image', 'Beard'))
    with pytest.raises(ValueError, match='no label'):
        P.predict(c19, torch.rand(2, 3, 64, 64), given=('image', 'Male'))
    with pytest.raises(RuntimeError, match='GPU'):
        P.predict(c19, torch.rand(2, 3, 64, 64), given=('image', 'Male'), label=torch.zeros(2, 18))
    assert m.training and c19.training                                               # a refused call leaves the model alone


def test_kernel_wrappers_refuse_host_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match='GPU'):
        K.predict_fold(torch.zeros(6, 4), 3, 'categorical', torch.zeros(3, 4, 2))
    with pytest.raises(RuntimeError, match='mode'):
        K.predict_fold(torch.zeros(6, 4), 3, 'softmax', torch.zeros(3, 4, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        K.predict_score(torch.zeros(3, 4), 'categorical', torch.zeros(3, dtype=torch.int64))
    st = K.fresh_predict_state(3, 4, 'bernoulli', 'cpu')
    assert st.shape == (3, 4, 2, 2) and (st[..., 0] == float('-inf')).all() and (st[..., 1] == 0).all()
    assert K.fresh_predict_state(3, 4, 'categorical', 'cpu').shape == (3, 4, 2)


def test_drop_ins_exist_for_every_kind():
    for kind in P.KINDS:
        path = os.path.join(ROOT, 'multimodal-vae-public_amd', kind, 'predict.py')
        assert os.path.exists(path), path
        assert "main('%s', load_checkpoint" % kind in open(path).read()


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('Kt', [1, 2, 7, 64])
def test_restatement_identical_samples_give_log_softmax(Kt):
    x = PR.fold_inputs(1, 5, 10, 3.0)                                                # [5, 10]
    rows = x.repeat(Kt, 1)                                                           # the same 5 rows K times, sample-major
    want = torch.log_softmax(x.double(), dim=1)
    assert torch.allclose(PR.fold_categorical(rows, 5), want, rtol=1e-13, atol=1e-13)
    got = PR.fold_bernoulli(rows, 5)
    assert torch.allclose(got[..., 0], torch.log(torch.sigmoid(x.double())), rtol=1e-12, atol=1e-12)
    assert torch.allclose(got[..., 1], torch.log(torch.sigmoid(-x.double())), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('Kc,B,C', PR.FOLD_SHAPES_CAT)
@pytest.mark.parametrize('scale', PR.SCALES)
def test_restatement_categorical_rows_sum_to_one(Kc, B, C, scale):
    logp = PR.fold_categorical(PR.fold_inputs(Kc, B, C, scale), B)
    assert logp.shape == (B, C) and logp.dtype == torch.float64
    assert torch.allclose(logp.exp().sum(1), torch.ones(B, dtype=torch.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize('scale', PR.SCALES)
def test_restatement_bernoulli_classes_sum_to_one(scale):
    Kc, B, C = PR.FOLD_SHAPE_BERN
    logp = PR.fold_bernoulli(PR.fold_inputs(Kc, B, C, scale), B)
    assert logp.shape == (B, C, 2)
    assert torch.allclose(logp.exp().sum(2), torch.ones(B, C, dtype=torch.float64), rtol=1e-12, atol=0)


def test_restatement_is_a_mean_in_the_probability_domain():
    x = PR.fold_inputs(6, 3, 4, 1.0)
    want = torch.softmax(x.double(), dim=1).view(6, 3, 4).mean(0).log()
    assert torch.allclose(PR.fold_categorical(x, 3), want, rtol=1e-12, atol=1e-12)


def test_restatement_score():
    logp = torch.tensor([[0.1, 0.7, 0.2], [0.5, 0.25, 0.25], [0.3, 0.3, 0.4], [0.2, 0.6, 0.2]], dtype=torch.float64).log()
    y = torch.tensor([1, 2, 2, 7])                                                   # the last target is out of range
    pred, nll, correct, conf = PR.score_categorical(logp, y)
    assert pred.tolist() == [1, 0, 2, 1] and correct.tolist() == [True, False, True, False]
    assert torch.allclose(nll[:3], -torch.tensor([0.7, 0.25, 0.4], dtype=torch.float64).log()) and math.isinf(nll[3].item())
    assert conf.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 1]] and conf.sum().item() == 3
    tie = torch.tensor([[0.4, 0.4, 0.2]], dtype=torch.float64).log()
    assert PR.score_categorical(tie, torch.tensor([0]))[0].item() == 0              # the lowest index on a tie
    lb = torch.tensor([[[0.8, 0.2], [0.3, 0.7]]], dtype=torch.float64).log()         # [1, 2, 2]
    pred, nll, correct, conf = PR.score_bernoulli(lb, torch.tensor([[1.0, 1.0]]))
    assert pred.tolist() == [[1, 0]] and correct.tolist() == [[True, False]]
    assert torch.allclose(nll, -torch.tensor([[0.8, 0.3]], dtype=torch.float64).log())
    assert conf.tolist() == [[[0, 0], [0, 1]], [[0, 0], [1, 0]]]


@pytest.mark.parametrize('B,mode', [(1, 'categorical'), (7, 'categorical'), (300, 'categorical'), (7, 'bernoulli'),
                                    (300, 'bernoulli')])
def test_score_cases_keep_their_margins(B, mode):
    _, _, logp = PR.score_case(B, mode)
    worst = PR.margin(logp, mode).min().item()
    assert worst > PR.MARGIN, '%s B = %d: margin %.3e' % (mode, B, worst)
