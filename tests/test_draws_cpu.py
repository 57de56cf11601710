"""CPU: the host helpers the evaluation paths share (mvae_amd.draws) -- the chunk schedule of the K draws, the eval-mode
guard and the ``score`` / ``given`` name resolution with each caller's wording."""
import pytest
import torch

from mvae_amd import draws as DR
from mvae_amd import loglike as LL
from mvae_amd.celeba19 import loglike as CL
from mvae_amd.vision import loglike as VL


def test_chunks_cover_the_draws_and_finish_on_the_last_chunk_only():
    assert list(DR.chunks(7, 2)) == [(0, 0, 2, 0), (1, 2, 2, 0), (2, 4, 2, 0), (3, 6, 1, 7)]
    assert list(DR.chunks(5, 5)) == [(0, 0, 5, 5)]
    assert list(DR.chunks(5, 9)) == [(0, 0, 5, 5)]              # Kc > n_samples: the same single chunk
    assert list(DR.chunks(1, 1)) == [(0, 0, 1, 1)]
    assert list(DR.chunks(6, 3)) == [(0, 0, 3, 0), (1, 3, 3, 6)]


def _flags(model):
    return [m.training for m in model.modules()]


def test_eval_mode_restores_every_flag_also_when_the_body_raises():
    model = torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Dropout(), torch.nn.Sequential(torch.nn.Linear(2, 2)))
    model.train()
    model[1].eval()                                             # one child already in eval mode
    before = _flags(model)
    assert before == [True, True, False, True, True]
    with DR.eval_mode(model):
        assert not any(_flags(model)) and not torch.is_grad_enabled()
    assert _flags(model) == before and torch.is_grad_enabled()
    with pytest.raises(KeyError):
        with DR.eval_mode(model):
            assert not any(_flags(model))
            raise KeyError('body')
    assert _flags(model) == before and torch.is_grad_enabled()


def test_names_follow_the_modality_order_and_expand_aliases():
    assert LL._names(('label', 'image'), 'score') == ('image', 'label')
    assert LL._names('label', 'given') == ('label',)
    assert VL._names(None, 'score', VL.MODALITIES[:2]) == VL.MODALITIES[:2]
    assert VL._names(tuple(reversed(VL.MODALITIES)), 'given', ()) == VL.MODALITIES
    assert VL._names(VL.MODALITIES[3], 'score', ()) == (VL.MODALITIES[3],)
    assert CL._names('attrs', 'score', ()) == CL.ATTRIBUTES
    assert CL._names(('Smiling', 'image', 'Male'), 'score', ()) == ('image', 'Male', 'Smiling')
    assert CL._names(('attrs', 'image'), 'given', ()) == CL.MODALITIES
    assert DR.names(('b', 'x'), 'score', ('a', 'b', 'c'), 'who', aliases={'x': ('c', 'a')}) == ('a', 'b', 'c')


def test_names_refuse_with_each_callers_wording():
    with pytest.raises(ValueError) as e:
        LL._names(('image', 'pixels'), 'score')
    assert str(e.value) == "log_likelihood: unknown modality 'pixels' in `score` (use 'image' and / or 'label')"
    with pytest.raises(ValueError) as e:
        LL._names((), 'given')
    assert str(e.value) == 'log_likelihood: `given` must name at least one modality'
    with pytest.raises(ValueError) as e:
        VL._names('label', 'given', ())
    assert str(e.value) == ("vision log_likelihood: unknown modality 'label' in `given` (the modalities are %s)"
                            % ', '.join(VL.MODALITIES))
    with pytest.raises(ValueError) as e:
        VL._names(None, 'score', ())
    assert str(e.value) == 'vision log_likelihood: `score` must name at least one modality'
    with pytest.raises(ValueError) as e:
        CL._names('Beard', 'score', ())
    assert str(e.value) == ("celeba19 log_likelihood: unknown modality 'Beard' in `score` (the modalities are %s; 'attrs' "
                            "names the 18 attributes)" % ', '.join(CL.MODALITIES))
    with pytest.raises(ValueError) as e:
        CL._names((), 'given', ())
    assert str(e.value) == 'celeba19 log_likelihood: `given` must name at least one modality'


def test_check_draws_and_require_gpu_word_the_shared_refusals():
    DR.check_draws('f', 1, 1, None, 2, 3)
    DR.check_draws('f', 4, 9, torch.zeros(4, 2, 3), 2, 3)
    with pytest.raises(ValueError) as e:
        DR.check_draws('f', 0, 1, None, 2, 3)
    assert str(e.value) == 'f: n_samples must be at least 1 (got 0)'
    with pytest.raises(ValueError) as e:
        DR.check_draws('f', 1, 0, None, 2, 3)
    assert str(e.value) == 'f: chunk_rows must be at least 1 (got 0)'
    with pytest.raises(ValueError) as e:
        DR.check_draws('f', 4, 1, torch.zeros(4, 2, 5), 2, 3)
    assert str(e.value) == 'f: eps must be [n_samples, B, D] = (4, 2, 3), got (4, 2, 5)'
    with pytest.raises(RuntimeError) as e:
        DR.require_gpu('f', torch.nn.Linear(2, 2))
    assert str(e.value) == 'f: the model must live on the GPU (model.cuda()); the HIP path has no CPU fallback'
    assert VL.fresh_state is DR.fresh_state and VL.report is DR.report
    state = DR.fresh_state(3, 2, 'cpu')
    assert state.shape == (3, 2, 2) and bool((state[..., 0] == float('-inf')).all()) and bool((state[..., 1] == 0).all())
