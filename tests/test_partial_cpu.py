"""CPU: the host side of weak supervision -- ``partial.plan`` on hand-written presence patterns, the paired subset of
``--n-paired``, the parsers' defaults, and the new entry points' argument checks (no launch: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import mvae_amd
from mvae_amd import _lib, partial as P
from mvae_amd.train_common import reference_parser

import partial_ref as PR

MIXED = [3, 1, 1, 3, 2, 1, 3]


def check_inverses(pl):
    """slot, row_of and erow invert one another; the compact order is [image-only | joint | label-only], ascending in b."""
    B, R = pl.B, pl.R
    assert pl.slot.shape == (3, B) and pl.row_of.shape == (R,) and pl.erow.shape == (2, B)
    assert pl.slot.dtype == pl.row_of.dtype == pl.erow.dtype == np.int32
    assert sorted(pl.slot[pl.slot >= 0].tolist()) == list(range(R))        # every compact row owned exactly once
    for t in range(3):
        for b in range(B):
            if pl.slot[t, b] >= 0:
                assert pl.row_of[pl.slot[t, b]] == b
    bounds = [0, pl.n_img, pl.n_img + pl.n_joint, R]
    for term, (lo, hi) in zip((1, 0, 2), zip(bounds[:-1], bounds[1:])):    # image-only, joint, label-only
        rows = pl.row_of[lo:hi]
        assert (np.diff(rows) > 0).all(), 'not stable in b'
        assert (pl.slot[term, rows] == np.arange(lo, hi)).all()
        assert int((pl.slot[term] >= 0).sum()) == hi - lo
    assert pl.image_slice == (0, pl.n_img + pl.n_joint) and pl.label_slice == (pl.n_img, R)
    for e in range(2):
        rows = pl.expert_rows[e]
        assert (pl.erow[e, rows] == np.arange(rows.size)).all() and int((pl.erow[e] >= 0).sum()) == rows.size
        assert (rows == np.flatnonzero(pl.present & (1 << e))).all()
    # every term's experts exist on the rows the term is active on
    for t, mask in enumerate(P.TERM_MASKS):
        for e in range(2):
            if (mask >> e) & 1:
                assert (pl.erow[e, pl.slot[t] >= 0] >= 0).all()


def test_plan_mixed_pattern():
    pl = P.plan(MIXED)
    assert pl.n == [3, 6, 4] and (pl.n_joint, pl.n_img, pl.n_lbl) == (3, 6, 4) and pl.R == 13
    assert pl.row_of.tolist() == [0, 1, 2, 3, 5, 6, 0, 3, 6, 0, 3, 4, 6]
    assert pl.slot.tolist() == [[6, -1, -1, 7, -1, -1, 8], [0, 1, 2, 3, -1, 4, 5], [9, -1, -1, 10, 11, -1, 12]]
    assert pl.erow.tolist() == [[0, 1, 2, 3, -1, 4, 5], [0, -1, -1, 1, 2, -1, 3]]
    assert pl.image_slice == (0, 9) and pl.label_slice == (6, 13)
    check_inverses(pl)
    for got, want in zip(PR.term_rows(MIXED, None), ([0, 3, 6], [0, 1, 2, 3, 5, 6], [0, 3, 4, 6])):
        assert got.tolist() == want


@pytest.mark.parametrize('present,paired,n', [
    ([3, 3, 3, 3], None, [4, 4, 4]),                 # all rows paired: the reference's step
    ([1, 1, 1], None, [0, 3, 0]),                    # image-only everywhere: two empty terms
    ([3], None, [1, 1, 1]), ([2], None, [0, 0, 1]),  # B = 1
    ([3, 3, 1], [1, 0, 1], [1, 3, 2]),               # a both-present row that is not paired
    (torch.tensor([2, 3, 1, 2]), torch.tensor([0, 1, 0, 1]), [1, 2, 3]),
])
def test_plan_patterns(present, paired, n):
    pl = P.plan(present, paired)
    assert pl.n == n and pl.R == sum(n)
    check_inverses(pl)
    if pl.n_joint == pl.B:
        assert pl.row_of.tolist() == list(range(pl.B)) * 3
        assert (pl.erow == np.arange(pl.B)).all()


def test_plan_refuses_what_it_cannot_lay_out():
    with pytest.raises(ValueError, match='row 2 observes no modality'):
        P.plan([3, 1, 0, 2])
    with pytest.raises(ValueError, match='bits beyond'):
        P.plan([3, 4])
    with pytest.raises(ValueError, match='paired has 1 entries for 2 rows'):
        P.plan([3, 3], [1])
    with pytest.raises(ValueError, match='empty batch'):
        P.plan(np.zeros(0, dtype=np.int32))
    with pytest.raises(ValueError, match='1-D integer'):
        P.plan([1.0, 3.0])


def test_plan_upload_is_one_buffer():
    pl = P.plan(MIXED)
    tb = pl.to('cpu')
    base = tb.slot.untyped_storage().data_ptr()
    for t in (tb.row_of, tb.erow, tb.expert_rows[0], tb.expert_rows[1], tb.masks):
        assert t.untyped_storage().data_ptr() == base and t.dtype == torch.int32 and t.is_contiguous()
    assert tb.slot.tolist() == pl.slot.tolist() and tb.erow.tolist() == pl.erow.tolist()
    assert tb.row_of.tolist() == pl.row_of.tolist() and tb.masks.tolist() == [3, 1, 2] and (tb.R, tb.B) == (13, 7)
    assert tb.expert_rows[1].tolist() == [0, 3, 4, 6]


def test_paired_subset_and_flags():
    a = P.paired_subset(1000, 37, seed=5)
    assert a.dtype == bool and a.shape == (1000,) and int(a.sum()) == 37
    assert (P.paired_subset(1000, 37, seed=5) == a).all()             # the same in every epoch / for the same seed
    assert (P.paired_subset(1000, 37, seed=6) != a).any()
    assert int(P.paired_subset(10, 0, 1).sum()) == 0 and bool(P.paired_subset(10, 10, 1).all())
    with pytest.raises(ValueError, match='outside 0..10'):
        P.paired_subset(10, 11, 0)
    flag = np.array([True, False, True])
    present, paired = P.batch_flags(flag, 'keep')
    assert present.tolist() == [3, 3, 3] and paired.tolist() == [1, 0, 1] and P.plan(present, paired).n == [2, 3, 3]
    present, paired = P.batch_flags(flag, 'drop')
    assert present.tolist() == [3, 1, 3] and paired.tolist() == [1, 1, 1] and P.plan(present, paired).n == [2, 3, 2]
    with pytest.raises(ValueError, match='keep'):
        P.batch_flags(flag, 'both')
    s = P.synthetic_flags(8, 0.5, 3, 1)
    assert int(s.sum()) == 4 and (P.synthetic_flags(8, 0.5, 3, 1) == s).all()
    assert any((P.synthetic_flags(8, 0.5, 3, i) != s).any() for i in range(2, 6))
    assert int(P.synthetic_flags(8, 0.0, 3, 0).sum()) == 0 and int(P.synthetic_flags(8, 1.0, 3, 0).sum()) == 8


@pytest.mark.parametrize('kind', ['mnist', 'fashionmnist'])
def test_parsers_keep_their_defaults_without_n_paired(kind):
    ns = reference_parser(kind).parse_args([])
    assert ns.n_paired is None and ns.paired_seed == 0 and ns.unpaired_labels == 'keep'
    assert (ns.n_latents, ns.batch_size, ns.epochs, ns.annealing_epochs, ns.lr, ns.log_interval, ns.lambda_image,
            ns.lambda_text, ns.cuda, ns.synthetic, ns.steps_per_epoch, ns.no_graph) == (
                64, 100, 500, 200, 1e-3, 10, 1.0, 10.0, False, False, 100, False)
    ns = reference_parser(kind).parse_args(['--n-paired', '100', '--paired-seed', '7', '--unpaired-labels', 'drop'])
    assert (ns.n_paired, ns.paired_seed, ns.unpaired_labels) == (100, 7, 'drop')
    with pytest.raises(SystemExit):
        reference_parser(kind).parse_args(['--unpaired-labels', 'maybe'])


@pytest.mark.parametrize('kind', ['celeba', 'celeba19', 'multimnist'])
def test_out_of_scope_parsers_do_not_grow_the_flag(kind):
    with pytest.raises(SystemExit):
        reference_parser(kind).parse_args(['--n-paired', '10'])


def test_partial_step_refuses_models_with_batchnorm_or_dropout():
    with pytest.raises(ValueError, match='without BatchNorm'):
        P.PartialStep(mvae_amd.celeba.model.MVAE(8))


def test_new_entry_points_refuse_bad_arguments_on_the_host():
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ex, gr = _lib.Experts(), _lib.ExpertGrads()
    ex.mu[0] = ex.logvar[0] = gr.dmu[0] = gr.dlogvar[0] = p.value
    n1, n0, big = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(3)

    def fwd(E=1, n=n1, T=1, R=1, draw=0, noise=p, counter=None, B=2, D=4, ld=4, variant=0, mu=p):
        return lib.mvae_poe_ragged_fwd(ctypes.byref(ex), ld, E, n, p, p, T, p, R, noise, draw, 1, counter, 0, mu, p, p, p,
                                       B, D, variant, None)
    assert fwd(E=0) == -1 and fwd(E=33) == -1 and fwd(T=0) == -1 and fwd(T=41) == -1 and fwd(R=-1) == -1
    assert fwd(B=0) == -1 and fwd(D=0) == -1 and fwd(ld=3) == -1 and fwd(variant=2) == -1 and fwd(mu=None) == -1
    assert fwd(n=big) == -1                         # more expert rows than batch rows
    assert fwd(draw=1) == -1                        # a draw without its counter
    assert fwd(R=0) == 0 and fwd(R=0, n=n0) == 0    # nothing active: no launch

    def bwd(E=1, n=n1, R=1, ldg=4, grads=gr):
        return lib.mvae_poe_ragged_bwd(ctypes.byref(ex), 4, E, n, p, p, 1, p, R, p, p, p, p, None, None, None,
                                       ctypes.byref(grads), ldg, 2, 4, 0, None)
    assert bwd(E=0) == -1 and bwd(ldg=3) == -1 and bwd(R=-1) == -1 and bwd(grads=_lib.ExpertGrads()) == -1
    assert bwd(n=n0) == 0                           # no expert row exists: nothing to write
    assert lib.mvae_bce_rows_indexed_fwd(p, p, None, None, p, None, 2, 4, 2, None) == -1
    assert lib.mvae_bce_rows_indexed_fwd(p, p, p, None, None, None, 2, 4, 2, None) == -1
    assert lib.mvae_bce_rows_indexed_bwd(p, p, p, None, None, 2, 4, 2, None) == -1
    assert lib.mvae_bce_rows_indexed_bwd(p, p, p, None, p, 0, 4, 2, None) == -1
    assert lib.mvae_ce_rows_indexed_fwd(p, p, p, None, p, None, 2, 1025, 2, None) == -1
    assert lib.mvae_ce_rows_indexed_fwd(p, p, p, None, None, None, 2, 10, 2, None) == -1
    assert lib.mvae_ce_rows_indexed_bwd(p, None, p, None, p, 2, 10, 2, None) == -1
    assert lib.mvae_ce_rows_indexed_bwd(p, p, p, None, p, 2, 10, 0, None) == -1
