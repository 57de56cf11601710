"""No GPU: which kernel every Linear launch takes (mvae_linear_route / mvae_linear_wgrad_batched_route: the route functions
the launches of csrc/linear.hip themselves switch on).

  * the Linear calls of the four shipped steps (the ``linear_*`` keys of profiles/r06_by_shape.json) keep their kernel, their
    split count and their finish launch -- a threshold that moves takes a whole step onto other code, and only the
    benchmark would notice;
  * every gate of make_plan, g2_plan_for, launch_gemm2s, launch_igemm_impl, wgrad_direct_ok / wgrad_direct_launch,
    wgrad_batched2_launch and linear_dgrad_impl from both sides, two shapes one step apart;
  * the query's own behaviour: the launch's error codes, names for every id, optional out-pointers.
tests/test_linear_routes_gpu.py runs every reachable route at its cheapest ragged shape.

What the query showed that the hand arithmetic of the issue did not:
  * no fused-loss call can split: linear_loss_impl plans with allow_split = false, so its ``splits != 1`` refusal is dead
    code and there is no MVAE_ERR_ARG of that kind to provoke (bad shapes and N > 32 classes are refused);
  * the split caps ``64`` and ``512 when tiles <= 4`` bind on the narrow plan only (one wave group per block, 512 blocks
    aimed at, tiles of 128 columns): five tiles ask for 102 partials and get 64, four get 128, one gets 512 -- the deepest
    Linear split.  The k-grouped 64 x 64 plans aim at 256 blocks: one tile asks for 256, five tiles for 51;
  * the batched keys (``linear_wgrad_batched n layers``) do not record their items' shapes; the batches pinned here are the
    MNIST batches tests/test_kernels_gpu.py and linear_direct.h name.
"""
import ctypes
import json
import os
import re

import pytest

import mvae_amd
from mvae_amd import _lib
from mvae_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS_MIN = K._WS_MIN_BYTES


def scratch(op, M, N, Kd, G=1):
    """What kernels.workspace hands the wrapper of this call: G x mvae_gemm_ws_bytes of the output, at least the floor."""
    I, J, R = {'fwd': (M, N, Kd), 'dgrad': (M, Kd, N), 'wgrad': (N, Kd, M)}[op]
    return max(G * _lib.lib().mvae_gemm_ws_bytes(I, J, R), WS_MIN)


def R(op, M, N, Kd, G=1, **kw):
    if op in ('fwd', 'dgrad', 'wgrad'):
        kw.setdefault('ws_bytes', scratch(op, M, N, Kd, G))
    return K.linear_route(op, M, N, Kd, G=G, **kw)


# ----------------------------------------------------------------------------- the shipped steps
# (key of profiles/r06_by_shape.json) -> (route, partials, finish launch).  Forward form: layers.forward_tape stores pre + act
# for a Linear with a Swish behind it and pre alone for one without (heads, layers in front of a BatchNorm),
# forward_tape_grouped likewise, a statistics-only pass keeps act alone (celeba19's 4608-row Linear(100, 6400)).  The form only
# matters where g2_plan_for's hints apply (>= 1536 tiles): FORMS names it for those four calls; every other call must take the
# same route in all three forms.  Weight gradients: every Linear here has a bias (db asked for).
FORMS = {('fashionmnist', 'linear_fwd M2048 N6272 K512'): 'pre+act',
         ('celeba19', 'linear_fwd M4608 N6400 K100'): 'act',
         ('celeba19', 'linear_fwd_grouped G18 M768 N512 K100'): 'pre+act',
         ('celeba19', 'linear_fwd_grouped G18 M768 N512 K512'): 'pre+act'}
NO = (1, None)
SHIPPED = {
    'mnist': {
        'linear_bce_fwd M1024 N784 K512': ('igs_64x32_k2',) + NO,
        'linear_ce_fwd M1024 N10 K512': ('igs_32x32_k8',) + NO,
        'linear_dgrad M1024 N10 K512': ('dgrad_smalln',) + NO,
        'linear_dgrad M1024 N512 K512': ('g2s_32x64_k4',) + NO,
        'linear_dgrad M1024 N512 K64': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M1024 N784 K512': ('g2s_32x64_k4',) + NO,
        'linear_dgrad M512 N128 K512': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M512 N512 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M1024 N512 K512': ('g2s_32x64_k4',) + NO,
        'linear_fwd M1024 N512 K64': ('g2s_32x64_k4',) + NO,
        'linear_fwd M512 N128 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M512 N512 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M512 N512 K784': ('g2s_32x32_k8',) + NO,
    },
    'fashionmnist': {
        'linear_ce_fwd M2048 N10 K512': ('igs_32x32_k8',) + NO,
        'linear_dgrad M1024 N128 K512': ('g2s_32x64_k4',) + NO,
        'linear_dgrad M1024 N512 K512': ('g2s_32x64_k4',) + NO,
        'linear_dgrad M1024 N512 K6272': ('ig_64x64',) + NO,
        'linear_dgrad M2048 N10 K512': ('dgrad_smalln',) + NO,
        'linear_dgrad M2048 N512 K512': ('ig_64x64', 2, 'finish_few_vec'),
        'linear_dgrad M2048 N512 K64': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M2048 N6272 K512': ('ig_64x128', 4, 'finish_few_vec'),
        'linear_fwd M1024 N128 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M1024 N512 K512': ('g2s_32x64_k4',) + NO,
        'linear_fwd M1024 N512 K6272': ('ig_64x128', 8, 'finish_few_vec'),
        'linear_fwd M2048 N512 K512': ('ig_64x64', 2, 'finish_few_vec'),
        'linear_fwd M2048 N512 K64': ('ig_64x64',) + NO,
        'linear_fwd M2048 N6272 K512': ('gemm2',) + NO,
        'linear_wgrad M1024 N128 K512': ('wgrad_direct_16',) + NO,
        'linear_wgrad M1024 N512 K6272': ('ig_64x64',) + NO,
        'linear_wgrad M2048 N512 K64': ('wgrad_direct_16',) + NO,
        'linear_wgrad M2048 N6272 K512': ('ig_64x64',) + NO,
    },
    'celeba': {
        'linear_bce_fwd M768 N18 K512': ('igs_32x32_k8',) + NO,
        'linear_dgrad M256 N200 K512': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M256 N512 K512': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M256 N512 K6400': ('ig_64x64',) + NO,
        'linear_dgrad M512 N200 K512': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M512 N6400 K100': ('ig_64x64_k4', 16, 'finish_few_vec'),
        'linear_dgrad M768 N18 K512': ('ig_64x64_s',) + NO,
        'linear_dgrad M768 N512 K100': ('g2s_32x32_k8',) + NO,
        'linear_dgrad M768 N512 K512': ('g2s_32x32_k4',) + NO,
        'linear_fwd M256 N200 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M256 N512 K18': ('ig_64x64_s',) + NO,
        'linear_fwd M256 N512 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M256 N512 K6400': ('ig_64x64_k4', 8, 'finish_few_vec'),
        'linear_fwd M256 N6400 K100': ('ig_64x64',) + NO,
        'linear_fwd M512 N200 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd M512 N6400 K100': ('ig_64x64',) + NO,
        'linear_fwd M768 N512 K100': ('g2s_32x32_k4',) + NO,
        'linear_fwd M768 N512 K512': ('g2s_32x32_k4',) + NO,
        'linear_wgrad M256 N512 K6400': ('ig_64x64',) + NO,
        'linear_wgrad M512 N200 K512': ('wgrad_direct_8',) + NO,
        'linear_wgrad M512 N6400 K100': ('wgrad_direct_4',) + NO,
    },
    'celeba19': {
        'linear_dgrad M256 N512 K6400': ('ig_64x64',) + NO,
        'linear_dgrad M256 N6400 K100': ('ig_64x64_k4', 29, 'finish'),
        'linear_dgrad M512 N6400 K100': ('ig_64x64_k4', 16, 'finish_few_vec'),
        'linear_dgrad M768 N200 K512': ('g2s_32x32_k4',) + NO,
        'linear_dgrad_grouped G18 M256 N200 K512': ('ig_64x64',) + NO,
        'linear_dgrad_grouped G18 M256 N512 K512': ('ig_64x64',) + NO,
        'linear_dgrad_grouped G18 M768 N1 K512': ('dgrad_smalln',) + NO,
        'linear_dgrad_grouped G18 M768 N512 K100': ('ig_64x64',) + NO,
        'linear_dgrad_grouped G18 M768 N512 K512': ('ig_64x64',) + NO,
        'linear_fwd M256 N512 K6400': ('ig_64x64_k4', 8, 'finish_few_vec'),
        'linear_fwd M256 N6400 K100': ('ig_64x64',) + NO,
        'linear_fwd M4608 N6400 K100': ('gemm2',) + NO,
        'linear_fwd M512 N6400 K100': ('ig_64x64',) + NO,
        'linear_fwd M768 N200 K512': ('g2s_32x32_k8',) + NO,
        'linear_fwd_grouped G18 M256 N200 K512': ('ig_64x64', 2, 'finish_few_vec'),
        'linear_fwd_grouped G18 M256 N512 K512': ('ig_64x64',) + NO,
        'linear_fwd_grouped G18 M768 N1 K512': ('g2s_64x32_k4',) + NO,
        'linear_fwd_grouped G18 M768 N512 K100': ('gemm2',) + NO,
        'linear_fwd_grouped G18 M768 N512 K512': ('gemm2',) + NO,
        'linear_wgrad M256 N512 K6400': ('ig_64x64',) + NO,
        'linear_wgrad M256 N6400 K100': ('wgrad_direct_4',) + NO,
        'linear_wgrad M512 N6400 K100': ('wgrad_direct_4',) + NO,
        'linear_wgrad M768 N200 K512': ('wgrad_direct_8',) + NO,
        'linear_wgrad_grouped G18 M256 N200 K512': ('ig_64x64',) + NO,
        'linear_wgrad_grouped G18 M256 N512 K512': ('ig_64x64',) + NO,
        'linear_wgrad_grouped G18 M768 N1 K512': ('ig_32x128_s', 3, 'finish_few'),
        'linear_wgrad_grouped G18 M768 N512 K100': ('ig_64x64', 2, 'finish_few_vec'),
        'linear_wgrad_grouped G18 M768 N512 K512': ('ig_64x64',) + NO,
    },
}


def _profile_calls(kind):
    with open(os.path.join(ROOT, 'profiles', 'r06_by_shape.json')) as f:
        table = json.load(f)[kind]
    return sorted(k for k in table if k.startswith('linear_'))


@pytest.mark.parametrize('kind,n_calls', [('mnist', 16), ('fashionmnist', 20), ('celeba', 23), ('celeba19', 28)])
def test_shipped_steps_keep_their_routes(kind, n_calls):
    calls = _profile_calls(kind)
    assert len(calls) == n_calls
    single = [k for k in calls if 'batched' not in k]
    assert sorted(SHIPPED[kind]) == single, 'the table of this test and the profile table name different calls'
    for key in single:
        name, rest = key.split(' ', 1)
        m = re.match(r'(?:G(\d+) )?M(\d+) N(\d+) K(\d+)$', rest)
        G, (M, N, Kd) = int(m.group(1) or 1), map(int, m.groups()[1:])
        op = name[len('linear_'):].replace('_grouped', '')
        want = SHIPPED[kind][key]
        if op == 'fwd':
            got = {f: R(op, M, N, Kd, G, form=f) for f in ('other', 'pre+act', 'act')}
            if (kind, key) in FORMS:
                assert got[FORMS[kind, key]] == want, (key, got)
                assert got['other'] == ('ig_64x64', 1, None), (key, got)     # what the hint takes the launch away from
            else:
                assert set(got.values()) == {want}, (key, got)
        elif op == 'wgrad':
            assert R(op, M, N, Kd, G, db=True) == want, key
            assert R(op, M, N, Kd, G, db=False)[:2] == want[:2], key         # the bias gradient moves no launch
        else:
            assert R(op, M, N, Kd, G) == want, key
    assert not [k for k in FORMS if k[0] == kind and k[1] not in single]


def test_mnist_weight_gradient_batches_keep_their_routes():
    """The batches of the all-Linear MNIST step (rows of two ELBO terms at batch 512; linear_direct.h quotes their tile
    counts): the image decoder's four layers on 64 x 64 wave tiles, the label decoder's and the image encoder's on 32 x 32."""
    def items(shapes):
        return [(M, N, Kd, N, Kd, True, False) for M, N, Kd in shapes]
    img_dec = [(1024, 512, 64), (1024, 512, 512), (1024, 512, 512), (1024, 784, 512)]
    lbl_dec = [(1024, 512, 64), (1024, 512, 512), (1024, 512, 512), (1024, 10, 512)]
    img_enc = [(512, 128, 512), (512, 512, 512), (512, 512, 784)]
    assert K.linear_wgrad_batched_route(items(img_dec)) == ('wgrad_batched2', (64, 64), 8)
    assert K.linear_wgrad_batched_route(items(lbl_dec)) == ('wgrad_batched2', (32, 32), 4)
    assert K.linear_wgrad_batched_route(items(img_enc)) == ('wgrad_batched2', (32, 32), 4)
    # with the update folded in (the single-GPU step): the 32 x 32 kernel, waves by its own tile count
    assert K.linear_wgrad_batched_route(items(img_dec), adam=True) == ('wgrad_batched_adam', (32, 32), 4)
    assert K.linear_wgrad_batched_route(items(img_enc), adam=True) == ('wgrad_batched_adam', (32, 32), 8)


# ----------------------------------------------------------------------------- both sides of every gate
U = dict(aligned=False)
GATES = [
    # --- make_plan, admission to the small layouts (float4-loadable operands only)
    ('t64 < 256', ('fwd', 1024, 960, 512), ('g2s_32x64_k2',) + NO, ('fwd', 1024, 964, 512), ('ig_64x64', 2, 'finish_few_vec')),
    ('K <= 1024 below 192 tiles of 32', ('fwd', 128, 128, 1024), ('g2s_32x32_k8',) + NO,
     ('fwd', 128, 128, 1028), ('ig_64x64_k4', 17, 'finish')),
    ('t32 >= 192 above K = 1024', ('fwd', 32, 6144, 1028), ('g2s_32x32_k8',) + NO,
     ('fwd', 32, 6112, 1028), ('ig_32x128', 11, 'finish_few_vec')),
    ('t32 >= 192 above K = 1024 (rows)', ('fwd', 384, 512, 1028), ('g2s_32x32_k8',) + NO,
     ('fwd', 352, 512, 1028), ('ig_64x64_k4', 5, 'finish_few_vec')),
    ('K < 4096', ('fwd', 384, 512, 4092), ('g2s_32x32_k8',) + NO, ('fwd', 384, 512, 4096), ('ig_64x64_k4', 5, 'finish_few_vec')),
    # --- inside the small layouts
    ('max(b_tall, b_wide) >= 224', ('fwd', 832, 512, 512), ('g2s_32x32_k4',) + NO, ('fwd', 896, 512, 512), ('g2s_32x64_k4',) + NO),
    ('tall against wide', ('fwd', 960, 480, 512), ('g2s_64x32_k4',) + NO, ('fwd', 960, 512, 512), ('g2s_32x64_k4',) + NO),
    ('320 blocks, 32 x 32', ('fwd', 640, 512, 512), ('g2s_32x32_k8',) + NO, ('fwd', 672, 512, 512), ('g2s_32x32_k4',) + NO),
    ('320 blocks, 32 x 64', ('fwd', 1280, 512, 512), ('g2s_32x64_k4',) + NO, ('fwd', 1344, 512, 512), ('g2s_32x64_k2',) + NO),
    ('320 blocks, 64 x 32', ('dgrad', 1280, 512, 480), ('g2s_64x32_k4',) + NO, ('dgrad', 1408, 512, 480), ('g2s_64x32_k2',) + NO),
    # --- the narrow plan
    ('narrow: I <= 32', ('fwd', 32, 128, 4096), ('ig_32x128', 64, 'finish'), ('fwd', 33, 128, 4096), ('ig_64x64_k4', 64, 'finish')),
    ('narrow: J >= 128', ('fwd', 32, 128, 4096), ('ig_32x128', 64, 'finish'), ('fwd', 32, 124, 4096), ('ig_64x64_k4', 64, 'finish')),
    # --- the 64 x 128 forward / dgrad gate
    ('64x128: K >= 4096', ('fwd', 1024, 512, 4096), ('ig_64x128', 8, 'finish_few_vec'), ('fwd', 1024, 512, 4092), ('g2s_32x64_k4',) + NO),
    ('64x128: J >= 128', ('fwd', 2048, 128, 4096), ('ig_64x128', 16, 'finish_few_vec'),
     ('fwd', 2048, 124, 4096), ('ig_64x64_k4', 4, 'finish_few_vec')),
    ('64x128: 64 tiles', ('fwd', 2048, 128, 4096), ('ig_64x128', 16, 'finish_few_vec'),
     ('fwd', 1984, 128, 4096), ('ig_64x64_k4', 4, 'finish_few_vec')),
    ('64x128: 256 tiles', ('fwd', 1024, 1024, 4096), ('ig_64x128', 4, 'finish_few_vec'),
     ('fwd', 1088, 1024, 4096), ('ig_64x64', 2, 'finish_few_vec')),
    ('64x128: not for weight gradients', ('dgrad', 1024, 4096, 512), ('ig_64x128', 8, 'finish_few_vec'),
     ('wgrad', 4096, 1024, 512, 2), ('ig_64x64', 2, 'finish_few_vec')),
    # --- k-groups
    ('4 k-groups: tiles * 4 <= 256', ('fwd', 4096, 64, 4096), ('ig_64x64_k4', 4, 'finish_few_vec'),
     ('fwd', 4160, 64, 4096), ('ig_64x64_k2', 4, 'finish_few_vec')),
    ('2 k-groups: tiles * 2 <= 256', ('fwd', 8192, 64, 4096), ('ig_64x64_k2', 2, 'finish_few_vec'),
     ('fwd', 8256, 64, 4096), ('ig_64x64', 4, 'finish_few_vec')),
    ('k-groups: K >= 128', ('fwd', 64, 64, 128, 1, U), ('ig_64x64_k4_s', 2, 'finish_few_vec'),
     ('fwd', 64, 64, 124, 1, U), ('ig_64x64_s', 2, 'finish_few_vec')),
    # --- split counts and the finish launch
    ('maxs = ceil(K / 64); 16 partials', ('fwd', 64, 64, 1024, 1, U), ('ig_64x64_k4_s', 16, 'finish_few_vec'),
     ('fwd', 64, 64, 1028, 1, U), ('ig_64x64_k4_s', 17, 'finish')),
    ('split cap 64 (5 narrow tiles ask for 102) against maxs = 63', ('fwd', 17, 640, 16384), ('ig_32x128', 64, 'finish'),
     ('fwd', 17, 640, 4032), ('ig_32x128', 63, 'finish')),
    ('split cap 64 holds for the data gradient too', ('dgrad', 17, 16384, 640), ('ig_32x128', 64, 'finish'),
     ('dgrad', 17, 4032, 640), ('ig_32x128', 63, 'finish')),
    ('split cap: 512 when tiles <= 4', ('fwd', 17, 512, 16384), ('ig_32x128', 128, 'finish'),
     ('fwd', 17, 640, 16384), ('ig_32x128', 64, 'finish')),
    ('deepest split: one narrow tile, 512 partials', ('fwd', 17, 128, 65536), ('ig_32x128', 512, 'finish'),
     ('fwd', 17, 128, 32704), ('ig_32x128', 511, 'finish')),
    ('one k-grouped tile asks for 256', ('fwd', 64, 64, 32768, 1, U), ('ig_64x64_k4_s', 256, 'finish'),
     ('fwd', 64, 64, 16320, 1, U), ('ig_64x64_k4_s', 255, 'finish')),
    ('k-grouped: 4 tiles against 5 (the block target, below either cap)', ('fwd', 128, 128, 32768), ('ig_64x64_k4', 64, 'finish'),
     ('fwd', 128, 160, 32768), ('ig_64x64_k4', 43, 'finish')),
    ('no scratch, no split', ('fwd', 64, 64, 1028, 1, dict(aligned=False, ws_bytes=0)), ('ig_64x64_k4_s',) + NO,
     ('fwd', 64, 64, 1028, 1, U), ('ig_64x64_k4_s', 17, 'finish')),
    ('finish: J % 4', ('wgrad', 132, 70, 68, 1, U), ('ig_64x64_k4_s', 3, 'finish_few_vec'),
     ('wgrad', 132, 68, 70, 1, U), ('ig_64x64_k4_s', 3, 'finish_few')),
    ('finish: stride % 4 (the row sums sit behind every partial)', ('wgrad', 132, 70, 68, 1, dict(aligned=False, db=False)),
     ('ig_64x64_k4_s', 3, 'finish_few_vec'), ('wgrad', 132, 70, 68, 1, dict(aligned=False, db=True)), ('ig_64x64_k4_s', 3, 'finish_few')),
    # --- PLAN_LIN_WGRAD: plain 4-wave blocks once tiles * w1 >= 128
    ('weight gradient: tiles * w1 >= 128', ('wgrad', 512, 512, 256, 2, U), ('ig_64x64_s', 2, 'finish_few_vec'),
     ('wgrad', 511, 512, 256, 2, U), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    # --- g2_plan_for
    ('gemm2, two outputs: K <= 640', ('fwd', 2048, 3072, 640, 1, dict(form='pre+act')), ('gemm2',) + NO,
     ('fwd', 2048, 3072, 644, 1, dict(form='pre+act')), ('ig_64x64',) + NO),
    ('gemm2, two outputs: 1536 tiles', ('fwd', 2048, 3072, 640, 1, dict(form='pre+act')), ('gemm2',) + NO,
     ('fwd', 2048, 3008, 640, 1, dict(form='pre+act')), ('ig_64x64',) + NO),
    ('gemm2, two outputs: the form', ('fwd', 2048, 3072, 640, 1, dict(form='pre+act')), ('gemm2',) + NO,
     ('fwd', 2048, 3072, 640, 1, dict(form='act')), ('ig_64x64',) + NO),
    ('gemm2, act alone: K <= 128', ('fwd', 2048, 3072, 128, 1, dict(form='act')), ('gemm2',) + NO,
     ('fwd', 2048, 3072, 132, 1, dict(form='act')), ('ig_64x64',) + NO),
    ('gemm2, act alone: 1536 tiles', ('fwd', 2048, 3072, 128, 1, dict(form='act')), ('gemm2',) + NO,
     ('fwd', 2048, 3008, 128, 1, dict(form='act')), ('ig_64x64',) + NO),
    ('gemm2, act alone: the form', ('fwd', 2048, 3072, 128, 1, dict(form='act')), ('gemm2',) + NO,
     ('fwd', 2048, 3072, 128, 1, dict(form='other')), ('ig_64x64',) + NO),
    ('gemm2: groups count as tiles', ('fwd', 768, 512, 512, 16, dict(form='pre+act')), ('gemm2',) + NO,
     ('fwd', 768, 512, 512, 15, dict(form='pre+act')), ('ig_64x64',) + NO),
    # --- float4 loaders against scalar ones
    ('scalar: K % 4', ('fwd', 512, 512, 512), ('g2s_32x32_k8',) + NO, ('fwd', 512, 512, 514), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    ('scalar: ldx % 4', ('fwd', 512, 512, 512, 1, dict(ld_a=516)), ('g2s_32x32_k8',) + NO,
     ('fwd', 512, 512, 512, 1, dict(ld_a=514)), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    ('scalar: a misaligned operand', ('fwd', 512, 512, 512), ('g2s_32x32_k8',) + NO,
     ('fwd', 512, 512, 512, 1, U), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    ('scalar: weight group stride % 4', ('fwd', 512, 512, 512, 3, dict(gs_b=512 * 512 + 4)), ('g2s_32x64_k2',) + NO,
     ('fwd', 512, 512, 512, 3, dict(gs_b=512 * 512 + 2)), ('ig_64x64_s', 3, 'finish_few_vec')),
    ('scalar: input group stride % 4', ('fwd', 512, 512, 512, 3, dict(gs_a=512 * 512 + 4)), ('g2s_32x64_k2',) + NO,
     ('fwd', 512, 512, 512, 3, dict(gs_a=512 * 512 + 2)), ('ig_64x64_s', 3, 'finish_few_vec')),
    ('scalar, dgrad: N % 4', ('dgrad', 512, 512, 512), ('g2s_32x32_k8',) + NO, ('dgrad', 512, 514, 512), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    ('scalar, dgrad: K % 4', ('dgrad', 512, 512, 512), ('g2s_32x32_k8',) + NO, ('dgrad', 512, 512, 514), ('ig_64x64_k2_s', 4, 'finish_few')),
    ('scalar, dgrad: lddy % 4', ('dgrad', 512, 512, 512, 1, dict(ld_a=516)), ('g2s_32x32_k8',) + NO,
     ('dgrad', 512, 512, 512, 1, dict(ld_a=514)), ('ig_64x64_k4_s', 4, 'finish_few_vec')),
    ('scalar, wgrad: ldx % 4', ('wgrad', 512, 64, 64, 1, dict(ld_b=68)), ('igs_32x32_k8',) + NO,
     ('wgrad', 512, 64, 64, 1, dict(ld_b=66)), ('ig_64x64_k4_s', 8, 'finish_few_vec')),
    ('scalar, wgrad: N % 4', ('wgrad', 512, 64, 64), ('igs_32x32_k8',) + NO, ('wgrad', 512, 66, 64), ('ig_64x64_k4_s', 8, 'finish_few_vec')),
    ('scalar, fused loss: K % 4', ('bce_fwd', 768, 18, 512), ('igs_32x32_k8',) + NO, ('bce_fwd', 768, 18, 514), ('ig_64x64_k4_s',) + NO),
    # --- linear_dgrad_impl
    ('dgrad: N <= 16', ('dgrad', 512, 16, 512), ('dgrad_smalln',) + NO, ('dgrad', 512, 20, 512), ('g2s_32x32_k8',) + NO),
    # --- wgrad_direct_ok, wgrad_direct_launch
    ('direct: 16 tiles', ('wgrad', 512, 128, 128), ('wgrad_direct_16',) + NO, ('wgrad', 512, 160, 96), ('igs_32x32_k8',) + NO),
    ('direct: 2048 tiles', ('wgrad', 512, 2048, 1024), ('wgrad_direct_4',) + NO, ('wgrad', 512, 2080, 1024), ('ig_64x64',) + NO),
    ('direct: M <= 4096', ('wgrad', 4096, 128, 128), ('wgrad_direct_16',) + NO, ('wgrad', 4097, 128, 128), ('ig_64x64_k4', 43, 'finish')),
    ('direct: one group', ('wgrad', 512, 128, 128), ('wgrad_direct_16',) + NO, ('wgrad', 512, 128, 128, 2), ('igs_32x32_k8',) + NO),
    ('direct: 8 waves from 96 tiles', ('wgrad', 512, 384, 256), ('wgrad_direct_8',) + NO, ('wgrad', 512, 608, 160), ('wgrad_direct_16',) + NO),
    ('direct: 4 waves from 192 tiles', ('wgrad', 512, 384, 512), ('wgrad_direct_4',) + NO, ('wgrad', 512, 32, 6112), ('wgrad_direct_8',) + NO),
    ('direct: takes operands float4 loads cannot', ('wgrad', 512, 129, 131, 1, U), ('wgrad_direct_16',) + NO,
     ('wgrad', 512, 129, 131, 2, U), ('ig_64x64_k4_s', 8, 'finish_few')),
]


def _call(t):
    op, M, N, Kd = t[:4]
    G = t[4] if len(t) > 4 else 1
    return R(op, M, N, Kd, G, **dict(t[5] if len(t) > 5 else {}))


@pytest.mark.parametrize('gate', GATES, ids=[g[0] for g in GATES])
def test_both_sides_of_a_gate(gate):
    name, a, want_a, b, want_b = gate
    assert _call(a) == want_a, '%s: %s' % (name, (a,))
    assert _call(b) == want_b, '%s: %s' % (name, (b,))


def test_small_igemm_layouts_are_not_reachable_from_forward_or_data_gradient():
    """launch_gemm2s has an instantiation for each of the six small layouts and is asked first: a forward or data-gradient
    launch never reaches igemm_kernel's BK = 64 forms (the fused losses and the weight gradients do)."""
    dims = (20, 36, 68, 132, 260, 516, 1028, 2052, 4100)
    seen = {'fwd': set(), 'dgrad': set(), 'wgrad': set(), 'bce_fwd': set()}
    for M in dims:
        for N in dims:
            for Kd in (20, 68, 516, 1028):
                for G in (1, 3):
                    for op in ('fwd', 'dgrad', 'wgrad'):
                        seen[op].add(R(op, M, N, Kd, G)[0])
                seen['bce_fwd'].add(R('bce_fwd', M, N, Kd)[0])
    small = {'igs_64x32_k4', 'igs_64x32_k2', 'igs_32x64_k4', 'igs_32x64_k2', 'igs_32x32_k8', 'igs_32x32_k4'}
    assert not (seen['fwd'] | seen['dgrad']) & small
    assert seen['wgrad'] | seen['bce_fwd'] >= small and len(seen['wgrad'] & small) >= 4 and len(seen['bce_fwd'] & small) >= 4
    assert {r for r in seen['fwd'] if r.startswith('g2s_')} == {r.replace('igs_', 'g2s_') for r in small}


# ----------------------------------------------------------------------------- the batched weight gradient
def B(*shapes, **kw):
    return K.linear_wgrad_batched_route([(M, N, Kd, N, Kd, True, False) for M, N, Kd in shapes], **kw)


def test_batched_wave_tile_is_the_one_with_the_least_busy_cu():
    """ceil(tiles / 256) x tile cost (4 / 2 / 1 for 64 x 64 / 64 x 32 / 32 x 32): the larger tile wins ties."""
    one = (1024, 512, 512)                      # 64 / 128 / 256 tiles
    assert B(one) == ('wgrad_batched2', (32, 32), 8)                            # 4 / 2 / 1
    assert B(one, one) == ('wgrad_batched2', (64, 32), 8)                       # 128 / 256 / 512: 4 / 2 / 2
    assert B(one, one, one, one) == ('wgrad_batched2', (64, 64), 8)             # 256 / 512 / 1024: 4 / 4 / 4
    assert B(one, one, one, one, (1024, 32, 32)) == ('wgrad_batched2', (32, 32), 4)      # 257 / 513 / 1025: 8 / 6 / 5


def test_batched_waves_per_tile():
    """16 / 8 / 4 / 2 waves from 160 / 400 / 1024 tiles of the chosen shape.  The busiest-CU rule changes the shape between
    256 and ~450-520 tiles, so the 400 line is crossed in a jump: the nearest batches either side are pinned.  64 x 64 and
    32 x 32 tiles run at least 4 waves.  A batch with few rows halves the waves until each has 32 rows."""
    # 32 x 32 tiles
    assert B((1024, 128, 1248)) == ('wgrad_batched2', (32, 32), 16)         # 156 tiles
    assert B((1024, 128, 1280)) == ('wgrad_batched2', (32, 32), 8)          # 160
    assert B((1024, 128, 2048)) == ('wgrad_batched2', (32, 32), 8)          # 256
    assert B((1024, 384, 1376)) == ('wgrad_batched2', (32, 32), 4)          # 516
    assert B((1024, 896, 2048)) == ('wgrad_batched2', (32, 32), 4)          # 1792: not 2
    # 64 x 32 tiles
    assert B((1024, 192, 1696)) == ('wgrad_batched2', (64, 32), 16)         # 159
    assert B((1024, 256, 1280)) == ('wgrad_batched2', (64, 32), 8)          # 160
    assert B((1024, 256, 2048)) == ('wgrad_batched2', (64, 32), 8)          # 256
    assert B((1024, 1856, 544)) == ('wgrad_batched2', (64, 32), 4)          # 493
    assert B((1024, 1984, 1056)) == ('wgrad_batched2', (64, 32), 4)         # 1023
    assert B((1024, 1984, 1056), (1024, 64, 32)) == ('wgrad_batched2', (64, 32), 2)     # 1024
    # 64 x 64 tiles
    assert B((1024, 448, 1760)) == ('wgrad_batched2', (64, 64), 8)          # 196
    assert B((1024, 512, 2048)) == ('wgrad_batched2', (64, 64), 8)          # 256
    assert B((1024, 1472, 1248)) == ('wgrad_batched2', (64, 64), 4)         # 460
    # rows: 16 waves need 512, 8 need 256, 4 need 128 -- and never fewer than 4 on a 32 x 32 tile
    assert B((512, 128, 1248)) == ('wgrad_batched2', (32, 32), 16)
    assert B((511, 128, 1248)) == ('wgrad_batched2', (32, 32), 8)
    assert B((255, 128, 1248)) == ('wgrad_batched2', (32, 32), 4)
    assert B((8, 128, 1248)) == ('wgrad_batched2', (32, 32), 4)
    # the rows of the LONGEST item count
    assert B((8, 128, 1248), (512, 32, 32)) == ('wgrad_batched2', (32, 32), 16)
    # 64 x 32 tiles go down to 2 waves by rows as well
    assert B((128, 1856, 544)) == ('wgrad_batched2', (64, 32), 4)
    assert B((127, 1856, 544)) == ('wgrad_batched2', (64, 32), 2)
    assert B((127, 1472, 1248)) == ('wgrad_batched2', (64, 64), 4)          # launched with 4 all the same


def test_batched_forms_that_exist_and_the_one_that_does_not():
    """Nine of the ten wgrad_batched2_kernel instantiations can be reached; 64 x 64 tiles with 16 waves cannot: fewer than
    160 tiles of 64 x 64 are fewer than 640 of 32 x 32, at most 3 units on the busiest CU against 4."""
    seen = set()
    dims = (20, 36, 100, 132, 260, 516, 900, 1284, 2052)
    for M in (20, 136, 264, 520):
        for n in (1, 2, 4, 6):
            for a in dims:
                for b in dims:
                    if ((a + 31) // 32) * ((b + 31) // 32) <= 2048:
                        seen.add(B(*[(M, a, b), (M, b, a)][:n] * ((n + 1) // 2)) if n > 1 else B((M, a, b)))
    forms = {(t, w) for r, t, w in seen if r == 'wgrad_batched2'}
    assert forms == {((32, 32), 4), ((32, 32), 8), ((32, 32), 16), ((64, 32), 2), ((64, 32), 4), ((64, 32), 8),
                     ((64, 32), 16), ((64, 64), 4), ((64, 64), 8)}, sorted(forms)
    assert {r for r, _, _ in seen} == {'wgrad_batched2'}


def test_batched_falls_back_to_the_older_kernel_past_31_bit_offsets():
    """(M + 1024) x ld x 4 >= 2^31 on either operand: wgrad_batched2_kernel's signed byte offsets could wrap; the 32 x 32
    kernel (unsigned, M x ld x 4 < 2^32) takes the batch.  Its waves: 4 from 768 tiles, 8 from 256."""
    ld = (1 << 31) // (4 * (8 + 1024)) + 1          # 520249 floats
    ok, past = (8, 64, 64, 64, ld - 1, True, False), (8, 64, 64, 64, ld, True, False)
    assert K.linear_wgrad_batched_route([ok]) == ('wgrad_batched2', (32, 32), 4)
    assert K.linear_wgrad_batched_route([past]) == ('wgrad_batched', (32, 32), 16)
    assert K.linear_wgrad_batched_route([(8, 64, 64, ld, 64, True, False)]) == ('wgrad_batched', (32, 32), 16)
    big = (8, 512, 512, 512, ld, False, False)
    assert K.linear_wgrad_batched_route([big]) == ('wgrad_batched', (32, 32), 8)                        # 256 tiles
    assert K.linear_wgrad_batched_route([big, (8, 512, 1024, 512, 1024, False, False)]) == ('wgrad_batched', (32, 32), 4)   # 768
    assert K.linear_wgrad_batched_route([(8, 512, 992, 512, ld, False, False)]) == ('wgrad_batched', (32, 32), 8)            # 496
    assert B((8, 512, 480), adam=True) == ('wgrad_batched_adam', (32, 32), 16)                          # 240
    assert B((8, 512, 512), adam=True) == ('wgrad_batched_adam', (32, 32), 8)
    assert B((8, 512, 1536), adam=True) == ('wgrad_batched_adam', (32, 32), 4)


def test_batched_table_refusals():
    """wgrad_batch_item_ok and wgrad_batch_table: what the launch refuses, the query refuses."""
    def one(*it, **kw):
        return K.linear_wgrad_batched_route([it], **kw)
    assert one(64, 2048, 1024, 2048, 1024, True, False)[0] == 'wgrad_batched2'         # 2048 tiles
    for bad in ((64, 2080, 1024, 2080, 1024, True, False),         # 2080 tiles
                (4097, 64, 64, 64, 64, True, False),               # M > 4096
                (4096, 64, 64, 1 << 18, 64, True, False),          # M x lddy x 4 = 2^32
                (4096, 64, 64, 64, 1 << 18, True, False),
                (64, 64, 64, 63, 64, True, False),                 # lddy < N
                (64, 64, 64, 64, 63, True, False),
                (0, 64, 64, 64, 64, True, False)):
        with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
            one(*bad)
    assert one(4096, 64, 64, (1 << 18) - 1, 64, True, False)[0] == 'wgrad_batched'      # inside 2^32, past 2^31
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.linear_wgrad_batched_route([])
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.linear_wgrad_batched_route([(64, 32, 32, 32, 32, True, False)] * (_lib.WGRAD_BATCH_MAX + 1))
    assert K.linear_wgrad_batched_route([(64, 32, 32, 32, 32, True, False)] * _lib.WGRAD_BATCH_MAX)[0] == 'wgrad_batched2'
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):        # the update needs the step's whole gradient
        one(64, 32, 32, 32, 32, True, True, adam=True)
    # two items that write one gradient
    arr = (_lib.WgradItem * 2)()
    for q in range(2):
        arr[q] = _lib.WgradItem(1 << 20, 32, 1 << 21, 32, 1 << 22, None, 64, 32, 32, 0)
    assert _lib.lib().mvae_linear_wgrad_batched_route(arr, 2, 0, None, None, None) == -1
    arr[1].dw = 1 << 23
    assert _lib.lib().mvae_linear_wgrad_batched_route(arr, 2, 0, None, None, None) == 50
    arr[1].dw = None
    assert _lib.lib().mvae_linear_wgrad_batched_route(arr, 2, 0, None, None, None) == -1
    assert _lib.lib().mvae_linear_wgrad_batched_route(None, 1, 0, None, None, None) == -1


# ----------------------------------------------------------------------------- the query itself
def _raw(op, G, M, N, Kd, ld_a, ld_b, ws, form=0, db=0, aligned=1, sp=None, fin=None):
    return _lib.lib().mvae_linear_route(op, G, M, N, Kd, ld_a, ld_b, M * Kd, N * Kd, aligned, form, db, ws, sp, fin)


def test_scratch_one_byte_short_is_err_ws():
    """A split plan needs splits x (I x J [+ I]) floats per group; one byte less is MVAE_ERR_WS, as in the launch."""
    FWD, DGRAD, WGRAD = (_lib.LINEAR_OPS[k] for k in ('fwd', 'dgrad', 'wgrad'))
    sp = ctypes.c_int(0)
    big = 1 << 30
    assert _raw(FWD, 1, 256, 512, 6400, 6400, 512, big, sp=ctypes.byref(sp)) == 18 and sp.value == 8
    need = 8 * 256 * 512 * 4
    assert _raw(FWD, 1, 256, 512, 6400, 6400, 512, need) == 18
    assert _raw(FWD, 1, 256, 512, 6400, 6400, 512, need - 1) == -3
    assert _raw(FWD, 3, 256, 512, 6400, 6400, 512, 3 * need - 1) == -3          # every group has its own region
    # data gradient of the same layer: I x J = M x K
    assert _raw(DGRAD, 1, 256, 6400, 100, 6400, 100, big, sp=ctypes.byref(sp)) == 18 and sp.value == 29
    assert _raw(DGRAD, 1, 256, 6400, 100, 6400, 100, 29 * 256 * 100 * 4) == 18
    assert _raw(DGRAD, 1, 256, 6400, 100, 6400, 100, 29 * 256 * 100 * 4 - 1) == -3
    # the scratch is checked in front of the N <= 16 gate too, as in the launch
    assert _raw(DGRAD, 1, 64, 16, 64, 16, 64, big) == 40
    # weight gradient with a bias gradient: N row sums behind every partial (celeba19's 18 groups of 768 x 512 x 100)
    assert _raw(WGRAD, 18, 768, 512, 100, 512, 100, big, db=1, sp=ctypes.byref(sp)) == 20 and sp.value == 2
    assert _raw(WGRAD, 18, 768, 512, 100, 512, 100, 18 * 2 * (512 * 100 + 512) * 4, db=1) == 20
    assert _raw(WGRAD, 18, 768, 512, 100, 512, 100, 18 * 2 * (512 * 100 + 512) * 4 - 1, db=1) == -3
    assert _raw(WGRAD, 18, 768, 512, 100, 512, 100, 18 * 2 * (512 * 100) * 4, db=0) == 20
    assert _raw(WGRAD, 18, 768, 512, 100, 512, 100, 18 * 2 * (512 * 100) * 4 - 1, db=0) == -3
    # no scratch at all: no split, no error
    assert _raw(FWD, 1, 256, 512, 6400, 6400, 512, 0, sp=ctypes.byref(sp)) == 18 and sp.value == 1


def test_bad_arguments_are_err_arg():
    ops = _lib.LINEAR_OPS
    ws = WS_MIN
    assert _raw(7, 1, 64, 64, 64, 64, 64, ws) == -1
    assert _raw(-1, 1, 64, 64, 64, 64, 64, ws) == -1
    for op in ops.values():
        for bad in ((0, 64, 64), (64, 0, 64), (64, 64, 0), (-5, 64, 64)):
            assert _raw(op, 1, *bad, 64, 64, ws) == -1
    assert _raw(ops['fwd'], 1, 64, 32, 64, 63, 32, ws) == -1            # ldx < K
    assert _raw(ops['fwd'], 1, 64, 32, 64, 64, 31, ws) == -1            # ldy < N
    assert _raw(ops['dgrad'], 1, 64, 32, 64, 31, 64, ws) == -1          # lddy < N
    assert _raw(ops['dgrad'], 1, 64, 32, 64, 32, 63, ws) == -1          # lddx < K
    assert _raw(ops['wgrad'], 1, 64, 32, 64, 31, 64, ws) == -1
    assert _raw(ops['wgrad'], 1, 64, 32, 64, 32, 63, ws) == -1
    assert _raw(ops['fwd'], 1, 64, 32, 64, 64, 32, ws, form=3) == -1
    assert _raw(ops['fwd'], 0, 64, 32, 64, 64, 32, ws) == -1
    assert _raw(ops['fwd'], 4097, 64, 32, 64, 64, 32, ws) == -1
    assert _raw(ops['fwd'], 4096, 64, 32, 64, 64, 32, ws) > 0
    # the fused losses: one group, at most 32 classes for the categorical term; no plan of theirs splits
    assert _raw(ops['bce_fwd'], 2, 64, 32, 64, 64, 32, ws) == -1
    assert _raw(ops['ce_fwd'], 1, 64, 33, 64, 64, 33, ws) == -1
    assert _raw(ops['ce_fwd'], 1, 64, 32, 64, 64, 32, ws) == 12
    sp, fin = ctypes.c_int(0), ctypes.c_int(9)
    for Kd in (64, 1028, 6400, 65536):
        for M, N in ((64, 32), (1, 784), (4096, 784), (32, 784)):
            assert _raw(ops['bce_fwd'], 1, M, N, Kd, Kd, N, ws, sp=ctypes.byref(sp), fin=ctypes.byref(fin)) > 0
            assert (sp.value, fin.value) == (1, 0)
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.linear_route('fwd', 64, 64, 64, ld_a=60)
    with pytest.raises(RuntimeError, match='MVAE_ERR_WS'):
        K.linear_route('fwd', 256, 512, 6400, ws_bytes=4096)


def test_every_route_id_has_a_name_and_out_pointers_are_optional():
    text = open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read()
    ids = {n: int(v) for n, v in re.findall(r'#define\s+MVAE_LROUTE_(\w+)\s+(\d+)', text)}
    assert len(ids) == 34 and sorted(ids.values()) == sorted(_lib.LINEAR_ROUTES)
    for name, v in ids.items():
        assert _lib.LINEAR_ROUTES[v] == name.lower(), name
    assert {n: int(v) for n, v in re.findall(r'#define\s+MVAE_LOP_(\w+)\s+(\d+)', text)} == \
        {k.upper(): v for k, v in _lib.LINEAR_OPS.items()}
    fins = {int(v): n.lower() for n, v in re.findall(r'#define\s+MVAE_LFINISH_(\w+)\s+(\d+)', text)}
    assert fins == {0: 'none', 1: 'finish', 2: 'few', 3: 'few_vec', 4: 'g2'}
    assert [_lib.LINEAR_FINISH[k] for k in range(5)] == [None, 'finish', 'finish_few', 'finish_few_vec', 'g2_finish']
    assert {n: int(v) for n, v in re.findall(r'#define\s+MVAE_LFORM_(\w+)\s+(\d+)', text)} == {'OTHER': 0, 'PRE_ACT': 1, 'ACT_ONLY': 2}
    # every id the query can return over a sweep is a named one
    ops = _lib.LINEAR_OPS
    sp, fin = ctypes.c_int(0), ctypes.c_int(0)
    for op in ops.values():
        for M, N, Kd in ((64, 8, 64), (300, 1028, 8), (100, 2048, 4096), (17, 132, 1030), (2048, 3072, 128)):
            if op == ops['ce_fwd'] and N > 32:
                continue
            lds = (Kd, N) if op in (ops['fwd'], ops['bce_fwd'], ops['ce_fwd']) else (N, Kd)
            for aligned in (0, 1):
                a = _raw(op, 1, M, N, Kd, lds[0], lds[1], WS_MIN, form=2, db=1, aligned=aligned)
                b = _raw(op, 1, M, N, Kd, lds[0], lds[1], WS_MIN, form=2, db=1, aligned=aligned, sp=ctypes.byref(sp), fin=ctypes.byref(fin))
                c = _raw(op, 1, M, N, Kd, lds[0], lds[1], WS_MIN, form=2, db=1, aligned=aligned, sp=ctypes.byref(sp))
                assert a == b == c and a in _lib.LINEAR_ROUTES
                assert sp.value >= 1 and (fin.value != 0) == (sp.value > 1)
    # an error leaves the out-pointers alone
    sp.value, fin.value = 77, 88
    assert _raw(ops['fwd'], 1, 256, 512, 6400, 6400, 512, 16, sp=ctypes.byref(sp), fin=ctypes.byref(fin)) == -3
    assert (sp.value, fin.value) == (77, 88)
    arr = (_lib.WgradItem * 1)()
    arr[0] = _lib.WgradItem(1 << 20, 32, 1 << 21, 32, 1 << 22, None, 64, 32, 32, 0)
    w = ctypes.c_int(0)
    assert _lib.lib().mvae_linear_wgrad_batched_route(arr, 1, 0, None, None, None) == 50
    assert _lib.lib().mvae_linear_wgrad_batched_route(arr, 1, 1, None, None, ctypes.byref(w)) == 52 and w.value == 16


def test_the_issues_example_shapes():
    """The shapes the issue's hand port named, as the real dispatch routes them (M x N x K)."""
    assert R('fwd', 300, 1028, 8) == ('g2s_32x32_k4', 1, None)
    assert R('fwd', 2048, 260, 8) == ('g2s_64x32_k4', 1, None)
    assert R('dgrad', 4100, 20, 132) == ('g2s_64x32_k2', 1, None)
    assert R('fwd', 100, 2048, 4096) == ('ig_64x128', 16, 'finish_few_vec')
