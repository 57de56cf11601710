"""No GPU: which kernel and loop a row of the BCE row sums takes (mvae_bce_route: bce_block_row + bce_row_vec of
csrc/loss.hip, the functions bce_launch and bce_row_block_kernel themselves go through), and the host-side refusals of every
launch of loss.hip.

  * the BCE calls of the shipped steps keep their route -- a threshold that moves takes a term onto other code, and only the
    benchmark would notice;
  * every gate from both sides, one step apart: the block gate, the first batched trip, a whole number of batched trips,
    P % 4, alignment, the column stride, column weights;
  * the trip count and the tail flag against a replay of the kernel's two loops for every thread, P = 512 .. 20000;
  * the two published thresholds equal _lib's mirrors; every route id has a name; the out-pointers are optional;
  * the launches return MVAE_ERR_ARG before anything is enqueued (dummy host pointers, only refused arguments).
tests/test_loss_routes_gpu.py runs every route at the cheapest shape that reaches its tails.
"""
import ctypes
import os
import re

import pytest

import mvae_amd  # noqa: F401
from mvae_amd import _lib
from mvae_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def header():
    return open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read()


# ----------------------------------------------------------------------------- the shipped steps
def test_shipped_calls_keep_their_route():
    assert K.bce_route(784) == ('block_vec', 0, 1)                           # MNIST / FashionMNIST image rows
    assert K.bce_route(12288) == ('block_vec_batched', 3, 0)                 # CelebA image rows: 3 x 64 x 64
    assert K.bce_route(18, colw=True)[0] == 'wave'                           # CelebA attribute rows
    assert K.bce_route(18)[0] == 'wave'
    assert K.bce_route(256, target_col_stride=18)[0] == 'wave'               # celeba19 attribute rows at batch 256
    assert K.bce_route(512, target_col_stride=18) == ('block_scalar', 0, 0)  # ... at batch 512


# ----------------------------------------------------------------------------- both sides of every gate
# (gate, P, options, (route, batched_trips, tail)) twice: the two calls are one step apart
A, U, W, S2 = dict(), dict(aligned=False), dict(colw=True), dict(target_col_stride=2)
GATES = [
    ('block gate', 511, A, ('wave', 0, 0), 512, A, ('block_vec', 0, 1)),
    ('block gate, unaligned', 511, U, ('wave', 0, 0), 512, U, ('block_scalar', 0, 0)),
    ('first batched trip: P / 4 = 768 | 769', 4 * 768, A, ('block_vec', 0, 1), 4 * 769, A, ('block_vec_batched', 1, 1)),
    ('P / 4 = 1023 | 1024: no tail', 4 * 1023, A, ('block_vec_batched', 1, 1), 4 * 1024, A, ('block_vec_batched', 1, 0)),
    ('P / 4 = 1024 | 1025: a tail again', 4 * 1024, A, ('block_vec_batched', 1, 0), 4 * 1025, A, ('block_vec_batched', 1, 1)),
    ('second batched trip: P / 4 = 1792 | 1793', 4 * 1792, A, ('block_vec_batched', 1, 1), 4 * 1793, A, ('block_vec_batched', 2, 1)),
    ('P % 4', 516, A, ('block_vec', 0, 1), 517, A, ('block_scalar', 0, 0)),
    ('P % 4 from below', 515, A, ('block_scalar', 0, 0), 516, A, ('block_vec', 0, 1)),
    ('aligned operands', 4096, A, ('block_vec_batched', 1, 0), 4096, U, ('block_scalar', 0, 0)),
    ('column stride', 4096, A, ('block_vec_batched', 1, 0), 4096, S2, ('block_scalar', 0, 0)),
    ('column weights keep P = 4096 off the batched loop', 4096, A, ('block_vec_batched', 1, 0), 4096, W, ('block_vec', 0, 1)),
    ('column weights at CelebA image width', 12288, A, ('block_vec_batched', 3, 0), 12288, W, ('block_vec', 0, 1)),
    ('column weights do not matter below the first trip', 3072, A, ('block_vec', 0, 1), 3072, W, ('block_vec', 0, 1)),
    ('the wave kernel has one loop', 511, S2, ('wave', 0, 0), 508, W, ('wave', 0, 0)),
]


@pytest.mark.parametrize('gate', GATES, ids=[g[0] for g in GATES])
def test_gate_from_both_sides(gate):
    _, lo, lo_kw, lo_want, hi, hi_kw, hi_want = gate
    assert K.bce_route(lo, **lo_kw) == lo_want, (lo, lo_kw)
    assert K.bce_route(hi, **hi_kw) == hi_want, (hi, hi_kw)


def replay(P, colw):
    """bce_row_block_kernel's float4 branch, thread by thread: (batched trips of thread 0, the most any thread makes,
    whether any thread makes a single-group trip)."""
    p4, trips, tail = P // 4, [], False
    for tid in range(256):
        i, n = tid, 0
        while not colw and i + 256 * 3 < p4:
            i += 256 * 4
            n += 1
        trips.append(n)
        tail |= i < p4
    return trips[0], max(trips), int(tail)


def test_trip_counts_equal_a_replay_of_the_kernels_loops():
    seen = set()
    for P in list(range(512, 20001, 4)) + [4 * 1024 * k for k in (5, 16, 100)]:
        for colw in (False, True):
            first, most, tail = replay(P, colw)
            assert first == most                               # thread 0 makes the most batched trips
            name, trips, tl = K.bce_route(P, colw=colw)
            assert (trips, tl) == (first, tail), (P, colw)
            assert name == ('block_vec_batched' if first else 'block_vec'), (P, colw)
            seen.add((first > 0, tail))
    assert seen == {(False, 1), (True, 1), (True, 0)}


def test_every_width_below_the_gate_is_the_wave_kernel_and_above_it_the_block_kernel():
    for P in range(1, 1100):
        for kw in (A, U, W, S2):
            name = K.bce_route(P, **kw)[0]
            if P < _lib.BCE_BLOCK_MIN_P:
                assert name == 'wave', (P, kw)
            else:
                vec = P % 4 == 0 and kw in (A, W)
                assert name == ('block_vec' if vec else 'block_scalar'), (P, kw)


# ----------------------------------------------------------------------------- the query itself
def test_constants_equal_the_headers():
    text = header()
    for name, mirror in (('MVAE_BCE_BLOCK_MIN_P', _lib.BCE_BLOCK_MIN_P), ('MVAE_ELBO_LONG_GROUP', _lib.ELBO_LONG_GROUP),
                         ('MVAE_ELBO_MAX_PARTS', _lib.ELBO_MAX_PARTS), ('MVAE_ELBO_MAX_TERMS', _lib.MAX_TERMS)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % name, text).group(1)) == mirror, name
    assert (_lib.BCE_BLOCK_MIN_P, _lib.ELBO_LONG_GROUP) == (512, 2048)
    # loss.hip uses the constants, not the literals
    src = open(os.path.join(ROOT, 'multimodal-vae-public_amd', 'csrc', 'loss.hip')).read()
    assert 'P >= 512' not in src and 'LONG_GROUP = 2048' not in src
    assert 'MVAE_BCE_BLOCK_MIN_P' in src and 'MVAE_ELBO_LONG_GROUP' in src


def test_every_id_has_a_name():
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+MVAE_BCEROUTE_(\w+)\s+(\d+)', header())}
    assert len(ids) == 4 and sorted(ids.values()) == sorted(_lib.BCE_ROUTES)
    for name, v in ids.items():
        assert _lib.BCE_ROUTES[v] == name.lower(), name


def test_error_codes_and_optional_out_pointers():
    lib = _lib.lib()
    for P, cs in ((0, 1), (-4, 1), (784, 0), (784, -1), (0, 0)):
        tr, tl = ctypes.c_int(-7), ctypes.c_int(-7)
        assert lib.mvae_bce_route(P, cs, 1, 0, ctypes.byref(tr), ctypes.byref(tl)) == ERR_ARG, (P, cs)
        assert (tr.value, tl.value) == (-7, -7)                # the out-pointers of a refused call are left alone
        assert lib.mvae_bce_route(P, cs, 1, 0, None, None) == ERR_ARG
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.bce_route(0)
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.bce_route(784, target_col_stride=0)
    seen = set()
    for P, al, cs, w in ((70, 1, 1, 0), (513, 1, 1, 0), (784, 1, 1, 0), (7296, 1, 1, 0), (4096, 1, 1, 1), (4096, 0, 1, 0)):
        name, trips, tail = K.bce_route(P, aligned=bool(al), target_col_stride=cs, colw=bool(w))
        rc = lib.mvae_bce_route(P, cs, al, w, None, None)
        tr, tl = ctypes.c_int(-7), ctypes.c_int(-7)
        assert rc == lib.mvae_bce_route(P, cs, al, w, ctypes.byref(tr), None)
        assert rc == lib.mvae_bce_route(P, cs, al, w, None, ctypes.byref(tl))
        assert _lib.BCE_ROUTES[rc] == name and (tr.value, tl.value) == (trips, tail)
        seen.add(name)
    assert seen == set(_lib.BCE_ROUTES.values())
    assert K.bce_route((1 << 31) - 4)[0] == 'block_vec_batched' and K.bce_route((1 << 31) - 1)[0] == 'block_scalar'


# ----------------------------------------------------------------------------- host-side refusals of the launches
# Checked in front of every launch, so no device is needed.  `p` is host memory: every call below carries an argument the
# launch refuses, and exactly one (the base of each family is a call the launch would take).
@pytest.fixture(scope='module')
def p():
    buf = (ctypes.c_float * 64)()
    yield ctypes.cast(buf, ctypes.c_void_p)


BCE_OK = dict(R=4, P=6, rows_per_group=2, target_rows=2, target_div=1, target_row_stride=6, target_col_stride=1)


@pytest.mark.parametrize('name', sorted(BCE_OK))
@pytest.mark.parametrize('bad', [0, -1])
def test_bce_rowsum_refuses_a_non_positive_dimension(p, name, bad):
    lib = _lib.lib()
    dims = [bad if k == name else v for k, v in BCE_OK.items()]
    assert list(BCE_OK)[:2] == ['R', 'P'] and len(dims) == 7
    assert lib.mvae_bce_rowsum_fwd(p, p, None, p, p, p, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_fwd(p, p, None, p, None, None, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_bwd(p, p, None, p, p, *dims, None) == ERR_ARG


def test_bce_rowsum_refuses_missing_pointers(p):
    lib = _lib.lib()
    dims = list(BCE_OK.values())
    assert lib.mvae_bce_rowsum_fwd(p, p, None, None, p, p, *dims, None) == ERR_ARG       # rowsum NULL
    assert lib.mvae_bce_rowsum_fwd(p, p, None, None, None, None, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_fwd(p, p, None, p, None, p, *dims, None) == ERR_ARG       # dlogits without drow
    assert lib.mvae_bce_rowsum_fwd(None, p, None, p, p, p, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_fwd(p, None, None, p, p, p, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_bwd(p, p, None, p, None, *dims, None) == ERR_ARG          # dlogits NULL
    assert lib.mvae_bce_rowsum_bwd(p, p, None, None, p, *dims, None) == ERR_ARG          # dlogits without drow
    assert lib.mvae_bce_rowsum_bwd(None, p, None, p, p, *dims, None) == ERR_ARG
    assert lib.mvae_bce_rowsum_bwd(p, None, None, p, p, *dims, None) == ERR_ARG


def test_ce_refusals(p):
    lib = _lib.lib()
    # (R, K, rows_per_group, label_rows); the base is (4, 10, 2, 2)
    for dims in ((4, 0, 2, 2), (4, 1025, 2, 2), (4, 10, 2, 0), (4, -1, 2, 2), (0, 10, 2, 2), (4, 10, 0, 2), (4, 10, 2, -2)):
        assert lib.mvae_ce_fwd(p, p, p, p, p, *dims, None) == ERR_ARG, dims
        assert lib.mvae_ce_fwd(p, p, p, None, None, *dims, None) == ERR_ARG, dims
        assert lib.mvae_ce_bwd(p, p, p, p, *dims, None) == ERR_ARG, dims
    ok = (4, 10, 2, 2)
    assert lib.mvae_ce_fwd(p, p, None, p, p, *ok, None) == ERR_ARG                       # row NULL
    assert lib.mvae_ce_fwd(p, p, p, None, p, *ok, None) == ERR_ARG                       # dlogits without drow
    assert lib.mvae_ce_fwd(p, None, p, p, p, *ok, None) == ERR_ARG
    assert lib.mvae_ce_bwd(p, p, None, p, *ok, None) == ERR_ARG
    assert lib.mvae_ce_bwd(p, p, p, None, *ok, None) == ERR_ARG


def parts_of(p, *specs):
    """specs: (first_term, groups, rows_per_group, term_of?)"""
    arr = (_lib.ElboPart * max(len(specs), 1))()
    for q, s in enumerate(specs):
        arr[q] = _lib.ElboPart(p, p, p if len(s) > 3 and s[3] else None, s[0], s[1], s[2])
    return arr


ELBO_REFUSED = {
    '0 parts': ([(0, 3, 4)], 0, 3),
    '-1 parts': ([(0, 3, 4)], -1, 3),
    '5 parts': ([(0, 1, 4)] * 5, 5, 3),
    'T = 41': ([(0, 3, 4)], 1, 41),
    'T = 0': ([(0, 3, 4, True)], 1, 0),
    'first_term + groups > T': ([(1, 3, 4)], 1, 3),
    'first_term + groups > T, second part': ([(0, 3, 4), (2, 2, 4)], 2, 3),
    'first_term < 0': ([(-1, 3, 4)], 1, 3),
    '41 groups of 2 rows': ([(0, 41, 2, True)], 1, 40),
    '1025 groups in all': ([(0, 1000, 1, True), (0, 25, 1, True)], 2, 40),
    '1025 groups in one part': ([(0, 1025, 1, True)], 1, 40),
    '0 groups': ([(0, 0, 4)], 1, 3),
    '0 rows per group': ([(0, 3, 0)], 1, 3),
}


@pytest.mark.parametrize('case', sorted(ELBO_REFUSED))
def test_elbo_reduce_refusals(p, case):
    lib = _lib.lib()
    specs, n, T = ELBO_REFUSED[case]
    arr = parts_of(p, *specs)
    assert lib.mvae_elbo_reduce(arr, n, p, T, None, 0, None, 0, None) == ERR_ARG
    assert lib.mvae_elbo_reduce(arr, n, p, T, p, 16, p, 1, None) == ERR_ARG
    assert lib.mvae_elbo_reduce_prepare(arr, n, p, T, None, 0, None, 0, p, 1, 1e-3, 0.9, 0.999, p, None) == ERR_ARG


def test_elbo_reduce_refuses_missing_pointers(p):
    lib = _lib.lib()
    ok = parts_of(p, (0, 3, 4))
    assert lib.mvae_elbo_reduce(None, 1, p, 3, None, 0, None, 0, None) == ERR_ARG
    assert lib.mvae_elbo_reduce(ok, 1, None, 3, None, 0, None, 0, None) == ERR_ARG
    norows = parts_of(p, (0, 3, 4))
    norows[0].rows = None
    assert lib.mvae_elbo_reduce(norows, 1, p, 3, None, 0, None, 0, None) == ERR_ARG
    assert lib.mvae_elbo_reduce_prepare(ok, 1, p, 3, None, 0, None, 0, None, 1, 1e-3, 0.9, 0.999, p, None) == ERR_ARG  # step_dev
    assert lib.mvae_elbo_reduce_prepare(ok, 1, p, 3, None, 0, None, 0, p, 1, 1e-3, 0.9, 0.999, None, None) == ERR_ARG  # coef2
    # the python wrapper's own check of the table length
    with pytest.raises(RuntimeError, match='ELBO parts'):
        K._elbo_parts([])
    with pytest.raises(RuntimeError, match='ELBO parts'):
        K._elbo_parts([None] * (_lib.ELBO_MAX_PARTS + 1))


def test_group_sums_refusals(p):
    lib = _lib.lib()
    assert lib.mvae_group_sums(p, p, None, None, 3, 4, 0, None) == ERR_ARG               # both destinations NULL
    assert lib.mvae_group_sums(p, None, None, None, 3, 4, _lib.ACCUMULATE, None) == ERR_ARG
    assert lib.mvae_group_sums(None, p, p, p, 3, 4, 0, None) == ERR_ARG
    assert lib.mvae_group_sums(p, p, p, p, 0, 4, 0, None) == ERR_ARG
    assert lib.mvae_group_sums(p, p, p, p, 3, 0, 0, None) == ERR_ARG
