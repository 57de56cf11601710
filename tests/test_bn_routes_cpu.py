"""No GPU: which kernel every training-mode BatchNorm launch takes (mvae_bn_route: bn_shape + bn_route of csrc/norm.hip,
the functions mvae_bn_train_fwd / mvae_bn_train_bwd themselves go through).

  * the BatchNorm calls of the shipped steps (the ``bn_train_*`` keys of profiles/r06_by_shape.json) keep their kernel and
    their slice count -- a threshold that moves takes a layer onto other code, and only the benchmark would notice;
  * every gate of bn_fused_kind and bn_shape from both sides, two shapes one step apart;
  * the two float4 sweeps of the two-launch kernels (rows in parallel / lanes along a row) at the map sizes that take them;
  * the slice count S never exceeds the records mvae_bn_ws_bytes leaves room for, and no ordinary shape is refused
    (n / 8192 + 2 refused 56 x 56 maps at batch 32);
  * the query's own behaviour: the launch's error codes, names for every id, optional out-pointers.
tests/test_bn_routes_gpu.py runs every route in both directions at its cheapest shape.

The host-side refusals of the launches that need no device (exactly one of running_mean / running_var, a tile count that
is no multiple of G) are checked here too: the launch returns before anything is enqueued.
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


def R(G, B, C, HW, bwd=False, aligned=True):
    """(route, slices) -- the launch count follows the route and is checked once, in test_launch_counts."""
    return K.bn_route(G, B, C, HW, bwd=bwd, aligned=aligned)[:2]


def refused(G, B, C, HW, bwd=0, aligned=1):
    return _lib.lib().mvae_bn_route(bwd, G, B, C, HW, aligned, None, None) == -1


# ----------------------------------------------------------------------------- the shipped steps
# (key of profiles/r06_by_shape.json: rows x C x spatial) -> (G, route, slices).  The keys record the rows G * B, not G:
# every step here runs B = 256 rows per group.  G = 1: the encoders (engine.py: forward_tape(image_encoder.plan(), ...),
# the celeba19 trunk) and CelebA's one-group statistics-only decoder pass; G = 2: the image decoder on the terms that
# hold the image (groups=ni / groups=2); G = 3: CelebA's attribute decoder on all three terms (groups=nl); G = 18:
# celeba19's statistics-only decoder pass over the attribute terms (groups=N_ATTRS, stats_only=True).
SHIPPED = {
    'celeba': {
        'bn_train_bwd 256x128x8x8': (1, 'fused_vec_g1', 1),
        'bn_train_bwd 256x256x5x5': (1, 'fused_scalar_g1', 1),
        'bn_train_bwd 256x512': (1, 'bn1d_g1', 1),
        'bn_train_bwd 256x64x16x16': (1, 'two_vec_rows', 8),
        'bn_train_bwd 512x128x8x8': (2, 'fused_vec_g2', 1),
        'bn_train_bwd 512x32x32x32': (2, 'two_vec_rows', 32),
        'bn_train_bwd 512x64x16x16': (2, 'two_vec_rows', 8),
        'bn_train_bwd 768x512': (3, 'bn1d_gn', 1),
        'bn_train_fwd 256x128x8x8': (1, 'fused_vec_g1', 1),
        'bn_train_fwd 256x256x5x5': (1, 'fused_scalar_g1', 1),
        'bn_train_fwd 256x512': (1, 'bn1d_g1', 1),
        'bn_train_fwd 256x64x16x16': (1, 'two_vec_rows', 8),
        'bn_train_fwd 512x128x8x8': (2, 'fused_vec_g2', 1),
        'bn_train_fwd 512x32x32x32': (2, 'two_vec_rows', 32),
        'bn_train_fwd 512x64x16x16': (2, 'two_vec_rows', 8),
        'bn_train_fwd 768x512': (3, 'bn1d_gn', 1),
    },
    'celeba19': {
        'bn_train_bwd 256x128x8x8': (1, 'fused_vec_g1', 1),
        'bn_train_bwd 256x256x5x5': (1, 'fused_scalar_g1', 1),
        'bn_train_bwd 256x32x32x32': (1, 'two_vec_rows', 32),
        'bn_train_bwd 256x64x16x16': (1, 'two_vec_rows', 8),
        'bn_train_bwd 512x128x8x8': (2, 'fused_vec_g2', 1),
        'bn_train_bwd 512x32x32x32': (2, 'two_vec_rows', 32),
        'bn_train_bwd 512x64x16x16': (2, 'two_vec_rows', 8),
        'bn_train_fwd 256x128x8x8': (1, 'fused_vec_g1', 1),
        'bn_train_fwd 256x256x5x5': (1, 'fused_scalar_g1', 1),
        'bn_train_fwd 256x32x32x32': (1, 'two_vec_rows', 32),
        'bn_train_fwd 256x64x16x16': (1, 'two_vec_rows', 8),
        'bn_train_fwd 4608x128x8x8': (18, 'two_vec_rows', 2),
        'bn_train_fwd 4608x64x16x16': (18, 'slice', 1),
        'bn_train_fwd 512x128x8x8': (2, 'fused_vec_g2', 1),
        'bn_train_fwd 512x32x32x32': (2, 'two_vec_rows', 32),
        'bn_train_fwd 512x64x16x16': (2, 'two_vec_rows', 8),
    },
    'fashionmnist': {},      # no BatchNorm in these two models
    'mnist': {},
}


@pytest.mark.parametrize('kind', sorted(SHIPPED))
def test_shipped_layers_keep_their_routes(kind):
    with open(os.path.join(ROOT, 'profiles', 'r06_by_shape.json')) as f:
        table = json.load(f)
    calls = sorted(k for k in table[kind] if k.startswith('bn_train_'))
    assert calls == sorted(SHIPPED[kind]), 'the table of this test and the profile table name different calls'
    batch = table['_meta'][kind]['batch']
    for key in calls:
        name, dims = key.split(' ')
        dims = [int(d) for d in dims.split('x')]
        G, route, slices = SHIPPED[kind][key]
        rows, C, HW = dims[0], dims[1], 1
        for d in dims[2:]:
            HW *= d
        assert rows == G * batch, key
        assert R(G, batch, C, HW, bwd=name.endswith('bwd')) == (route, slices), key


# ----------------------------------------------------------------------------- both sides of every gate
# (gate, (G, B, C, HW) [, options], (route, slices)) twice: the two shapes are one step apart
FWD, BWD, U = dict(), dict(bwd=True), dict(aligned=False)
UB = dict(bwd=True, aligned=False)
GATES = [
    # --- bn_fused_kind: B * C * HW < 2^30 for every single-launch form
    ('2^30 elements, BatchNorm1d', (1, 512, (1 << 21) - 1, 1), FWD, ('bn1d_g1', 1), (1, 512, 1 << 21, 1), FWD, ('two_scalar', 1)),
    ('2^30 elements, spatial', (1, 16, 65535, 1024), FWD, ('fused_vec_g1', 1), (1, 16, 65536, 1024), FWD, ('two_vec_rows', 2)),
    ('2^30 elements, spatial backward', (1, 16, 65535, 1024), BWD, ('fused_vec_g1', 1), (1, 16, 65536, 1024), BWD, ('two_vec_rows', 2)),
    ('2^30 elements, slice form', (2, 65, 64527, 256), FWD, ('slice', 1), (2, 65, 64528, 256), FWD, ('two_vec_rows', 3)),
    # --- BatchNorm1d: G <= 3, B <= 512
    ('BatchNorm1d G <= 3', (3, 512, 40, 1), FWD, ('bn1d_gn', 1), (4, 512, 40, 1), FWD, ('two_scalar', 1)),
    ('BatchNorm1d G <= 3 backward', (3, 512, 40, 1), BWD, ('bn1d_gn', 1), (4, 512, 40, 1), BWD, ('two_scalar', 1)),
    ('BatchNorm1d B <= 512', (1, 512, 40, 1), FWD, ('bn1d_g1', 1), (1, 513, 40, 1), FWD, ('two_scalar', 1)),
    ('BatchNorm1d B <= 512, groups', (3, 512, 40, 1), FWD, ('bn1d_gn', 1), (3, 513, 40, 1), FWD, ('two_scalar', 1)),
    ('BatchNorm1d B <= 512 backward', (2, 512, 40, 1), BWD, ('bn1d_gn', 1), (2, 513, 40, 1), BWD, ('two_scalar', 1)),
    ('BatchNorm1d G = 1 / 2', (1, 300, 40, 1), FWD, ('bn1d_g1', 1), (2, 300, 40, 1), FWD, ('bn1d_gn', 1)),
    ('BatchNorm1d unaligned', (1, 512, 40, 1), U, ('bn1d_g1', 1), (1, 513, 40, 1), U, ('two_scalar', 1)),
    # --- all groups in one block, float4 units: n <= 16384
    ('n <= 16384, G = 1', (1, 64, 2, 256), FWD, ('fused_vec_g1', 1), (1, 65, 2, 256), FWD, ('two_vec_rows', 3)),
    ('n <= 16384, G = 2', (2, 64, 2, 256), FWD, ('fused_vec_g2', 1), (2, 65, 2, 256), FWD, ('two_vec_rows', 3)),
    ('n <= 16384, G = 3', (3, 64, 2, 256), FWD, ('fused_vec_g3', 1), (3, 65, 2, 256), FWD, ('two_vec_rows', 3)),
    ('forward G <= 3', (3, 64, 2, 256), FWD, ('fused_vec_g3', 1), (4, 64, 2, 256), FWD, ('two_vec_rows', 2)),
    ('n = 16384, G = 4: two-launch on both sides', (4, 64, 2, 256), FWD, ('two_vec_rows', 2), (4, 65, 2, 256), FWD, ('two_vec_rows', 3)),
    ('n <= 16384, G = 1 backward', (1, 64, 2, 256), BWD, ('fused_vec_g1', 1), (1, 65, 2, 256), BWD, ('two_vec_rows', 3)),
    ('n <= 16384, G = 2 backward', (2, 64, 2, 256), BWD, ('fused_vec_g2', 1), (2, 65, 2, 256), BWD, ('two_vec_rows', 3)),
    ('backward G <= 2', (2, 64, 2, 256), BWD, ('fused_vec_g2', 1), (3, 64, 2, 256), BWD, ('two_vec_rows', 2)),
    ('n = 16384, G = 3 backward: two-launch on both sides', (3, 64, 2, 256), BWD, ('two_vec_rows', 2), (3, 65, 2, 256), BWD, ('two_vec_rows', 3)),
    ('n <= 16384 at HW = 4', (1, 4096, 2, 4), FWD, ('fused_vec_g1', 1), (1, 4097, 2, 4), FWD, ('two_vec_rows', 3)),
    # --- one element per register: n <= 16384 for one group, <= 8192 for several
    ('scalar n <= 16384, G = 1', (1, 655, 2, 25), FWD, ('fused_scalar_g1', 1), (1, 656, 2, 25), FWD, ('two_scalar', 3)),
    ('scalar n <= 16384, G = 1 backward', (1, 655, 2, 25), BWD, ('fused_scalar_g1', 1), (1, 656, 2, 25), BWD, ('two_scalar', 3)),
    ('scalar n = 16384 exactly (HW = 2)', (1, 8192, 2, 2), FWD, ('fused_scalar_g1', 1), (1, 8193, 2, 2), FWD, ('two_scalar', 3)),
    ('unaligned n <= 16384, G = 1', (1, 64, 2, 256), U, ('fused_scalar_g1', 1), (1, 65, 2, 256), U, ('two_scalar', 3)),
    ('unaligned n <= 16384, G = 1 backward', (1, 64, 2, 256), UB, ('fused_scalar_g1', 1), (1, 65, 2, 256), UB, ('two_scalar', 3)),
    ('scalar n <= 8192, G = 2', (2, 327, 2, 25), FWD, ('fused_scalar_gn', 1), (2, 328, 2, 25), FWD, ('two_scalar', 2)),
    ('scalar n <= 8192, G = 2 backward', (2, 327, 2, 25), BWD, ('fused_scalar_gn', 1), (2, 328, 2, 25), BWD, ('two_scalar', 2)),
    ('scalar n <= 8192, G = 3', (3, 327, 2, 25), FWD, ('fused_scalar_gn', 1), (3, 328, 2, 25), FWD, ('two_scalar', 2)),
    ('unaligned n = 8192 exactly, G = 2', (2, 32, 2, 256), U, ('fused_scalar_gn', 1), (2, 33, 2, 256), U, ('two_scalar', 2)),
    ('unaligned n = 8192 exactly, G = 2 backward', (2, 32, 2, 256), UB, ('fused_scalar_gn', 1), (2, 33, 2, 256), UB, ('two_scalar', 2)),
    ('the halved limit is for several groups only', (1, 33, 2, 256), U, ('fused_scalar_g1', 1), (2, 33, 2, 256), U, ('two_scalar', 2)),
    ('aligned groups keep 16384', (2, 33, 2, 256), FWD, ('fused_vec_g2', 1), (2, 33, 2, 256), U, ('two_scalar', 2)),
    ('scalar forward G <= 3', (3, 40, 3, 25), FWD, ('fused_scalar_gn', 1), (4, 40, 3, 25), FWD, ('two_scalar', 1)),
    ('scalar backward G <= 2', (2, 40, 3, 25), BWD, ('fused_scalar_gn', 1), (3, 40, 3, 25), BWD, ('two_scalar', 1)),
    # --- one block per (channel, group) slice: 16384 < n <= 65536, C * G >= 512, HW / 4 divides the 1024 threads
    ('slice n > 16384', (8, 64, 64, 256), FWD, ('two_vec_rows', 2), (8, 65, 64, 256), FWD, ('slice', 1)),
    ('slice n <= 65536', (8, 256, 64, 256), FWD, ('slice', 1), (8, 257, 64, 256), FWD, ('two_vec_rows', 9)),
    ('slice C * G >= 512', (7, 65, 73, 256), FWD, ('two_vec_rows', 3), (8, 65, 64, 256), FWD, ('slice', 1)),
    ('slice C * G >= 512 (channels)', (8, 65, 63, 256), FWD, ('two_vec_rows', 3), (8, 65, 64, 256), FWD, ('slice', 1)),
    ('slice C * G >= 512 (one group)', (1, 65, 511, 256), FWD, ('two_vec_rows', 3), (1, 65, 512, 256), FWD, ('slice', 1)),
    ('slice HW / 4 divides 1024', (1, 342, 512, 48), FWD, ('two_vec_cols', 3), (1, 257, 512, 64), FWD, ('slice', 1)),
    ('slice HW / 4 <= 1024', (1, 5, 512, 4096), FWD, ('slice', 1), (1, 3, 512, 8192), FWD, ('two_vec_cols', 3)),
    ('slice G <= 65535', (65535, 65, 1, 256), FWD, ('slice', 1), (65536, 65, 1, 256), FWD, ('two_vec_rows', 3)),
    ('slice is a forward form', (8, 65, 64, 256), FWD, ('slice', 1), (8, 65, 64, 256), BWD, ('two_vec_rows', 3)),
    ('slice needs float4 operands', (8, 65, 64, 256), FWD, ('slice', 1), (8, 65, 64, 256), U, ('two_scalar', 3)),
    ('slice at the workload shape', (18, 256, 64, 256), FWD, ('slice', 1), (18, 256, 64, 256), BWD, ('two_vec_rows', 8)),
    # --- the float4 path needs HW % 4 == 0 and aligned operands
    ('HW % 4', (4, 8, 4, 64), FWD, ('two_vec_rows', 1), (4, 8, 4, 63), FWD, ('two_scalar', 1)),
    ('aligned operands', (4, 8, 4, 64), FWD, ('two_vec_rows', 1), (4, 8, 4, 64), U, ('two_scalar', 1)),
    # --- bn_shape: a slice is floor(8192 / HW) rows, at least one, at most B
    ('rows = 8192 / HW', (4, 16, 2, 512), FWD, ('two_vec_rows', 1), (4, 17, 2, 512), FWD, ('two_vec_rows', 2)),
    ('rows >= 1', (4, 3, 2, 8192), FWD, ('two_vec_cols', 3), (4, 3, 2, 8196), FWD, ('two_vec_cols', 3)),
    ('rows floor', (4, 3, 2, 4096), FWD, ('two_vec_cols', 2), (4, 3, 2, 4100), FWD, ('two_vec_cols', 3)),
]


@pytest.mark.parametrize('gate', GATES, ids=[g[0] for g in GATES])
def test_gate_from_both_sides(gate):
    _, lo, lo_kw, lo_want, hi, hi_kw, hi_want = gate
    assert R(*lo, **lo_kw) == lo_want, (lo, lo_kw)
    assert R(*hi, **hi_kw) == hi_want, (hi, hi_kw)


def test_backward_and_unaligned_calls_never_take_the_slice_form():
    for G in (1, 2, 8, 18, 600):
        for C in (1, 64, 512, 600):
            for B, HW in ((65, 256), (256, 256), (17, 1024), (5, 4096), (4200, 4), (342, 48)):
                fwd = R(G, B, C, HW)[0]
                assert (fwd == 'slice') == (C * G >= 512 and HW != 48), (G, B, C, HW, fwd)
                assert R(G, B, C, HW, bwd=True)[0] in ('two_vec_rows', 'two_vec_cols'), (G, B, C, HW)
                assert R(G, B, C, HW, aligned=False)[0] == 'two_scalar', (G, B, C, HW)
                assert R(G, B, C, HW, bwd=True, aligned=False)[0] == 'two_scalar', (G, B, C, HW)


# ----------------------------------------------------------------------------- the two float4 sweeps
@pytest.mark.parametrize('HW', [4, 16, 64, 256, 1024])
def test_two_vec_rows(HW):
    """HW / 4 a power of two up to the 256 threads: a row per HW / 4 lanes, rows in parallel."""
    for bwd in (False, True):
        assert R(4, 2, 3, HW, bwd=bwd)[0] == 'two_vec_rows', (HW, bwd)
        assert R(1, 16384 // HW + 1, 3, HW, bwd=bwd)[0] == 'two_vec_rows', (HW, bwd)


@pytest.mark.parametrize('HW', [12, 36, 144, 784, 4096])
def test_two_vec_cols(HW):
    """HW / 4 no power of two (3, 9, 36, 196), or more float4 columns than threads (1024): lanes walk a row's columns."""
    for bwd in (False, True):
        assert R(4, 2, 3, HW, bwd=bwd)[0] == 'two_vec_cols', (HW, bwd)
        assert R(1, 16384 // HW + 1, 3, HW, bwd=bwd)[0] == 'two_vec_cols', (HW, bwd)


def test_rows_and_cols_split_at_every_width():
    """hw4 <= tx with tx the largest power of two <= min(hw4, 256): exactly the powers of two up to 256."""
    for hw4 in range(1, 2100):
        want = 'two_vec_rows' if hw4 <= 256 and hw4 & (hw4 - 1) == 0 else 'two_vec_cols'
        assert R(4, 2, 3, 4 * hw4)[0] == want, hw4


# ----------------------------------------------------------------------------- the slice bound
def _slices(B, HW):
    rows = min(max(8192 // HW, 1), B)
    return (B + rows - 1) // rows


FORMERLY_REFUSED = [(32, 56 * 56, 16, 14), (64, 48 * 48, 22, 20), (6, 72 * 72, 6, 5), (64, 4100, 64, 34)]


@pytest.mark.parametrize('B,HW,S,old_bound', FORMERLY_REFUSED)
def test_formerly_refused_shapes(B, HW, S, old_bound):
    """Ordinary BatchNorm2d shapes whose slice count passed n / 8192 + 2 (the floor of 8192 / HW loses up to half a slice)."""
    assert B * HW // 8192 + 2 == old_bound and S > old_bound
    for bwd in (False, True):
        for aligned in (True, False):
            route, slices, launches = K.bn_route(1, B, 2, HW, bwd=bwd, aligned=aligned)
            assert (route, slices, launches) == ('two_vec_cols' if aligned else 'two_scalar', S, 2)
    assert S * 2 * 12 <= _lib.lib().mvae_bn_ws_bytes(1, 2, B * HW)


def test_slice_count_fits_the_workspace_and_nothing_is_refused():
    """S <= mvae_bn_ws_bytes / (G * C * 12 bytes per record) for HW in 1 .. 9300 against nine batch sizes, none refused."""
    lib = _lib.lib()
    sl = ctypes.c_int(0)
    worst = 0.0
    for B in (1, 2, 3, 6, 32, 64, 255, 256, 2056):
        for HW in range(1, 9301):
            for bwd in (0, 1):
                rc = lib.mvae_bn_route(bwd, 1, B, 1, HW, 1, ctypes.byref(sl), None)
                assert rc > 0, (B, HW, bwd, rc)
                S = sl.value
                if _lib.BN_ROUTES[rc].startswith('two_'):
                    assert S == _slices(B, HW), (B, HW, S)
                else:
                    assert S == 1
                room = lib.mvae_bn_ws_bytes(1, 1, B * HW) // 12
                assert _slices(B, HW) <= room == B * HW // 4096 + 2, (B, HW, S, room)
                worst = max(worst, _slices(B, HW) / room)
    assert 0.5 < worst <= 1.0       # the bound is used, not slack by an order of magnitude
    # several groups and channels scale the room, not the slice count
    assert lib.mvae_bn_ws_bytes(3, 5, 32 * 3136) == 15 * lib.mvae_bn_ws_bytes(1, 1, 32 * 3136)
    assert lib.mvae_bn_ws_bytes(0, 5, 64) == 0 and lib.mvae_bn_ws_bytes(1, 1, 0) == 0


# ----------------------------------------------------------------------------- the query itself
def test_error_codes():
    lib = _lib.lib()
    for bwd in (0, 1):
        for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4), (4, 4, 4, -4)):
            assert refused(*bad, bwd=bwd), bad
        assert refused(1, 1 << 16, 1, 1 << 15, bwd=bwd)                        # B * HW = 2^31
        assert not refused(1, 1, 1, (1 << 31) - 1, bwd=bwd)                    # ... and one below
        assert refused(1 << 10, 1 << 10, 1 << 10, 1 << 10, bwd=bwd)            # G * B * C * HW = 2^40
        assert not refused((1 << 10) - 1, 1 << 10, 1 << 10, 1 << 10, bwd=bwd)
    assert R(1, 1, 1, (1 << 31) - 1) == ('two_scalar', 1)
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        K.bn_route(1, 0, 4, 4)
    # the out-pointers of a refused call are left alone
    sl, ln = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.mvae_bn_route(0, 0, 4, 4, 4, 1, ctypes.byref(sl), ctypes.byref(ln)) == -1
    assert (sl.value, ln.value) == (-7, -7)


def test_every_id_has_a_name():
    text = open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define\s+MVAE_BNROUTE_(\w+)\s+(\d+)', text)}
    assert len(ids) == 11 and sorted(ids.values()) == sorted(_lib.BN_ROUTES)
    for name, v in ids.items():
        assert _lib.BN_ROUTES[v] == name.lower(), name


def test_launch_counts_and_optional_out_pointers():
    lib = _lib.lib()
    seen = set()
    for G, B, C, HW in [(4, 2, 3, 64), (4, 2, 3, 36), (4, 2, 3, 25), (1, 64, 2, 256), (2, 64, 2, 256), (3, 64, 2, 256),
                        (1, 655, 2, 25), (2, 327, 2, 25), (1, 512, 17, 1), (3, 512, 1, 1), (8, 65, 64, 256),
                        (1, 2056, 1, 1024)]:
        for bwd in (False, True):
            name, slices, launches = K.bn_route(G, B, C, HW, bwd=bwd)
            two = name.startswith('two_')
            assert launches == (2 if two or name == 'slice' else 1), (name, launches)
            assert two or slices == 1, (name, slices)
            seen.add(name)
            rc = lib.mvae_bn_route(int(bwd), G, B, C, HW, 1, None, None)
            sl, ln = ctypes.c_int(0), ctypes.c_int(0)
            assert rc == lib.mvae_bn_route(int(bwd), G, B, C, HW, 1, ctypes.byref(sl), None)
            assert rc == lib.mvae_bn_route(int(bwd), G, B, C, HW, 1, None, ctypes.byref(ln))
            assert _lib.BN_ROUTES[rc] == name and (sl.value, ln.value) == (slices, launches)
    assert seen == set(_lib.BN_ROUTES.values())
    assert K.bn_route(1, 2056, 1, 1024)[1] == 257


def test_host_side_refusals_of_the_launches():
    """Checked in front of every launch, so no device is needed: exactly one of running_mean / running_var, and a record
    count that is no multiple of G."""
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for rm, rv in ((p, None), (None, p)):
        assert lib.mvae_bn_train_fwd(p, p, p, p, p, p, rm, rv, 1, 2, 2, 4, 1e-5, 0.1, 1, None, 0, p, 256, None) == -1
        assert lib.mvae_bn_stats_merge(p, 4, 512, 2, 2, p, p, rm, rv, 1e-5, 0.1, 1, None, None) == -1
    assert lib.mvae_bn_stats_merge(p, 5, 512, 2, 2, p, p, p, p, 1e-5, 0.1, 1, None, None) == -1      # 5 tiles, 2 groups
    assert lib.mvae_bn_stats_merge(p, 0, 512, 2, 2, p, p, p, p, 1e-5, 0.1, 1, None, None) == -1
