"""No GPU: which kernel every 4x4 conv launch takes (mvae_conv_k4_route, the decision function the launches of
csrc/conv.hip switch on), pinned for the shipped configurations and on both sides of every gate, so that a change to the
dispatch shows up here as a diff.  The GPU side -- that each of these kernels computes the right thing at these sizes -- is
tests/test_conv_routes_gpu.py."""
import ctypes
import os
import re

import pytest

import mvae_amd
from mvae_amd import _lib
from mvae_amd import kernels as K

WS = 64 << 20       # the scratch kernels.py hands every launch until one asks for more


def route(op, B, Cin, H, Cout, s=2, p=1, ws=WS):
    return K.conv_route(op, B, Cin, H, H, Cout, s, p, ws)


def raw(op, B, Cin, H, W, Cout, s, p, ws=WS):
    return _lib.lib().mvae_conv_k4_route(op, B, Cin, H, W, Cout, s, p, ws, None)


# Every conv-shaped launch of the BASELINE configurations (profiles/r06_*_by_shape.txt; MNIST has none), as
# (launch, B, Cin, H, Cout, stride, pad) of the MODULE and its INPUT map -> the kernel, and why.
FASHIONMNIST = [    # 1024 images, the decoder on the 2048 rows of two ELBO terms
    ('conv_fwd', 1024, 1, 28, 64, 2, 1, 'small_fwd16'),     # 1 input channel: direct kernel; 392 x 2 = 784 < 1024 blocks
    ('conv_fwd', 1024, 64, 14, 128, 2, 1, 'igemm'),         # the forward form has no patch kernel built in
    ('conv_dgrad', 1024, 64, 14, 128, 2, 1, 'patch7'),      # 7 x 7 lattice, 64 rows: 785 tiles x 2 >= 512
    ('conv_wgrad', 1024, 64, 14, 128, 2, 1, 'igemm'),       # wgrad_patch serves 8 x 8 / 16 x 16 lattices only
    ('conv_wgrad', 1024, 1, 28, 64, 2, 1, 'wgrad_smallcin2'),       # the (64, 1, p16) instantiation
    ('convT_fwd', 2048, 128, 7, 64, 2, 1, 'patch7'),        # 7 x 7, 64 rows, 1568 tiles
    ('convT_fwd', 2048, 64, 14, 1, 2, 1, 'dgrad_small3d'),  # 1 output channel, >= 1024 blocks, 64 % 4 == 0: rows by DMA
    ('convT_dgrad', 2048, 128, 7, 64, 2, 1, 'igemm'),       # a conv forward form with 64 input channels
    ('convT_dgrad', 2048, 64, 14, 1, 2, 1, 'small_fwd32'),  # conv forward form, 1 input channel: 784 x 2 >= 1024 blocks
    ('convT_wgrad', 2048, 128, 7, 64, 2, 1, 'igemm'),       # 7 x 7 lattice
    ('convT_wgrad', 2048, 64, 14, 1, 2, 1, 'wgrad_smallcin2'),
]
CELEBA = [          # 256 images, the decoder on 512 rows + 256 rows of the statistics-only pass
    ('conv_fwd', 256, 3, 64, 32, 2, 1, 'small_fwd16'),      # 3 input channels; 512 blocks of 32 channels < 1024
    ('conv_fwd', 256, 32, 32, 64, 2, 1, 'igemm'),
    ('conv_fwd', 256, 64, 16, 128, 2, 1, 'igemm'),
    ('conv_fwd', 256, 128, 8, 256, 1, 0, 'igemm'),
    ('conv_dgrad', 256, 128, 8, 256, 1, 0, 's1'),           # stride 1, 5 x 5: dense GEMM + col2im; 32 x 56 blocks < 6144
    ('conv_dgrad', 256, 64, 16, 128, 2, 1, 'patch8'),       # 8 x 8, 64 rows: 256 tiles x 2 = 512, the gate exactly
    ('conv_dgrad', 256, 32, 32, 64, 2, 1, 'patch16'),       # 16 x 16, 32 rows: 1024 tiles
    ('conv_wgrad', 256, 128, 8, 256, 1, 0, 'igemm'),        # stride 1
    ('conv_wgrad', 256, 64, 16, 128, 2, 1, 'wgrad_patch'),  # 8 x 8 lattice, 16 tiles x 16 splits
    ('conv_wgrad', 256, 32, 32, 64, 2, 1, 'wgrad_patch'),   # 16 x 16 lattice, 4 tiles x 64 splits
    ('conv_wgrad', 256, 3, 64, 32, 2, 1, 'wgrad_smallcin2'),        # the (32, 3, p32) instantiation
    ('convT_fwd', 512, 256, 5, 128, 1, 0, 's1'),
    ('convT_fwd', 256, 256, 5, 128, 1, 0, 's1'),
    ('convT_fwd', 512, 128, 8, 64, 2, 1, 'patch8'),
    ('convT_fwd', 256, 128, 8, 64, 2, 1, 'patch8'),         # the gate exactly
    ('convT_fwd', 512, 64, 16, 32, 2, 1, 'patch16'),
    ('convT_fwd_stats', 256, 64, 16, 32, 2, 1, 'patch_stats'),
    ('convT_fwd', 512, 32, 32, 3, 2, 1, 'dgrad_small3d'),   # 3 output channels, 2048 blocks
    ('convT_dgrad', 512, 256, 5, 128, 1, 0, 'igemm'),
    ('convT_dgrad', 512, 128, 8, 64, 2, 1, 'igemm'),
    ('convT_dgrad', 512, 64, 16, 32, 2, 1, 'igemm'),
    ('convT_dgrad', 512, 32, 32, 3, 2, 1, 'small_fwd32'),   # 1024 blocks of 32 channels
    ('convT_wgrad', 512, 256, 5, 128, 1, 0, 'igemm'),
    ('convT_wgrad', 512, 128, 8, 64, 2, 1, 'wgrad_patch'),
    ('convT_wgrad', 512, 64, 16, 32, 2, 1, 'wgrad_patch'),
    ('convT_wgrad', 512, 32, 32, 3, 2, 1, 'wgrad_smallcin2'),
]
CELEBA19 = CELEBA + [   # the same encoder / decoder; decoder passes of 256, 512 and 18 x 256 = 4608 rows
    ('convT_fwd', 4608, 256, 5, 128, 1, 0, 's1_wide'),      # 16 x 1152 blocks of 128 columns >= 6144
    ('convT_fwd', 4608, 128, 8, 64, 2, 1, 'patch8'),
    ('convT_fwd_stats', 4608, 64, 16, 32, 2, 1, 'patch_stats'),
    ('convT_fwd', 256, 64, 16, 32, 2, 1, 'patch16'),
    ('convT_fwd', 256, 32, 32, 3, 2, 1, 'dgrad_small2'),    # 1024 blocks of the LDS-staged form would be < 4 per CU: from memory
    ('convT_dgrad', 256, 256, 5, 128, 1, 0, 'igemm'),
    ('convT_dgrad', 256, 128, 8, 64, 2, 1, 'igemm'),
    ('convT_dgrad', 256, 64, 16, 32, 2, 1, 'igemm'),
    ('convT_dgrad', 256, 32, 32, 3, 2, 1, 'small_fwd16'),
    ('convT_wgrad', 256, 256, 5, 128, 1, 0, 'igemm'),
    ('convT_wgrad', 256, 128, 8, 64, 2, 1, 'wgrad_patch'),
    ('convT_wgrad', 256, 64, 16, 32, 2, 1, 'wgrad_patch'),
    ('convT_wgrad', 256, 32, 32, 3, 2, 1, 'wgrad_smallcin2'),
]


@pytest.mark.parametrize('config,table', [('fashionmnist', FASHIONMNIST), ('celeba', CELEBA), ('celeba19', CELEBA19)])
def test_routes_of_the_baseline_configurations(config, table):
    wrong = []
    for op, B, Cin, H, Cout, s, p, expect in table:
        got = route(op, B, Cin, H, Cout, s, p)[0]
        if got != expect:
            wrong.append('%s %s: %s, expected %s' % (op, (B, Cin, H, Cout, s, p), got, expect))
    assert not wrong, '%s: %s' % (config, '; '.join(wrong))


def test_finish_forms_of_the_baseline_weight_gradients():
    """The partial counts behind the finish kernels the profiles show: few (<= 16), normal (17-64), wide (> 64)."""
    assert route('conv_wgrad', 256, 64, 16, 128) == ('wgrad_patch', 16)
    assert route('conv_wgrad', 256, 32, 32, 64) == ('wgrad_patch', 64)
    assert route('conv_wgrad', 256, 3, 64, 32) == ('wgrad_smallcin2', 256)
    assert route('conv_wgrad', 1024, 1, 28, 64) == ('wgrad_smallcin2', 256)
    assert route('conv_fwd', 256, 3, 64, 32) == ('small_fwd16', 1)      # no finish launch: 1


# the patch kernel needs ceil(B * OH * OW / 64) * (rows / 32) >= 512 blocks (convt_patch_plan); below it the gather launch,
# with pair stores where the reduction is short enough (K = 4 x 64 channels <= 256)
@pytest.mark.parametrize('Cin,H,Cout,below,at,family,patch', [
    (128, 7, 64, 333, 334, 'igemm', 'patch7'),
    (64, 7, 32, 667, 668, 'igemm_pair', 'patch7'),
    (128, 8, 64, 255, 256, 'igemm', 'patch8'),
    (64, 8, 32, 511, 512, 'igemm_pair', 'patch8'),
    (64, 16, 32, 127, 128, 'igemm_pair', 'patch16'),
    (128, 16, 64, 63, 64, 'igemm', 'patch16'),
])
def test_patch_gate_flips_exactly_at_the_threshold(Cin, H, Cout, below, at, family, patch):
    assert route('convT_fwd', below, Cin, H, Cout)[0] == family
    assert route('convT_fwd', at, Cin, H, Cout)[0] == patch
    # ... and the data gradient of the mirrored Conv2d(Cout, Cin) on the map twice as large is the same launch
    assert route('conv_dgrad', below, Cout, 2 * H, Cin)[0] == family
    assert route('conv_dgrad', at, Cout, 2 * H, Cin)[0] == patch


def test_patch_kernel_serves_32_and_64_rows_only():
    assert route('convT_fwd', 4096, 64, 8, 16)[0] == 'igemm_pair'
    assert route('convT_fwd', 4096, 64, 8, 128)[0] == 'igemm_pair'
    assert route('convT_fwd', 4096, 24, 8, 64)[0] == 'igemm_pair'        # the reduction in phases of 16 channels
    assert route('convT_fwd', 4096, 64, 4, 32)[0] == 'igemm_pair'        # 4 x 4 lattice


@pytest.mark.parametrize('Cin,H,Cout,splits', [(32, 32, 64, 64), (64, 16, 128, 16)])
def test_wgrad_patch_gate_at_16_images(Cin, H, Cout, splits):
    """tiles x splits >= 256 with splits <= chunks of 64 positions: 4 tiles x 4 B chunks, 16 tiles x B chunks."""
    for op, a in (('conv_wgrad', (Cin, H, Cout)), ('convT_wgrad', (Cout, H // 2, Cin))):
        assert route(op, 15, *a)[0] == 'igemm'
        assert route(op, 16, *a) == ('wgrad_patch', splits)


def test_wgrad_patch_needs_scratch_for_256_over_tiles_partials():
    per_split = 64 * 32 * 16 * 4        # one partial of Conv2d(32, 64)'s gradient: 4 tiles, so 64 partials at least
    op = _lib.CONV_OPS['conv_wgrad']
    for B in (17, 64):
        assert route('conv_wgrad', B, 32, 32, 64, ws=64 * per_split) == ('wgrad_patch', 64)
        # one partial short: the patch kernel falls back to the gather launch, whose own plan wants 64 partials here as
        # well -- so the launch refuses (the wrappers in kernels.py never hand out less than 64 MiB)
        assert raw(op, B, 32, 32, 32, 64, 2, 1, 64 * per_split - 4) == -3
    # 3072 images aim at 512 blocks = 128 partials; scratch for 100 still runs the patch kernel, on 100
    assert route('conv_wgrad', 3072, 32, 32, 64) == ('wgrad_patch', 128)
    assert route('conv_wgrad', 3072, 32, 32, 64, ws=100 * per_split) == ('wgrad_patch', 100)
    assert raw(op, 3072, 32, 32, 32, 64, 2, 1, 63 * per_split) in (-3, 1)      # refused, or the gather launch: not the patch kernel


def test_wgrad_patch_takes_three_column_blocks_only_at_the_larger_target():
    """splits = target // tiles and tiles x splits >= 256.  The target is 256 blocks, and 512 once B x chunks per image x
    tiles >= 24 x 512.  With 3 tiles (Conv2d(24, 64)) the small target gives 3 x 85 = 255 < 256: the gather launch; the
    large one 3 x 170 = 510: the patch kernel, on 170 partials -- from 1024 images of 32 x 32 (4 chunks each), from 4096
    of 16 x 16."""
    for B in (16, 90, 1000, 1023):
        assert route('conv_wgrad', B, 24, 32, 64)[0] == 'igemm', B
    assert route('conv_wgrad', 1024, 24, 32, 64) == ('wgrad_patch', 170)
    assert route('convT_wgrad', 1023, 64, 16, 24)[0] == 'igemm'
    assert route('convT_wgrad', 1024, 64, 16, 24) == ('wgrad_patch', 170)
    for B in (16, 90, 4095):
        assert route('conv_wgrad', B, 24, 16, 64)[0] == 'igemm', B
    assert route('conv_wgrad', 4096, 24, 16, 64) == ('wgrad_patch', 170)
    # the same switch for a layer either target serves: 4 tiles, 64 partials below it and 128 from it
    assert route('conv_wgrad', 767, 32, 32, 64) == ('wgrad_patch', 64)
    assert route('conv_wgrad', 768, 32, 32, 64) == ('wgrad_patch', 128)
    # two column blocks at the small target: 128 partials wanted, so 128 chunks needed
    assert route('conv_wgrad', 90, 16, 16, 64)[0] == 'igemm'
    assert route('conv_wgrad', 128, 16, 16, 64) == ('wgrad_patch', 128)


def test_small_cin_wgrad_instantiations():
    for Cin, H, Cout, expect in [(3, 64, 32, 'wgrad_smallcin2'), (1, 28, 64, 'wgrad_smallcin2'), (1, 64, 32, 'wgrad_smallcin2'),
                                 (1, 32, 32, 'wgrad_smallcin2'), (4, 16, 64, 'wgrad_smallcin'), (2, 8, 32, 'wgrad_smallcin'),
                                 (3, 32, 64, 'wgrad_smallcin'), (3, 32, 48, 'igemm'), (5, 32, 32, 'igemm')]:
        assert route('conv_wgrad', 5, Cin, H, Cout)[0] == expect, (Cin, H, Cout)
    # one partial per block of 8 (image, row) units, at most 256 blocks
    assert route('conv_wgrad', 5, 1, 64, 32) == ('wgrad_smallcin2', 20)
    assert route('conv_wgrad', 70, 1, 64, 32) == ('wgrad_smallcin2', 256)
    # without scratch for the 20 partials: not this kernel (and the gather launch it falls back to wants more still)
    assert raw(_lib.CONV_OPS['conv_wgrad'], 5, 1, 64, 64, 32, 2, 1, 19 * 32 * 16 * 4) == -3


def test_small_cin_forward_takes_32_channel_groups_from_1024_blocks():
    assert route('conv_fwd', 511, 3, 64, 32)[0] == 'small_fwd16'
    assert route('conv_fwd', 512, 3, 64, 32)[0] == 'small_fwd32'
    assert route('convT_dgrad', 511, 32, 32, 3)[0] == 'small_fwd16'
    assert route('convT_dgrad', 512, 32, 32, 3)[0] == 'small_fwd32'
    assert route('conv_fwd', 4, 3, 64, 24)[0] == 'small_fwd32'           # 24 channels: no 16-channel groups
    assert route('conv_fwd', 4, 5, 64, 32)[0] == 'igemm'


def test_stride1_wide_form_from_6144_blocks():
    # ConvTranspose2d(256, 128) on 5 x 5: 5 images per block, the image groups rounded up to a multiple of 8, 16 column
    # blocks of 128: 16 x 384 = 6144 from ceil(B / 5) = 377 groups
    assert route('convT_fwd', 1880, 256, 5, 128, 1, 0)[0] == 's1'
    assert route('convT_fwd', 1881, 256, 5, 128, 1, 0)[0] == 's1_wide'
    assert route('conv_dgrad', 1881, 128, 8, 256, 1, 0)[0] == 's1_wide'   # the mirrored Conv2d's data gradient


def test_statistics_only_launch():
    assert route('convT_fwd_stats', 30, 64, 16, 32)[0] == 'patch_stats'
    assert route('convT_fwd_stats', 32, 64, 8, 32)[0] == 'igemm'          # 8 x 8 lattice: the gather launch's records
    assert raw(_lib.CONV_OPS['convT_fwd_stats'], 3, 64, 7, 7, 32, 2, 1) == -1        # J % 128 != 0: not covered
    assert raw(_lib.CONV_OPS['convT_fwd_stats'], 32, 64, 16, 16, 64, 2, 1) == -1     # > 32 output channels


def test_bad_arguments():
    ok = (_lib.CONV_OPS['conv_fwd'], 4, 3, 64, 64, 32, 2, 1)
    assert raw(*ok) > 0
    for bad in [(-1,) + ok[1:], (7,) + ok[1:],                          # no such launch
                (0, 0, 3, 64, 64, 32, 2, 1), (0, -4, 3, 64, 64, 32, 2, 1),   # no images
                (0, 4, 0, 64, 64, 32, 2, 1), (0, 4, 3, 64, 64, 0, 2, 1),     # no channels
                (0, 4, 3, 64, 64, 32, 3, 1), (0, 4, 3, 64, 64, 32, 0, 1),    # stride
                (0, 4, 3, 2, 2, 32, 1, 0),                                   # map smaller than the kernel
                (3, 4, 3, 64, 64, 32, 3, 1), (3, 0, 3, 64, 64, 32, 2, 1), (6, 4, 3, 0, 0, 32, 2, 1)]:
        assert raw(*bad) == -1, bad
    n = ctypes.c_int(-7)
    assert _lib.lib().mvae_conv_k4_route(7, 4, 3, 64, 64, 32, 2, 1, WS, ctypes.byref(n)) == -1 and n.value == -7
    with pytest.raises(RuntimeError):
        K.conv_route('conv_fwd', 0, 3, 64, 64, 32, 2, 1)
    # a dgrad-form launch without room for its repacked weights
    assert raw(_lib.CONV_OPS['convT_fwd'], 4, 128, 8, 8, 64, 2, 1, ws=128 * 64 * 16 * 4 - 4) == -3
    assert raw(_lib.CONV_OPS['convT_fwd'], 4, 32, 32, 32, 3, 2, 1, ws=0) > 0    # a direct kernel: no scratch


def test_splits_pointer_is_optional_and_every_route_has_a_name():
    assert raw(_lib.CONV_OPS['conv_wgrad'], 17, 32, 32, 32, 64, 2, 1) > 0
    n = ctypes.c_int(0)
    rc = _lib.lib().mvae_conv_k4_route(_lib.CONV_OPS['conv_wgrad'], 17, 32, 32, 32, 64, 2, 1, WS, ctypes.byref(n))
    assert _lib.CONV_ROUTES[rc] == 'wgrad_patch' and n.value == 64
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mvae_hip.h')).read()
    codes = {name.lower(): int(v) for name, v in re.findall(r'#define MVAE_ROUTE_(\w+)\s+(\d+)', text)}
    assert codes == {v: k for k, v in _lib.CONV_ROUTES.items()}
    ops = {name: int(v) for name, v in re.findall(r'#define MVAE_OP_(\w+)\s+(\d+)', text)}
    assert ops == {k.upper(): v for k, v in _lib.CONV_OPS.items()}
