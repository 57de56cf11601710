"""GPU: the 4x4 conv kernels at the batch sizes where the dispatch of csrc/conv.hip changes kernel.

tests/test_kernels_gpu.py runs the conv launches at batches of 1-130, below almost every gate that selects the kernels
the shipped steps run.  Every case here
  * first asserts, through the host-only query ``kernels.conv_route`` (mvae_conv_k4_route: the decision function the
    launch itself switches on), WHICH kernel it is about to run -- a later change to a threshold fails that line instead
    of silently moving the case onto another kernel;
  * hands the launch views into larger NaN-filled device buffers (``Guarded``): >= 4096 floats of margin either side, at
    offsets that are multiples of 64 floats so the alignment gates hold.  The result must match the reference and hold no
    NaN (a position the kernel never writes, or a read outside an input, shows), and the margins of every buffer and
    every input must be bit-identical afterwards (a write outside the tensor shows);
  * compares with F.conv2d / F.conv_transpose2d / autograd in FLOAT64 on the CPU, cast to float32 at the end, at the
    project's own bound util.REL_TOL (1e-4 of max |ref|);
  * runs the launch in every output form it has: pre / pre + act / act, the producer's Swish' folded in (pre_in), the
    repacked weights made in the launch and ahead of it (bit-equal), weight gradients overwriting and accumulating.

Where the issue's case and the dispatch disagree (found with the query, kept as assertions in test_conv_routes_cpu.py):
  * wgrad_patch_kernel needs tiles x splits >= 256 with splits = target // tiles; a layer with THREE column blocks (24
    input channels) misses that at the small target (3 x (256 // 3) = 255) and reaches the kernel only once the launch
    aims at 512 blocks: from 1024 images of 32 x 32 (170 partials).  Conv2d(24, 64) runs here at 1024 images on the
    patch kernel and at the issue's 90 images of 16 x 16 on the gather launch;
  * the data gradient of Conv2d(64, 128) on 14 x 14 at 701 images is past the 7 x 7 gate: it is a patch-kernel case;
  * the statistics form of the patch kernel serves the 16 x 16 lattice only, where an image is two records of 128
    positions: a group always holds an EVEN number of records.  The odd count (5 per group) runs on the 8 x 8 lattice,
    i.e. on the gather launch's statistics form.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import mvae_amd
from mvae_amd import _lib
from mvae_amd import kernels as K
from util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 4096          # floats in front of and behind every view (a multiple of 64: the views stay 256-byte aligned)
NAN = float('nan')


def g64(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def swish(x):
    return x * torch.sigmoid(x)


def swish_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


class Guarded:
    """Device tensors as views into NaN-filled buffers; ``check()`` after the launches: margins and inputs untouched."""

    def __init__(self):
        self.items = []         # (name, buffer, snapshot of what must not change (int32 bits), whole buffer?)

    def _buf(self, n):
        body = (n + 63) // 64 * 64
        return torch.full((MARGIN + body + MARGIN,), NAN, dtype=torch.float32, device=DEV)

    def inp(self, t, name='in'):
        """An input: float64 CPU tensor -> float32 view; the WHOLE buffer must stay as it is."""
        buf = self._buf(t.numel())
        view = buf[MARGIN:MARGIN + t.numel()].view(t.shape)
        view.copy_(t.to(torch.float32))
        self.items.append((name, buf, buf.view(torch.int32).clone(), None))
        return view

    def out(self, shape, name='out', init=None):
        """An output: NaN (or ``init``) inside, NaN margins; the margins must stay as they are."""
        n = 1
        for d in shape:
            n *= d
        buf = self._buf(n)
        view = buf[MARGIN:MARGIN + n].view(shape)
        if init is not None:
            view.copy_(init.to(torch.float32))
        bits = buf.view(torch.int32)
        self.items.append((name, buf, (bits[:MARGIN].clone(), bits[MARGIN + n:].clone()), n))
        return view

    def check(self):
        for name, buf, snap, n in self.items:
            bits = buf.view(torch.int32)
            if n is None:
                assert torch.equal(bits, snap), 'input %s (or its margins) was written' % name
            else:
                assert torch.equal(bits[:MARGIN], snap[0]), 'write in front of %s' % name
                assert torch.equal(bits[MARGIN + n:], snap[1]), 'write behind %s' % name


def close(route, got, ref64, what):
    """No NaN, within REL_TOL of the float64 reference; the figure is printed (pytest -rP shows it per test)."""
    assert not torch.isnan(got).any().item(), '%s: NaN in the result (unwritten output or a read outside an input)' % what
    e = assert_close(got, ref64.to(torch.float32), what)
    print('ROUTE-ERR %-16s %-40s %.3e (bound %.0e)' % (route, what, e, REL_TOL))
    return e


def ws_bytes(need=0):
    """The scratch a wrapper that asks kernels.workspace for ``need`` bytes hands its launch (asked the same way: the
    scratch grows here exactly as it would in the wrapper)."""
    return K.workspace(need, torch.device(DEV, torch.cuda.current_device())).numel() * 4


def route_is(op, B, Cin, H, Cout, s, p, route, splits=None, need=0):
    got = K.conv_route(op, B, Cin, H, H, Cout, s, p, ws_bytes(need))
    assert got[0] == route, '%s %s runs %s, the case is about %s' % (op, (B, Cin, H, Cout, s, p), got[0], route)
    if splits is not None:
        assert got[1] == splits, '%s %s: %d partials, the case is about %d' % (op, (B, Cin, H, Cout, s, p), got[1], splits)


# ----------------------------------------------------------------------------- the four launch forms
def run_convT_fwd(B, Cin, H, Cout, route, s=2, p=1):
    """ConvTranspose2d(Cin, Cout) forward (a dgrad-form launch): pre / pre + act / act, weights repacked in the launch
    and ahead of it."""
    route_is('convT_fwd', B, Cin, H, Cout, s, p, route)
    x, w = g64(B, Cin, H, H, seed=70), g64(Cin, Cout, 4, 4, seed=71, scale=(Cin * 4) ** -0.5)
    y = F.conv_transpose2d(x, w, None, s, p)
    G = Guarded()
    xd, wd = G.inp(x, 'x'), G.inp(w, 'w')
    n = K.conv_repack_floats(True, wd, B, Cin, H, H, Cout, s, p)
    wr = None
    if n:
        wr = G.out((n,), 'wr')
        K.conv_repack_batched([(wd, wr, True, Cin, Cout, s, p)])
    outs = {}
    for form in ('pre', 'pre+act', 'act'):
        for ahead in ((False, True) if n else (False,)):
            pre = G.out(y.shape, 'pre') if 'pre' in form else None
            act = G.out(y.shape, 'act') if 'act' in form else None
            K.convT2d_fwd(xd, wd, pre, act, s, p, wr=wr if ahead else None)
            outs[form, ahead] = (pre, act)
    G.check()
    for (form, ahead), (pre, act) in outs.items():
        if not ahead:
            if pre is not None:
                close(route, pre, y, 'convT fwd [%s] pre' % form)
            if act is not None:
                close(route, act, swish(y), 'convT fwd [%s] act' % form)
        else:
            for a, b in zip(outs[form, False], (pre, act)):
                assert a is None or torch.equal(a, b), 'convT fwd [%s]: repack ahead != repack in the launch' % form


def run_conv_dgrad(B, Cin, H, Cout, route, s=2, p=1):
    """Data gradient of Conv2d(Cin, Cout) on H x H (a dgrad-form launch): dx, dx * swish'(pre_in), both weight copies."""
    route_is('conv_dgrad', B, Cin, H, Cout, s, p, route)
    OH = (H + 2 * p - 4) // s + 1
    dy, w = g64(B, Cout, OH, OH, seed=72), g64(Cout, Cin, 4, 4, seed=73, scale=(Cout * 4) ** -0.5)
    dx = F.conv_transpose2d(dy, w, None, s, p)
    assert dx.shape == (B, Cin, H, H)
    pre_in = g64(B, Cin, H, H, seed=74)
    G = Guarded()
    dyd, wd, pd = G.inp(dy, 'dy'), G.inp(w, 'w'), G.inp(pre_in, 'pre_in')
    n = K.conv_repack_floats(False, wd, B, Cin, H, H, Cout, s, p)
    wr = None
    if n:
        wr = G.out((n,), 'wr')
        K.conv_repack_batched([(wd, wr, False, Cin, Cout, s, p)])
    outs = {}
    for form in ('plain', 'swish'):
        for ahead in ((False, True) if n else (False,)):
            o = G.out(dx.shape, 'dx')
            K.conv2d_dgrad(dyd, wd, o, pd if form == 'swish' else None, s, p, wr=wr if ahead else None)
            outs[form, ahead] = o
    G.check()
    for (form, ahead), o in outs.items():
        if not ahead:
            close(route, o, dx if form == 'plain' else dx * swish_grad(pre_in), 'conv dgrad [%s]' % form)
        else:
            assert torch.equal(outs[form, False], o), 'conv dgrad [%s]: repack ahead != repack in the launch' % form


def run_conv_fwd(B, Cin, H, Cout, route, s=2, p=1):
    """Conv2d(Cin, Cout) forward: pre / pre + act / act."""
    route_is('conv_fwd', B, Cin, H, Cout, s, p, route)
    x, w = g64(B, Cin, H, H, seed=75), g64(Cout, Cin, 4, 4, seed=76, scale=(Cin * 16) ** -0.5)
    y = F.conv2d(x, w, None, s, p)
    G = Guarded()
    xd, wd = G.inp(x, 'x'), G.inp(w, 'w')
    outs = []
    for form in ('pre', 'pre+act', 'act'):
        pre = G.out(y.shape, 'pre') if 'pre' in form else None
        act = G.out(y.shape, 'act') if 'act' in form else None
        K.conv2d_fwd(xd, wd, pre, act, s, p)
        outs.append((form, pre, act))
    G.check()
    for form, pre, act in outs:
        if pre is not None:
            close(route, pre, y, 'conv fwd [%s] pre' % form)
        if act is not None:
            close(route, act, swish(y), 'conv fwd [%s] act' % form)


def run_convT_dgrad(B, Cin, H, Cout, route, s=2, p=1):
    """Data gradient of ConvTranspose2d(Cin, Cout) on H x H (a forward-form launch): dx and dx * swish'(pre_in)."""
    route_is('convT_dgrad', B, Cin, H, Cout, s, p, route)
    OH = (H - 1) * s - 2 * p + 4
    dy, w = g64(B, Cout, OH, OH, seed=77), g64(Cin, Cout, 4, 4, seed=78, scale=(Cout * 16) ** -0.5)
    dx = F.conv2d(dy, w, None, s, p)
    assert dx.shape == (B, Cin, H, H)
    pre_in = g64(B, Cin, H, H, seed=79)
    G = Guarded()
    dyd, wd, pd = G.inp(dy, 'dy'), G.inp(w, 'w'), G.inp(pre_in, 'pre_in')
    o1, o2 = G.out(dx.shape, 'dx'), G.out(dx.shape, 'dx swish')
    K.convT2d_dgrad(dyd, wd, o1, None, s, p)
    K.convT2d_dgrad(dyd, wd, o2, pd, s, p)
    G.check()
    close(route, o1, dx, 'convT dgrad [plain]')
    close(route, o2, dx * swish_grad(pre_in), 'convT dgrad [swish]')


@functools.lru_cache(maxsize=1)
def wgrad_reference(B, Cin, H, Cout, s, p):
    """(x, dy, dw, base) in float64, computed once for the conv and the transposed-conv form of a case; read only."""
    x = g64(B, Cin, H, H, seed=80)
    w = g64(Cout, Cin, 4, 4, seed=81, scale=(Cin * 16) ** -0.5).requires_grad_()
    y = F.conv2d(x, w, None, s, p)
    dy = g64(*y.shape, seed=82)
    y.backward(dy)
    dw = w.grad             # [Cout, Cin, 4, 4]: also the gradient of ConvTranspose2d(Cout, Cin)'s weight for (x = dy, dy = x)
    return x, dy, dw, g64(*dw.shape, seed=83, scale=dw.abs().max().item())


def run_wgrad(transposed, B, Cin, H, Cout, route, splits=None, s=2, p=1):
    """Weight gradient of Conv2d(Cin, Cout) on H x H -- or, transposed, of the mirrored ConvTranspose2d(Cout, Cin) on the
    small map, which is the same launch with the operands swapped: overwriting, then accumulating onto a base."""
    OH = (H + 2 * p - 4) // s + 1
    need = _lib.lib().mvae_gemm_ws_bytes(Cout, Cin * 16, B * OH * OH)      # what both wrappers ask kernels.workspace for
    if transposed:
        route_is('convT_wgrad', B, Cout, OH, Cin, s, p, route, splits, need)
    else:
        route_is('conv_wgrad', B, Cin, H, Cout, s, p, route, splits, need)
    x, dy, dw, base = wgrad_reference(B, Cin, H, Cout, s, p)
    G = Guarded()
    xd, dyd = G.inp(x, 'x'), G.inp(dy, 'dy')
    o1, o2 = G.out(dw.shape, 'dw'), G.out(dw.shape, 'dw accumulate', init=base)
    if transposed:
        K.convT2d_wgrad(xd, dyd, o1, s, p)                      # the transposed conv's dy is the big map, its x the small one
        K.convT2d_wgrad(xd, dyd, o2, s, p, accumulate=True)
    else:
        K.conv2d_wgrad(dyd, xd, o1, s, p)
        K.conv2d_wgrad(dyd, xd, o2, s, p, accumulate=True)
    G.check()
    what = 'convT wgrad' if transposed else 'conv wgrad'
    close(route, o1, dw, what)
    close(route, o2, base + dw, what + ' accumulate')


# ----------------------------------------------------------------------------- convT_patch2_kernel and the gather launch below its gate
# (B, Cin, H, Cout) of the ConvTranspose2d; J = B * H * H lattice positions in tiles of 64
PATCH_CONVT = [
    # 7 x 7, 64 rows (gate: 334 images).  334: the threshold, J % 64 = 46.  337: J % 64 = 1 -- the last tile holds ONE
    # position, the last of the last image, and would span two absent images.  338: J % 64 = 50 -- the last tile starts at
    # position 48 of image 336, holds all of image 337, the third image is absent.
    (334, 128, 7, 64, 'patch7'), (337, 128, 7, 64, 'patch7'), (338, 128, 7, 64, 'patch7'), (333, 128, 7, 64, 'igemm'),
    # 7 x 7, 32 rows (gate: 668).  669: 13 positions in the last tile, which would span three images; 670: 62, third absent
    (669, 64, 7, 32, 'patch7'), (670, 64, 7, 32, 'patch7'), (667, 64, 7, 32, 'igemm_pair'),
    # 8 x 8: one image per tile (gates: 256 / 512)
    (259, 128, 8, 64, 'patch8'), (255, 128, 8, 64, 'igemm'), (515, 64, 8, 32, 'patch8'), (511, 64, 8, 32, 'igemm_pair'),
    # 16 x 16: bands of four rows; the 32-row grid; ONE phase of 16 channels (no double-buffer hand-over); three phases
    (130, 64, 16, 32, 'patch16'), (127, 64, 16, 32, 'igemm_pair'),
    (66, 16, 16, 64, 'patch16'), (63, 16, 16, 64, 'igemm_pair'),
    (66, 48, 16, 64, 'patch16'), (63, 48, 16, 64, 'igemm_pair'),
]


@pytest.mark.parametrize('B,Cin,H,Cout,route', PATCH_CONVT)
def test_convT_fwd_across_the_patch_gate(B, Cin, H, Cout, route):
    run_convT_fwd(B, Cin, H, Cout, route)


# (B, Cin, H, Cout) of the Conv2d whose data gradient it is
PATCH_DGRAD = [
    (334, 64, 14, 128, 'patch7'), (337, 64, 14, 128, 'patch7'), (338, 64, 14, 128, 'patch7'), (333, 64, 14, 128, 'igemm'),
    (701, 64, 14, 128, 'patch7'),           # J = 34 349, J % 64 = 45 (the batch of the ragged gather cases below)
    (130, 32, 32, 64, 'patch16'), (127, 32, 32, 64, 'igemm_pair'),
]


@pytest.mark.parametrize('B,Cin,H,Cout,route', PATCH_DGRAD)
def test_conv_dgrad_across_the_patch_gate(B, Cin, H, Cout, route):
    run_conv_dgrad(B, Cin, H, Cout, route)


# ----------------------------------------------------------------------------- wgrad_patch_kernel and its three finish kernels
WGRAD_PATCH = [
    (17, 32, 32, 64, 'wgrad_patch', 64),    # 68 chunks over 64 splits (ragged q_lo / q_hi); the normal finish (17-64)
    (19, 64, 16, 128, 'wgrad_patch', 16),   # 19 chunks over 16 splits; the few finish (<= 16); two row blocks
    (65, 8, 32, 64, 'wgrad_patch', 256),    # 260 chunks over 256 splits; the wide finish (> 64); a single column block
    (15, 32, 32, 64, 'igemm', None), (15, 64, 16, 128, 'igemm', None),     # one batch below the gate: the gather launch
    # THREE column blocks (blockIdx.x = 0, 1, 2): out of reach at the small target -- 3 x (256 // 3) = 255 < 256, the issue's
    # 90 images run the gather launch -- and taken once the launch aims at 512 blocks (B x 4 chunks x 3 tiles >= 24 x 512):
    # 4096 chunks over 512 // 3 = 170 splits, ragged; the wide finish
    (90, 24, 16, 64, 'igemm', None), (1024, 24, 32, 64, 'wgrad_patch', 170),
]


@pytest.mark.parametrize('B,Cin,H,Cout,route,splits', WGRAD_PATCH)
@pytest.mark.parametrize('transposed', [False, True])
def test_wgrad_patch_and_its_finish_kernels(B, Cin, H, Cout, route, splits, transposed):
    run_wgrad(transposed, B, Cin, H, Cout, route, splits)


# ----------------------------------------------------------------------------- the <= 4-input-channel weight gradients
# (Cin, H, Cout, route, batch whose B * OH units exceed the 256 blocks x 8 waves: waves take several units, blocks clamped)
SMALLCIN = [
    (1, 64, 32, 'wgrad_smallcin2', 70),     # wgrad_smallcin2_kernel<1, 1, 1, 32>
    (1, 32, 32, 'wgrad_smallcin2', 130),    # wgrad_smallcin2_kernel<1, 1, 1, 16>
    (4, 16, 64, 'wgrad_smallcin', 260),     # no instantiation of the newer kernel: wgrad_smallcin_kernel<2, 2>
    (2, 8, 32, 'wgrad_smallcin', 520),      # wgrad_smallcin_kernel<1, 1>
    (3, 32, 64, 'wgrad_smallcin', 130),     # 64 channels with 3 inputs: wgrad_smallcin_kernel<2, 2>
]


@pytest.mark.parametrize('Cin,H,Cout,route,Bbig', SMALLCIN)
@pytest.mark.parametrize('big', [False, True])
@pytest.mark.parametrize('transposed', [False, True])
def test_small_cin_wgrad_instantiations(Cin, H, Cout, route, Bbig, big, transposed):
    B = Bbig if big else 5
    units = B * (H // 2)
    assert (units > 256 * 8) == big
    run_wgrad(transposed, B, Cin, H, Cout, route, min((units + 7) // 8, 256))


# ----------------------------------------------------------------------------- conv_small_fwd_kernel<., 32> / <., 16>
@pytest.mark.parametrize('B,route', [(513, 'small_fwd32'), (511, 'small_fwd16')])
def test_small_cin_forward_both_channel_groupings(B, route):
    """Conv2d(3, 32) on 64 x 64: from 1024 blocks of 32 channels on the 32-channel form, below it the 16-channel one; as a
    forward and -- with and without the producer's Swish' -- as the data gradient of ConvTranspose2d(32, 3)."""
    run_conv_fwd(B, 3, 64, 32, route)
    run_convT_dgrad(B, 32, 32, 3, route)


# ----------------------------------------------------------------------------- the gather launches at a ragged B * 49
def test_igemm_at_a_ragged_lattice():
    """Conv2d(64, 128) on 14 x 14 and ConvTranspose2d(128, 64) on 7 x 7 at 701 images: J = 34 349 columns (forward; not a
    multiple of any tile), a reduction of 34 349 (weight gradients; not a multiple of the k-tile, 64 partials)."""
    B = 701
    run_conv_fwd(B, 64, 14, 128, 'igemm')
    run_convT_dgrad(B, 128, 7, 64, 'igemm')
    run_wgrad(False, B, 64, 14, 128, 'igemm')
    run_wgrad(True, B, 64, 14, 128, 'igemm')        # ConvTranspose2d(128, 64) on 7 x 7


# ----------------------------------------------------------------------------- statistics-only form of the patch kernel
@pytest.mark.parametrize('H,route,per_group', [(16, 'patch_stats', 20), (8, 'igemm', 5)])
def test_convT_stats_with_groups_of_ten_images(H, route, per_group):
    """(G, B) = (3, 10), 64 -> 32 channels, J % 128 == 0 -- against float64 statistics, at the bound
    test_convT_stats_only_matches_conv_then_batchnorm holds the same launch to (1e-5).  On 16 x 16 (the patch kernel's
    statistics form) an image is two records of 128 positions, so a group holds an even number whatever its size: 20.
    The ODD count per group -- 5 -- exists on the 8 x 8 lattice only, which the gather launch's statistics form serves."""
    Gn, B, Cin, Cout = 3, 10, 64, 32
    route_is('convT_fwd_stats', Gn * B, Cin, H, Cout, 2, 1, route)
    x = g64(Gn * B, Cin, H, H, seed=60) * 0.8 + 0.3
    w = g64(Cin, Cout, 4, 4, seed=61, scale=(Cin * 4) ** -0.5)
    y = F.conv_transpose2d(x, w, None, 2, 1)
    rm = 0.05 * g64(Cout, seed=62)
    rv = 1 + 0.1 * torch.rand(Cout, generator=torch.Generator().manual_seed(63), dtype=torch.float64)
    rm0, rv0 = rm.clone(), rv.clone()
    means, invstds = [], []
    for gi in range(Gn):
        yg = y[gi * B:(gi + 1) * B]
        for _ in range(2):
            F.batch_norm(yg, rm, rv, None, None, True, 0.1, 1e-5)
        means.append(yg.mean(dim=(0, 2, 3)))
        invstds.append((yg.var(dim=(0, 2, 3), unbiased=False) + 1e-5).rsqrt())
    G = Guarded()
    xd, wd = G.inp(x, 'x'), G.inp(w, 'w')
    tiles = K.convT2d_stats_tiles(xd, wd, 2, 1)
    assert tiles == Gn * B * H * H // 128 == Gn * per_group
    part = K.convT2d_fwd_stats(xd, wd, 2, 1)
    assert part.shape == (tiles, Cout, 2) and not torch.isnan(part).any().item()
    sm, si = G.out((Gn, Cout), 'save_mean'), G.out((Gn, Cout), 'save_invstd')
    rmd, rvd = G.out((Cout,), 'running_mean', init=rm0), G.out((Cout,), 'running_var', init=rv0)
    K.bn_stats_merge(part, Gn, sm, si, rmd, rvd, n_updates=2)
    G.check()
    for got, ref, what in ((sm, torch.stack(means), 'group means'), (si, torch.stack(invstds), 'group invstd'),
                           (rmd, rm, 'running_mean'), (rvd, rv, 'running_var')):
        assert not torch.isnan(got).any().item(), what
        e = assert_close(got, ref.to(torch.float32), what, tol=1e-5)
        print('ROUTE-ERR %-16s %-40s %.3e (bound 1e-05)' % (route + ' stats', what, e))
