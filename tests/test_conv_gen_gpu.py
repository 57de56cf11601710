"""GPU: the general stride-2 conv family (csrc/conv_gen.hip; ks in {4, 5}, stride 2, pad in {0, 1}, any map size).

Conventions of tests/test_conv_routes_gpu.py: every launch gets views into larger NaN-filled device buffers
(``Guarded``) whose margins -- and the inputs -- must be bit-identical afterwards; results hold no NaN and match
F.conv2d / F.conv_transpose2d / autograd in FLOAT64 on the CPU, cast to float32, at util.REL_TOL.  Every case runs all
six launches: the case's own module (Conv2d or ConvTranspose2d: forward, data gradient, weight gradient) and its mirror
(the transposed module on the case's output map, resp. the conv on it).  Forward: pre only, act only, both; data
gradient: with and without the producer's pre-activation; weight gradient: overwriting, then accumulating onto a
non-zero ``dw``.  Everything runs twice on the same inputs and must come out bit-identical (no atomics, fixed-order
split reductions).

Cases: tiny ragged non-square maps (odd sizes, one partial tile, 1 x 1 input), then MultiMNIST's four geometries at
full channel counts at batches that cross the 32- / 64- / 128-column tiles and make the four parity classes unequal
(25 x 25: lattices 13 x 13, 13 x 12, 12 x 13, 12 x 12); the 6 -> 2 and 2 -> 6 layers at B = 1, 37, 100 take the
32 x 32-tile kernel whose four waves split the 2048-long reduction (B = 1, 37) and the 64 x 64 one (B = 100 mirror)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from test_conv_routes_gpu import Guarded, close, g64, swish, swish_grad

pytestmark = pytest.mark.gpu

# (name, transposed, B, Cin, Cout, ks, pad, H, W): the MODULE's channels and its input map
CASES = [
    ('tiny-9x11-k4p1', False, 2, 3, 5, 4, 1, 9, 11),
    ('tiny-T4x3-k5p1', True, 3, 5, 7, 5, 1, 4, 3),
    ('tiny-6x6-k4p0', False, 1, 4, 6, 4, 0, 6, 6),
    ('tiny-T1x1-k4p0', True, 2, 6, 4, 4, 0, 1, 1),
    ('tiny-7x9-k5p0', False, 2, 3, 5, 5, 0, 7, 9),
    ('mm-conv32-64-B3', False, 3, 32, 64, 4, 1, 25, 25),
    ('mm-conv32-64-B100', False, 100, 32, 64, 4, 1, 25, 25),
    ('mm-conv128-256-B1', False, 1, 128, 256, 4, 0, 6, 6),
    ('mm-conv128-256-B37', False, 37, 128, 256, 4, 0, 6, 6),
    ('mm-conv128-256-B100', False, 100, 128, 256, 4, 0, 6, 6),
    ('mm-convT256-128-B1', True, 1, 256, 128, 4, 0, 2, 2),
    ('mm-convT256-128-B37', True, 37, 256, 128, 4, 0, 2, 2),
    ('mm-convT256-128-B100', True, 100, 256, 128, 4, 0, 2, 2),
    ('mm-convT64-32-k5-B3', True, 3, 64, 32, 5, 1, 12, 12),
    ('mm-convT64-32-k5-B100', True, 100, 64, 32, 5, 1, 12, 12),
]


def out_map(transposed, H, W, ks, p):
    if transposed:
        return (H - 1) * 2 - 2 * p + ks, (W - 1) * 2 - 2 * p + ks
    return (H + 2 * p - ks) // 2 + 1, (W + 2 * p - ks) // 2 + 1


@functools.lru_cache(maxsize=None)
def reference(transposed, B, Cin, Cout, ks, p, H, W):
    """float64 CPU: x, w, y, dy, pre_in, dx, dw, dw0 of one module (computed once per geometry)."""
    x = g64(B, Cin, H, W, seed=11).requires_grad_()
    wshape = (Cin, Cout, ks, ks) if transposed else (Cout, Cin, ks, ks)
    w = g64(*wshape, seed=12, scale=(Cin * ks * ks / (4 if transposed else 1)) ** -0.5).requires_grad_()
    y = F.conv_transpose2d(x, w, None, 2, p) if transposed else F.conv2d(x, w, None, 2, p)
    assert tuple(y.shape[2:]) == out_map(transposed, H, W, ks, p)
    dy = g64(*y.shape, seed=13)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    return dict(x=x.detach(), w=w.detach(), y=y.detach(), dy=dy, pre_in=g64(B, Cin, H, W, seed=14), dx=dx, dw=dw,
                dw0=g64(*wshape, seed=15))


def run_family(transposed, B, Cin, Cout, ks, p, H, W):
    """The three launches of one module in every output form; returns the outputs (for the determinism comparison)."""
    r = reference(transposed, B, Cin, Cout, ks, p, H, W)
    tag = '%s(%d,%d,k%d,p%d) %dx%dx%d' % ('convT' if transposed else 'conv', Cin, Cout, ks, p, B, H, W)
    fwd, dgrad, wgrad = ((K.convT2d_gen_fwd, K.convT2d_gen_dgrad, K.convT2d_gen_wgrad) if transposed else
                         (K.conv2d_gen_fwd, K.conv2d_gen_dgrad, K.conv2d_gen_wgrad))
    assert K.conv_gen_supported(transposed, B, Cin, H, W, Cout, ks, 2, p)
    G = Guarded()
    xd, wd, dyd, pd = G.inp(r['x'], 'x'), G.inp(r['w'], 'w'), G.inp(r['dy'], 'dy'), G.inp(r['pre_in'], 'pre_in')
    outs = []
    for form in ('pre', 'act', 'pre+act'):
        pre = G.out(r['y'].shape, 'pre') if 'pre' in form else None
        act = G.out(r['y'].shape, 'act') if 'act' in form else None
        fwd(xd, wd, pre, act, 2, p)
        outs += [(pre, r['y'], '%s fwd [%s] pre' % (tag, form)), (act, swish(r['y']), '%s fwd [%s] act' % (tag, form))]
    for form in ('plain', 'swish'):
        o = G.out(r['dx'].shape, 'dx')
        dgrad(dyd, wd, o, pd if form == 'swish' else None, 2, p)
        outs.append((o, r['dx'] if form == 'plain' else r['dx'] * swish_grad(r['pre_in']), '%s dgrad [%s]' % (tag, form)))
    dw = G.out(r['dw'].shape, 'dw')
    wgrad(dyd, xd, dw, 2, p)
    dw2 = G.out(r['dw'].shape, 'dw2', init=r['dw0'])
    wgrad(dyd, xd, dw2, 2, p, accumulate=True)
    outs += [(dw, r['dw'], '%s wgrad [overwrite]' % tag), (dw2, r['dw0'] + r['dw'], '%s wgrad [accumulate]' % tag)]
    torch.cuda.synchronize()
    G.check()
    got = []
    for o, ref, what in outs:
        if o is not None:
            close('gen', o, ref, what)
            got.append(o.clone())
    return got


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_gen_family_all_six_launches(case):
    _, transposed, B, Cin, Cout, ks, p, H, W = case
    OH, OW = out_map(transposed, H, W, ks, p)
    first = run_family(transposed, B, Cin, Cout, ks, p, H, W)             # the case's own module
    first += run_family(not transposed, B, Cout, Cin, ks, p, OH, OW)      # its mirror, on the case's output map
    again = run_family(transposed, B, Cin, Cout, ks, p, H, W)
    again += run_family(not transposed, B, Cout, Cin, ks, p, OH, OW)
    for i, (a, b) in enumerate(zip(first, again)):
        assert torch.equal(a, b), 'output %d differs between two runs on the same inputs' % i


REJECTS = [   # (what, transposed, B, Cin, H, W, Cout, ks, stride, pad)
    ('ks=3', False, 2, 3, 8, 8, 4, 3, 2, 1),
    ('stride=1', False, 2, 3, 8, 8, 4, 4, 1, 1),
    ('pad=2', False, 2, 3, 8, 8, 4, 4, 2, 2),
    ('H+2pad<ks', False, 2, 3, 2, 8, 4, 4, 2, 0),
    ('ks=3 transposed', True, 2, 3, 4, 4, 4, 3, 2, 1),
    ('stride=1 transposed', True, 2, 3, 4, 4, 4, 5, 1, 1),
    ('pad=2 transposed', True, 2, 3, 4, 4, 4, 4, 2, 2),
]


@pytest.mark.parametrize('rej', REJECTS, ids=[r[0] for r in REJECTS])
def test_outside_the_domain_is_refused(rej):
    _, transposed, B, Cin, H, W, Cout, ks, s, p = rej
    assert not K.conv_gen_supported(transposed, B, Cin, H, W, Cout, ks, s, p)
    dev = 'cuda'
    x = torch.zeros(B, Cin, H, W, device=dev)
    w = torch.zeros((Cin, Cout, ks, ks) if transposed else (Cout, Cin, ks, ks), device=dev)
    y = torch.full((B, Cout, 16, 16), 7.0, device=dev)          # never written: the launch is refused on the host
    dx, dw = torch.full_like(x, 7.0), torch.full_like(w, 7.0)
    fwd, dgrad, wgrad = ((K.convT2d_gen_fwd, K.convT2d_gen_dgrad, K.convT2d_gen_wgrad) if transposed else
                         (K.conv2d_gen_fwd, K.conv2d_gen_dgrad, K.conv2d_gen_wgrad))
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        fwd(x, w, y, None, s, p)
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        dgrad(y, w, dx, None, s, p)
    with pytest.raises(RuntimeError, match='MVAE_ERR_ARG'):
        wgrad(y, x, dw, s, p)
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 and float(dx.min()) == 7.0 and float(dw.min()) == 7.0
