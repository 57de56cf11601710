"""GPU: every Linear kernel instantiation the dispatch of csrc/linear.hip can reach, at the cheapest shape that reaches it.

tests/test_kernels_gpu.py runs the Linear launches at 17 + 6 + 4 shapes and four batches; by the route query those reach
33 of the 94 (launch, kernel instantiation, finish launch) combinations run here and 3 of the 9 reachable
wgrad_batched2_kernel forms.  Every case here
  * first asserts, through the host-only queries ``kernels.linear_route`` / ``kernels.linear_wgrad_batched_route`` (the route
    functions the launches themselves switch on), WHICH kernel it is about to run, into how many partials the reduction is
    split and which launch sums them -- a later change to a threshold fails that line instead of moving the case;
  * hands the launch views into NaN-filled guarded buffers (``Guarded`` of tests/test_conv_routes_gpu.py): no NaN may be
    left in an output, margins and inputs must be bit-unchanged;
  * compares with a float64 CPU reference (x @ w.T + b, Swish, mask; dy @ w times Swish' times mask; dy.T @ x and dy.sum(0);
    oracle.functional's BCE / CE on the float64 logits) at util.REL_TOL, 1e-5 for the fused-loss rows and logits;
  * runs every launch twice into separate outputs and requires equal bits.  No Linear route sums through an atomic (the
    split reductions write partial slabs that a finish launch adds in a fixed order; the k-groups of a block add through LDS
    in group order), so no route is exempt.
Shapes: the last row tile, the last column tile and the last k-step are partial (K off a multiple of 64 on gemm2s and the
small layouts, of 32 on the large ones, of 16 on gemm2; "off by 4" where float4 loaders need multiples of 4), at least two
tiles either way, and on a split the last k range is shorter than the others (K is no multiple of 32).

What the query showed against the issue's list (M x N x K):
  * forward 300 x 1028 x 8 runs gemm2s 32 x 32 with 4 k-groups, 2048 x 260 x 8 gemm2s 64 x 32 with 4, the data gradient
    4100 x 20 x 132 gemm2s 64 x 32 with 2; forward 100 x 2048 x 4096 is 64 x 128 with 16 partials as stated;
  * gemm2s 32 x 64 / 64 x 32 with 2 k-groups need more than 320 two-tile blocks: one side of ~5000 for one group,
    ~2500 for three -- the three-group launches are the cheaper cases and are the ones run;
  * a single weight gradient reaches igemm_kernel only outside wgrad_direct_ok (fewer than 16 or more than 2048 tiles of
    32 x 32, more than 4096 rows): five of the six small layouts need G > 1;
  * unreachable for any input, no case: igemm_kernel's BK = 64 layouts under EpRowMajor from the forward and the data
    gradient (launch_gemm2s has all six and is asked first); wgrad_batched2_kernel<16, 2, 2, 1> (fewer than 160 tiles of
    64 x 64 are fewer than 640 of 32 x 32: at most 3 units on the busiest CU against 4); the 128-row igemm tiles (conv
    plans); g2_finish_kernel and the persistent gemm2 modes (tuning builds); finish_few_kernel behind a float4 forward on
    64 x 64 tiles needs N % 4 != 0, which the scalar-loader cases cover on the same kernel;
  * the categorical term has one column tile (N <= 32): past 224 blocks it takes the tall 64 x 32 layout, so 32 x 32 with 4
    k-groups, 32 x 64 and the 64 x 128 tile are out of its reach;
  * the split caps 64 / 512 bind on the narrow plan only; the 128-partial case below is past the 64 cap (4 tiles).
"""
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib
from mvae_amd import kernels as K
from oracle import functional as OF
from test_conv_routes_gpu import Guarded, close, g64, swish, swish_grad, ws_bytes
from util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
NO = (1, None)


def route_is(op, M, N, Kd, want, G=1, **kw):
    I, J, R = {'fwd': (M, N, Kd), 'dgrad': (M, Kd, N), 'wgrad': (N, Kd, M)}.get(op, (M, N, Kd))
    if op in ('fwd', 'dgrad', 'wgrad'):
        kw['ws_bytes'] = ws_bytes(G * _lib.lib().mvae_gemm_ws_bytes(I, J, R))
    got = K.linear_route(op, M, N, Kd, G=G, **kw)
    assert got == tuple(want), '%s %s G=%d %s runs %s, the case is about %s' % (op, (M, N, Kd), G, kw, got, tuple(want))


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s: two runs of one launch differ' % what


def keep_mask(shape, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) < 0.9).to(torch.float64)


def params(G_, shapes, pad, seed, scale):
    """The parameters of G groups at a uniform stride inside one flat buffer with NaN padding between them (the experts'
    slices of the parameter arena): float64 tensors [G, ...], the flat float64 image, the stride in floats."""
    n = 1
    for d in shapes:
        n *= d
    stride = (n + pad + 3) // 4 * 4
    vals = g64(G_, *shapes, seed=seed, scale=scale)
    flat = torch.full((G_ * stride,), NAN, dtype=torch.float64)
    for i in range(G_):
        flat[i * stride:i * stride + n] = vals[i].reshape(-1)
    return vals, flat, stride, n


# ----------------------------------------------------------------------------- forward
def run_fwd(M, N, Kd, route, G=1, how='aligned', alt=None):
    """``route``: (name, partials, finish) of every form, or of the forms ``alt`` does not name: {form: route}.
    how: 'aligned', 'offset' (x one float off 16 bytes), 'ldx' (x a column slice with a leading dimension % 4 == 2),
    'slice' (x a column slice at a multiple of 4, y a column block of a wider buffer)."""
    alt = alt or {}
    ldx = Kd + {'ldx': 2, 'slice': 8}.get(how, 0)
    ldy = N + (12 if how == 'slice' else 0)
    forms = ('pre', 'pre+act', 'act') + (('act*mask', 'pre nobias') if G == 1 else ())     # the grouped launch takes no mask
    for form in forms:
        qform = form if form in ('pre+act', 'act') else 'other'
        route_is('fwd', M, N, Kd, alt.get(form, route), G, form=qform, aligned=how != 'offset', ld_a=ldx, ld_b=ldy,
                 **({'gs_a': M * ldx, 'gs_b': (N * Kd + 40 + 3) // 4 * 4} if G > 1 else {}))
    gd = Guarded()
    sc = Kd ** -0.5
    if G == 1:
        x, w, b = g64(M, Kd, seed=11), g64(N, Kd, seed=12, scale=sc), g64(N, seed=13)
        ref = x @ w.t() + b
        ref_nb = x @ w.t()
        if how == 'offset':
            xp = torch.cat([torch.zeros(3, dtype=torch.float64), x.reshape(-1)])
            xd = gd.inp(xp, 'x')[3:].view(M, Kd)
            assert xd.data_ptr() % 16 == 12
        elif how in ('ldx', 'slice'):
            xp = torch.full((M, ldx), NAN, dtype=torch.float64)        # the columns beside the slice are never to be read
            c0 = 4 if how == 'slice' else 0
            xp[:, c0:c0 + Kd] = x
            xd = gd.inp(xp, 'x')[:, c0:c0 + Kd]
        else:
            xd = gd.inp(x, 'x')
        wd, bd = gd.inp(w, 'w'), gd.inp(b, 'b')
    else:
        assert how == 'aligned'
        x = g64(G, M, Kd, seed=11)
        w, wflat, w_gs, _ = params(G, (N, Kd), 40, 12, sc)
        b, bflat, b_gs, _ = params(G, (N,), 8, 13, 1.0)
        ref = torch.einsum('gmk,gnk->gmn', x, w) + b[:, None, :]
        xd, wf, bf = gd.inp(x, 'x'), gd.inp(wflat, 'w'), gd.inp(bflat, 'b')
        wd, bd = wf[:N * Kd].view(N, Kd), bf[:N]
    mask = keep_mask((M, N), 14) if G == 1 else None
    md = gd.inp(mask, 'mask') if G == 1 else None

    parents = []

    def out(name):
        if how == 'slice':
            parents.append(gd.out((M, ldy), name))
            return parents[-1][:, 8:8 + N]
        return gd.out((G, M, N) if G > 1 else (M, N), name)

    def launch(form):
        pre = out('pre') if form in ('pre', 'pre+act', 'pre nobias') else None
        act = out('act') if form in ('pre+act', 'act', 'act*mask') else None
        if G > 1:
            K.linear_fwd_grouped(xd, wd, w_gs, bd, b_gs, pre, act)
        elif form == 'act*mask':
            K.linear_fwd(xd, wd, bd, None, act, md, 1 / 0.9)
        else:
            K.linear_fwd(xd, wd, None if form == 'pre nobias' else bd, pre, act)
        return pre, act
    runs = {f: (launch(f), launch(f)) for f in forms}
    gd.check()
    name = route[0]
    for f, ((pre, act), (pre2, act2)) in runs.items():
        rname = alt.get(f, route)[0]
        r = ref_nb if f == 'pre nobias' else ref
        if pre is not None:
            close(rname, pre, r, 'fwd [%s] pre' % f)
            same_bits(pre, pre2, 'fwd [%s] pre' % f)
        if act is not None:
            close(rname, act, swish(r) * (mask / 0.9 if f == 'act*mask' else 1.0), 'fwd [%s] act' % f)
            same_bits(act, act2, 'fwd [%s] act' % f)
    if alt.get('pre', route)[0] == alt.get('pre+act', route)[0]:
        same_bits(runs['pre'][0][0], runs['pre+act'][0][0], 'fwd pre of [pre] and of [pre+act] (%s)' % name)
    if alt.get('act', route)[0] == alt.get('pre+act', route)[0]:
        same_bits(runs['act'][0][1], runs['pre+act'][0][1], 'fwd act of [act] and of [pre+act] (%s)' % name)
    for parent in parents:      # y as a column block of a wider buffer: the columns beside it stay NaN
        assert torch.isnan(parent[:, :8]).all() and torch.isnan(parent[:, 8 + N:]).all(), 'write beside the output columns'


G2S_ON = 'gemm2s block re-map on (tiles_i % 8 == 0)'
XCD_ON = 'igemm xcd_map on (grid.x % 2 == 0, grid.y % 4 == 0)'
FWD_CASES = [
    # gemm2s: six instantiations, Q_RK = true
    (36, 36, 68, ('g2s_32x32_k8',) + NO, 1, 'aligned', None),
    (228, 36, 68, ('g2s_32x32_k8',) + NO, 1, 'aligned', G2S_ON),                 # 8 row tiles
    (36, 5124, 68, ('g2s_32x32_k4',) + NO, 1, 'aligned', None),
    (68, 4100, 68, ('g2s_32x64_k4',) + NO, 1, 'aligned', None),
    (4100, 68, 68, ('g2s_64x32_k4',) + NO, 1, 'aligned', None),
    (4036, 68, 68, ('g2s_64x32_k4',) + NO, 1, 'slice', G2S_ON),                  # 64 row tiles
    (68, 2564, 68, ('g2s_32x64_k2',) + NO, 3, 'aligned', None),
    (2564, 68, 68, ('g2s_64x32_k2',) + NO, 3, 'aligned', None),
    (68, 1284, 132, ('g2s_32x64_k4',) + NO, 3, 'aligned', None),
    # igemm large layouts, float4 loaders
    (68, 8196, 36, ('ig_64x64',) + NO, 1, 'aligned', None),
    (196, 4036, 36, ('ig_64x64',) + NO, 1, 'aligned', XCD_ON),                   # grid 64 x 4
    (68, 8196, 68, ('ig_64x64', 2, 'finish_few_vec'), 1, 'slice', None),
    (68, 68, 1028, ('ig_64x64_k4', 17, 'finish'), 1, 'aligned', None),
    (68, 452, 1028, ('ig_64x64_k4', 11, 'finish_few_vec'), 1, 'aligned', None),
    (68, 132, 1028, ('ig_64x64_k4', 11, 'finish_few_vec'), 3, 'aligned', None),
    (68, 644, 1028, ('ig_64x64_k2', 4, 'finish_few_vec'), 3, 'aligned', None),
    (68, 2052, 4100, ('ig_64x128', 15, 'finish_few_vec'), 1, 'aligned', None),
    (17, 132, 1028, ('ig_32x128', 17, 'finish'), 1, 'aligned', None),
    (17, 3076, 1284, ('ig_32x128', 14, 'finish_few_vec'), 1, 'aligned', None),
    (17, 4101, 1028, ('ig_32x128', 11, 'finish_few'), 1, 'aligned', None),
    (17, 6148, 36, ('ig_32x128',) + NO, 3, 'aligned', None),
    (17, 500, 16388, ('ig_32x128', 103, 'finish'), 1, 'aligned', None),          # 4 narrow tiles: past the split cap of 64
    (20, 644, 16388, ('ig_32x128', 57, 'finish'), 1, 'aligned', None),           # 5: capped at 64 ranges of 288
    # igemm large layouts, scalar loaders: K % 4, a misaligned pointer, a leading dimension % 4
    (68, 68, 50, ('ig_64x64_s',) + NO, 1, 'aligned', None),
    (68, 70, 70, ('ig_64x64_s', 2, 'finish_few'), 1, 'aligned', None),
    (68, 68, 1030, ('ig_64x64_k4_s', 17, 'finish'), 1, 'aligned', None),
    (68, 68, 133, ('ig_64x64_k4_s', 3, 'finish_few_vec'), 1, 'aligned', None),
    (68, 68, 132, ('ig_64x64_k4_s', 3, 'finish_few_vec'), 1, 'offset', None),
    (68, 68, 132, ('ig_64x64_k4_s', 3, 'finish_few_vec'), 1, 'ldx', None),
    (68, 2052, 133, ('ig_64x64_k2_s', 3, 'finish_few_vec'), 1, 'aligned', None),
    (17, 132, 50, ('ig_32x128_s',) + NO, 1, 'aligned', None),
    (17, 133, 70, ('ig_32x128_s', 2, 'finish_few'), 1, 'aligned', None),
    (68, 2052, 4101, ('ig_64x128_s', 15, 'finish_few_vec'), 1, 'aligned', None),
]


@pytest.mark.parametrize('M,N,Kd,route,G,how,note', FWD_CASES,
                         ids=['%s-%dx%dx%d-G%d-%s' % (c[3][0], c[0], c[1], c[2], c[4], c[5]) for c in FWD_CASES])
def test_forward(M, N, Kd, route, G, how, note):
    tm, tn = (int(v) for v in route[0].split('_')[1].split('x'))
    if note == G2S_ON:
        assert ((M + tm - 1) // tm) % 8 == 0
    elif route[0].startswith('g2s_'):
        assert ((M + tm - 1) // tm) % 8 != 0
    elif G == 1 and route[1] == 1:
        assert (((N + tn - 1) // tn) % 2 == 0 and ((M + tm - 1) // tm) % 4 == 0) == (note == XCD_ON)
    run_fwd(M, N, Kd, route, G, how)


def test_forward_gemm2_both_hints():
    """One 64 x 64 tile per block (1544 tiles): pre + act over K <= 640 and act alone over K <= 128 take gemm2_kernel, pre
    alone and act under a dropout mask stay on igemm_kernel -- the same shape on two kernels, pre of both to the bound."""
    ig = ('ig_64x64',) + NO
    run_fwd(452, 12292, 20, ('gemm2',) + NO, 1, 'aligned', alt={'pre': ig, 'act*mask': ig, 'pre nobias': ig})
    # past K = 128 only the two-output form is left on it
    run_fwd(452, 12292, 132, ('gemm2',) + NO, 1, 'aligned', alt={'pre': ig, 'act': ig, 'act*mask': ig, 'pre nobias': ig})


def test_forward_gemm2_grouped():
    """Groups count as tiles (3 x 4 x 129 = 1548); group 2's parameters sit behind NaN padding."""
    ig = ('ig_64x64',) + NO
    run_fwd(196, 8196, 20, ('gemm2',) + NO, 3, 'aligned', alt={'pre': ig})


# ----------------------------------------------------------------------------- data gradient
def run_dgrad(M, N, Kd, route, G=1, how='aligned'):
    lddy = N + {'lddy': 2, 'slice': 8}.get(how, 0)
    route_is('dgrad', M, N, Kd, route, G, aligned=how != 'offset', ld_a=lddy,
             **({'gs_a': M * lddy, 'gs_b': (N * Kd + 40 + 3) // 4 * 4} if G > 1 else {}))
    gd = Guarded()
    sc = N ** -0.5
    if G == 1:
        dy, w = g64(M, N, seed=21), g64(N, Kd, seed=22, scale=sc)
        ref = dy @ w
        if how == 'offset':
            dyd = gd.inp(torch.cat([torch.zeros(3, dtype=torch.float64), dy.reshape(-1)]), 'dy')[3:].view(M, N)
        elif how in ('lddy', 'slice'):
            p = torch.full((M, lddy), NAN, dtype=torch.float64)
            c0 = 4 if how == 'slice' else 0
            p[:, c0:c0 + N] = dy
            dyd = gd.inp(p, 'dy')[:, c0:c0 + N]
        else:
            dyd = gd.inp(dy, 'dy')
        wd = gd.inp(w, 'w')
        shape = (M, Kd)
    else:
        assert how == 'aligned'
        dy = g64(G, M, N, seed=21)
        w, wflat, w_gs, _ = params(G, (N, Kd), 40, 22, sc)
        ref = torch.einsum('gmn,gnk->gmk', dy, w)
        dyd = gd.inp(dy, 'dy')
        wd = gd.inp(wflat, 'w')[:N * Kd].view(N, Kd)
        shape = (G, M, Kd)
    pre_in, base = g64(*shape, seed=23), g64(*shape, seed=24)
    pd = gd.inp(pre_in, 'pre_in')
    mask = keep_mask(shape, 25) if G == 1 else None
    md = gd.inp(mask, 'mask') if G == 1 else None

    def launch(form):
        dx = gd.out(shape, 'dx', init=base if form == 'accumulate' else None)
        if G > 1:
            K.linear_dgrad_grouped(dyd, wd, w_gs, dx, pd if form == 'pre_in' else None, accumulate=form == 'accumulate')
        else:
            K.linear_dgrad(dyd, wd, dx, pd if form in ('pre_in', 'pre_in*mask') else None,
                           md if form == 'pre_in*mask' else None, 1 / 0.9 if form == 'pre_in*mask' else 1.0,
                           accumulate=form == 'accumulate')
        return dx
    forms = ('plain', 'pre_in', 'accumulate') + (('pre_in*mask',) if G == 1 else ())
    runs = {f: (launch(f), launch(f)) for f in forms}
    gd.check()
    want = {'plain': ref, 'pre_in': ref * swish_grad(pre_in), 'accumulate': base + ref}
    if G == 1:
        want['pre_in*mask'] = ref * swish_grad(pre_in) * (mask / 0.9)
    for f, (a, b) in runs.items():
        close(route[0], a, want[f], 'dgrad [%s]' % f)
        same_bits(a, b, 'dgrad [%s]' % f)


DGRAD_CASES = [
    (37, 16, 300, ('dgrad_smalln',) + NO, 1, 'aligned', None),
    (300, 1, 516, ('dgrad_smalln',) + NO, 1, 'aligned', None),
    (70, 10, 259, ('dgrad_smalln',) + NO, 3, 'aligned', None),
    # gemm2s: six instantiations, Q_RK = false
    (36, 68, 36, ('g2s_32x32_k8',) + NO, 1, 'aligned', None),
    (228, 68, 36, ('g2s_32x32_k8',) + NO, 1, 'slice', G2S_ON),
    (36, 68, 5124, ('g2s_32x32_k4',) + NO, 1, 'aligned', None),
    (68, 68, 4100, ('g2s_32x64_k4',) + NO, 1, 'aligned', None),
    (4100, 68, 68, ('g2s_64x32_k4',) + NO, 1, 'aligned', None),
    (4036, 68, 68, ('g2s_64x32_k4',) + NO, 1, 'aligned', G2S_ON),
    (68, 68, 2564, ('g2s_32x64_k2',) + NO, 3, 'aligned', None),
    (2564, 68, 68, ('g2s_64x32_k2',) + NO, 3, 'aligned', None),
    (1284, 132, 68, ('g2s_64x32_k4',) + NO, 3, 'aligned', None),
    # igemm large layouts, float4 loaders
    (68, 36, 8196, ('ig_64x64',) + NO, 1, 'aligned', None),
    (196, 36, 4036, ('ig_64x64',) + NO, 1, 'aligned', XCD_ON),
    (68, 68, 8196, ('ig_64x64', 2, 'finish_few_vec'), 1, 'aligned', None),
    (68, 1028, 68, ('ig_64x64_k4', 17, 'finish'), 1, 'slice', None),
    (68, 1028, 452, ('ig_64x64_k4', 11, 'finish_few_vec'), 1, 'aligned', None),
    (68, 1028, 644, ('ig_64x64_k2', 4, 'finish_few_vec'), 3, 'aligned', None),
    (68, 4100, 2052, ('ig_64x128', 15, 'finish_few_vec'), 1, 'aligned', None),
    (17, 1028, 132, ('ig_32x128', 17, 'finish'), 1, 'aligned', None),
    (17, 1284, 3076, ('ig_32x128', 14, 'finish_few_vec'), 1, 'aligned', None),
    # scalar loaders: N % 4, K % 4, a misaligned pointer, a leading dimension % 4
    (68, 36, 70, ('ig_64x64_s',) + NO, 1, 'aligned', None),
    (68, 68, 70, ('ig_64x64_s', 2, 'finish_few'), 1, 'aligned', None),
    (68, 1030, 68, ('ig_64x64_k4_s', 17, 'finish'), 1, 'aligned', None),
    (68, 132, 70, ('ig_64x64_k4_s', 3, 'finish_few'), 1, 'aligned', None),
    (68, 132, 68, ('ig_64x64_k4_s', 3, 'finish_few_vec'), 1, 'offset', None),
    (68, 132, 68, ('ig_64x64_k4_s', 3, 'finish_few_vec'), 1, 'lddy', None),
    (2052, 132, 70, ('ig_64x64_k2_s', 3, 'finish_few'), 1, 'aligned', None),
    (17, 36, 133, ('ig_32x128_s',) + NO, 1, 'aligned', None),
    (17, 68, 133, ('ig_32x128_s', 2, 'finish_few'), 1, 'aligned', None),
    (68, 4101, 2052, ('ig_64x128_s', 15, 'finish_few_vec'), 1, 'aligned', None),
    (768, 18, 516, ('ig_64x64_s',) + NO, 1, 'aligned', None),                    # celeba's attribute head
]


@pytest.mark.parametrize('M,N,Kd,route,G,how,note', DGRAD_CASES,
                         ids=['%s-%dx%dx%d-G%d-%s' % (c[3][0], c[0], c[1], c[2], c[4], c[5]) for c in DGRAD_CASES])
def test_data_gradient(M, N, Kd, route, G, how, note):
    if route[0] != 'dgrad_smalln':
        tm, tn = (int(v) for v in route[0].split('_')[1].split('x'))
        if note == G2S_ON:
            assert ((M + tm - 1) // tm) % 8 == 0
        elif route[0].startswith('g2s_'):
            assert ((M + tm - 1) // tm) % 8 != 0
        elif G == 1 and route[1] == 1:
            assert (((Kd + tn - 1) // tn) % 2 == 0 and ((M + tm - 1) // tm) % 4 == 0) == (note == XCD_ON)
    run_dgrad(M, N, Kd, route, G, how)


# ----------------------------------------------------------------------------- weight gradient
def run_wgrad(M, N, Kd, route, route_nodb=None, G=1, how='aligned'):
    """``route``: with a bias gradient; ``route_nodb``: without one where that differs (the row sums sit behind every partial:
    the finish launch follows stride % 4)."""
    route_nodb = route_nodb or route
    ldx = Kd + (2 if how == 'ldx' else 0)
    for db, want in ((True, route), (False, route_nodb)):
        route_is('wgrad', M, N, Kd, want, G, db=db, aligned=how != 'offset', ld_b=ldx, **({'gs_b': M * ldx} if G > 1 else {}))
    gd = Guarded()
    lead = (G,) if G > 1 else ()
    dy, x = g64(*lead, M, N, seed=31), g64(*lead, M, Kd, seed=32)
    if G > 1:
        dw_ref, db_ref = torch.einsum('gmn,gmk->gnk', dy, x), dy.sum(1)
    else:
        dw_ref, db_ref = dy.t() @ x, dy.sum(0)
    if how == 'offset':
        dyd = gd.inp(torch.cat([torch.zeros(3, dtype=torch.float64), dy.reshape(-1)]), 'dy')[3:].view(M, N)
        xd = gd.inp(x, 'x')
    elif how == 'ldx':
        p = torch.full((M, ldx), NAN, dtype=torch.float64)
        p[:, :Kd] = x
        dyd, xd = gd.inp(dy, 'dy'), gd.inp(p, 'x')[:, :Kd]
    else:
        dyd, xd = gd.inp(dy, 'dy'), gd.inp(x, 'x')
    n = N * Kd
    dw_gs, db_gs = (n + 40 + 3) // 4 * 4, (N + 8 + 3) // 4 * 4          # the groups' gradients with padding between them
    dw_base, db_base = g64(*lead, N, Kd, seed=33), g64(*lead, N, seed=34)

    def launch(form):
        acc = form == 'accumulate'
        if G == 1:
            dw = gd.out((N, Kd), 'dw', init=dw_base if acc else None)
            db = gd.out((N,), 'db', init=db_base if acc else None) if form != 'dw' else None
            K.linear_wgrad(dyd, xd, dw, db, accumulate=acc)
            return dw, db, None, None
        dwf = gd.out((G * dw_gs,), 'dw')
        dbf = gd.out((G * db_gs,), 'db') if form != 'dw' else None
        dws = [dwf[i * dw_gs:i * dw_gs + n].view(N, Kd) for i in range(G)]
        dbs = [dbf[i * db_gs:i * db_gs + N] for i in range(G)] if dbf is not None else None
        if acc:
            for i in range(G):
                dws[i].copy_(dw_base[i].to(torch.float32)); dbs[i].copy_(db_base[i].to(torch.float32))
        K.linear_wgrad_grouped(dyd, xd, dws[0], dw_gs, dbs[0] if dbs else None, db_gs if dbs else 0, accumulate=acc)
        # the padding between the groups' gradients stays NaN
        for i in range(G):
            assert torch.isnan(dwf[i * dw_gs + n:(i + 1) * dw_gs]).all(), 'padding behind dw of group %d written' % i
            if dbf is not None:
                assert torch.isnan(dbf[i * db_gs + N:(i + 1) * db_gs]).all(), 'padding behind db of group %d written' % i
        return torch.stack(dws), torch.stack(dbs) if dbs else None, dwf, dbf
    runs = {f: (launch(f), launch(f)) for f in ('dw', 'dw+db', 'accumulate')}
    gd.check()
    for f, (a, b) in runs.items():
        name = (route_nodb if f == 'dw' else route)[0]
        close(name, a[0], dw_ref + (dw_base if f == 'accumulate' else 0), 'wgrad [%s] dw' % f)
        same_bits(a[0], b[0], 'wgrad [%s] dw' % f)
        if a[1] is not None:
            close(name, a[1], db_ref + (db_base if f == 'accumulate' else 0), 'wgrad [%s] db' % f)
            same_bits(a[1], b[1], 'wgrad [%s] db' % f)


FEW, VEC = 'finish_few', 'finish_few_vec'
WGRAD_CASES = [
    # wgrad_direct_kernel: 20 / 105 / 225 tiles of 32 x 32; it takes operands float4 loads cannot
    (300, 100, 132, ('wgrad_direct_16',) + NO, None, 1, 'aligned'),
    (77, 129, 131, ('wgrad_direct_16',) + NO, None, 1, 'offset'),
    (300, 132, 644, ('wgrad_direct_8',) + NO, None, 1, 'aligned'),
    (200, 260, 772, ('wgrad_direct_4',) + NO, None, 1, 'aligned'),
    (515, 200, 516, ('wgrad_direct_8',) + NO, None, 1, 'ldx'),                   # celeba's 512 x 200 x 512, ragged
    # igemm small layouts (EpRowMajor with and without ROWSUM)
    (68, 36, 36, ('igs_32x32_k8',) + NO, None, 1, 'aligned'),
    (68, 36, 2052, ('igs_32x32_k4',) + NO, None, 3, 'aligned'),
    (68, 68, 1284, ('igs_32x64_k4',) + NO, None, 3, 'aligned'),
    (68, 1284, 68, ('igs_64x32_k4',) + NO, None, 3, 'aligned'),
    (68, 68, 2564, ('igs_32x64_k2',) + NO, None, 3, 'aligned'),
    (68, 2564, 68, ('igs_64x32_k2',) + NO, None, 3, 'aligned'),
    # igemm large layouts, float4 loaders; the bias gradient's row sums carried through each finish launch
    (36, 228, 8196, ('ig_64x64',) + NO, None, 1, 'aligned'),                     # 2056 tiles of 32 x 32
    (8196, 68, 68, ('ig_64x64', 29, 'finish'), None, 1, 'aligned'),              # more than 4096 rows
    (4100, 68, 196, ('ig_64x64', 15, VEC), None, 1, 'aligned'),
    (3076, 68, 68, ('ig_64x64', 11, VEC), None, 3, 'aligned'),
    (1028, 68, 68, ('ig_64x64_k4', 17, 'finish'), None, 1, 'aligned'),
    (1028, 68, 132, ('ig_64x64_k4', 11, VEC), None, 3, 'aligned'),
    (1028, 20, 132, ('ig_32x128', 17, 'finish'), None, 1, 'aligned'),
    (4100, 20, 900, ('ig_32x128', 15, VEC), None, 1, 'aligned'),
    # scalar loaders
    (36, 70, 68, ('ig_64x64_s',) + NO, None, 1, 'aligned'),
    (68, 70, 68, ('ig_64x64_s', 2, FEW), ('ig_64x64_s', 2, VEC), 1, 'aligned'),
    (8196, 70, 68, ('ig_64x64_s', 29, 'finish'), None, 1, 'aligned'),
    (1028, 70, 68, ('ig_64x64_k4_s', 17, 'finish'), None, 1, 'aligned'),
    (132, 70, 68, ('ig_64x64_k4_s', 3, FEW), ('ig_64x64_k4_s', 3, VEC), 1, 'aligned'),
    (132, 68, 70, ('ig_64x64_k4_s', 3, FEW), None, 1, 'aligned'),
    (132, 1540, 5, ('ig_64x64_k2_s', 3, FEW), None, 3, 'aligned'),
    (36, 17, 132, ('ig_32x128_s',) + NO, None, 1, 'aligned'),
    (68, 17, 132, ('ig_32x128_s', 2, FEW), ('ig_32x128_s', 2, VEC), 1, 'aligned'),
    (1028, 17, 132, ('ig_32x128_s', 17, 'finish'), None, 1, 'aligned'),
    (768, 1, 516, ('ig_32x128_s', 12, FEW), ('ig_32x128_s', 12, VEC), 3, 'aligned'),       # celeba19's one-logit heads
]


@pytest.mark.parametrize('M,N,Kd,route,route_nodb,G,how', WGRAD_CASES,
                         ids=['%s-%dx%dx%d-G%d-%s' % (c[3][0], c[0], c[1], c[2], c[5], c[6]) for c in WGRAD_CASES])
def test_weight_gradient(M, N, Kd, route, route_nodb, G, how):
    run_wgrad(M, N, Kd, route, route_nodb, G, how)


# ----------------------------------------------------------------------------- fused losses
def run_bce(M, N, Kd, route, groups, how='aligned'):
    route_is('bce_fwd', M, N, Kd, route, aligned=how != 'offset')
    rpg = M // groups
    assert rpg * groups == M and groups > 1                       # rows per group smaller than M
    x = g64(M, Kd, seed=41)
    w, b = g64(N, Kd, seed=42, scale=Kd ** -0.5).requires_grad_(), g64(N, seed=43, scale=0.1)
    t = torch.rand(rpg, N, generator=torch.Generator().manual_seed(44), dtype=torch.float64)
    drow = torch.tensor([0.5, 0.0, 2.0, 1.25][:groups], dtype=torch.float64)
    logits = x @ w.t() + b
    logits.retain_grad()
    rows = OF.binary_cross_entropy_with_logits(logits, t.repeat(groups, 1)).sum(1)
    (rows * drow.repeat_interleave(rpg)).sum().backward()
    gd = Guarded()
    if how == 'offset':
        xd = gd.inp(torch.cat([torch.zeros(3, dtype=torch.float64), x.reshape(-1)]), 'x')[3:].view(M, Kd)
    else:
        xd = gd.inp(x, 'x')
    wd, bd, td, dd = gd.inp(w.detach(), 'w'), gd.inp(b, 'b'), gd.inp(t, 't'), gd.inp(drow, 'drow')
    nparts = K.bce_partials(N)
    outs = []
    for _ in range(2):
        dl, lg, part = gd.out((M, N), 'dlogits'), gd.out((M, N), 'logits'), gd.out((M * nparts,), 'partial')
        K.linear_bce_fwd(xd, wd, bd, td, dd, dl, part, rpg, rpg, logits=lg)
        outs.append((dl, lg, part))
    gd.check()
    dl, lg, part = outs[0]
    for t_, what in zip(outs[0], ('dlogits', 'logits', 'partial')):
        assert not torch.isnan(t_).any().item(), 'bce %s: NaN left' % what
    e1 = assert_close(lg, logits.detach().to(torch.float32), 'bce logits', tol=1e-5)
    e2 = assert_close(part.view(M, nparts).sum(1), rows.detach().to(torch.float32), 'bce rows', tol=1e-5)
    print('ROUTE-ERR %-16s %-40s %.3e (bound 1e-05)' % (route[0], 'bce logits', e1))
    print('ROUTE-ERR %-16s %-40s %.3e (bound 1e-05)' % (route[0], 'bce rows', e2))
    close(route[0], dl, logits.grad, 'bce d loss / d logits')
    for a, b_, what in zip(outs[0], outs[1], ('dlogits', 'logits', 'partial')):
        same_bits(a, b_, 'bce %s' % what)


BCE_CASES = [
    (72, 36, 68, ('igs_32x32_k8',) + NO, 2, 'aligned'),
    (36, 5124, 68, ('igs_32x32_k4',) + NO, 3, 'aligned'),
    (68, 4100, 68, ('igs_32x64_k4',) + NO, 2, 'aligned'),
    (4100, 68, 68, ('igs_64x32_k4',) + NO, 4, 'aligned'),
    (5124, 100, 68, ('igs_32x64_k2',) + NO, 3, 'aligned'),
    (100, 5124, 68, ('igs_64x32_k2',) + NO, 2, 'aligned'),
    (1024, 784, 516, ('igs_64x32_k2',) + NO, 2, 'aligned'),                      # MNIST's image decoder head, K ragged
    (68, 8196, 36, ('ig_64x64',) + NO, 2, 'aligned'),
    (68, 68, 1028, ('ig_64x64_k4',) + NO, 2, 'aligned'),
    (18, 132, 1028, ('ig_32x128',) + NO, 2, 'aligned'),
    (68, 68, 50, ('ig_64x64_s',) + NO, 2, 'aligned'),
    (68, 68, 133, ('ig_64x64_k4_s',) + NO, 2, 'aligned'),
    (768, 18, 516, ('ig_64x64_k4_s',) + NO, 3, 'offset'),                        # celeba's attribute head on a misaligned x
    (68, 2052, 133, ('ig_64x64_k2_s',) + NO, 2, 'aligned'),
]


@pytest.mark.parametrize('M,N,Kd,route,groups,how', BCE_CASES,
                         ids=['%s-%dx%dx%d-%s' % (c[3][0], c[0], c[1], c[2], c[5]) for c in BCE_CASES])
def test_linear_with_bernoulli_term(M, N, Kd, route, groups, how):
    run_bce(M, N, Kd, route, groups, how)


CE_CASES = [
    (72, 10, 68, ('igs_32x32_k8',) + NO, 2),
    (8196, 10, 68, ('igs_64x32_k4',) + NO, 3),           # one column tile: past 224 blocks the tall layout, never 32 x 32 / 4
    (4100, 32, 132, ('igs_32x32_k8',) + NO, 2),                                  # a full 32-class tile
    (68, 20, 1028, ('ig_64x64_k4',) + NO, 2),
    (68, 10, 50, ('ig_64x64_s',) + NO, 2),
    (68, 10, 133, ('ig_64x64_k4_s',) + NO, 2),
]


@pytest.mark.parametrize('M,N,Kd,route,groups', CE_CASES, ids=['%s-%dx%dx%d' % (c[3][0], c[0], c[1], c[2]) for c in CE_CASES])
def test_linear_with_categorical_term(M, N, Kd, route, groups):
    route_is('ce_fwd', M, N, Kd, route)
    rpg = M // groups
    assert rpg * groups == M
    x = g64(M, Kd, seed=51)
    w, b = g64(N, Kd, seed=52, scale=3 * Kd ** -0.5).requires_grad_(), g64(N, seed=53, scale=0.1)
    y = torch.randint(0, N, (rpg,), generator=torch.Generator().manual_seed(54))
    drow = torch.tensor([0.7, 1.3, 0.0][:groups], dtype=torch.float64)
    logits = x @ w.t() + b
    logits.retain_grad()
    rows = OF.cross_entropy(logits, y.repeat(groups)).sum(1)
    (rows * drow.repeat_interleave(rpg)).sum().backward()
    gd = Guarded()
    xd, wd, bd, dd = gd.inp(x, 'x'), gd.inp(w.detach(), 'w'), gd.inp(b, 'b'), gd.inp(drow, 'drow')
    yd = y.to(DEV)
    outs = []
    for _ in range(2):
        dl, lg, rw = gd.out((M, N), 'dlogits'), gd.out((M, N), 'logits'), gd.out((M,), 'rows')
        K.linear_ce_fwd(xd, wd, bd, yd, dd, dl, rw, rpg, rpg, logits=lg)
        outs.append((dl, lg, rw))
    gd.check()
    assert torch.equal(yd.cpu(), y)
    dl, lg, rw = outs[0]
    for t_, what in zip(outs[0], ('dlogits', 'logits', 'rows')):
        assert not torch.isnan(t_).any().item(), 'ce %s: NaN left' % what
    e1 = assert_close(lg, logits.detach().to(torch.float32), 'ce logits', tol=1e-5)
    e2 = assert_close(rw, rows.detach().to(torch.float32), 'ce rows', tol=1e-5)
    print('ROUTE-ERR %-16s %-40s %.3e (bound 1e-05)' % (route[0], 'ce logits', e1))
    print('ROUTE-ERR %-16s %-40s %.3e (bound 1e-05)' % (route[0], 'ce rows', e2))
    close(route[0], dl, logits.grad, 'ce d loss / d logits')
    for a, b_, what in zip(outs[0], outs[1], ('dlogits', 'logits', 'rows')):
        same_bits(a, b_, 'ce %s' % what)


def test_xcd_map_on_under_the_row_sum_and_the_fused_loss_epilogues():
    """igemm_kernel's launch-order re-map (one group, no split, grid.x % 2 == 0 and grid.y % 4 == 0) under ROWSUM and
    EpRowBce, on a small and on a large layout; tests/test_forward and test_data_gradient have it under EpRowMajor.  The
    categorical term has one column tile (grid.x = 1): the re-map is never on for it."""
    def on(rows, cols, tm, tn):
        return ((cols + tn - 1) // tn) % 2 == 0 and ((rows + tm - 1) // tm) % 4 == 0
    assert on(100, 36, 32, 32) and on(196, 9412, 64, 64) and on(196, 8132, 64, 64)
    run_wgrad(68, 100, 36, ('igs_32x32_k8',) + NO)                      # grid 2 x 4
    run_wgrad(36, 196, 9412, ('ig_64x64',) + NO)                        # grid 148 x 4; 2065 tiles of 32 x 32: past wgrad_direct_ok
    run_bce(100, 36, 68, ('igs_32x32_k8',) + NO, 2)
    run_bce(196, 8132, 36, ('ig_64x64',) + NO, 2)                       # grid 128 x 4


# ----------------------------------------------------------------------------- batched weight gradient
def run_batch(shapes, want, strided=None):
    """Mixed items: db absent on every third, accumulation on every second; ``strided``: (item, ldx) -- that item's x is a
    column slice of a wide parent."""
    gd = Guarded()
    items, refs = [], []
    for q, (M, N, Kd) in enumerate(shapes):
        dy, x = g64(M, N, seed=100 + q), g64(M, Kd, seed=200 + q)
        dyd = gd.inp(dy, 'dy%d' % q)
        if strided and strided[0] == q:
            parent = torch.zeros(M, strided[1], dtype=torch.float64)
            parent[:, :Kd] = x
            xd = gd.inp(parent, 'x%d' % q)[:, :Kd]
        else:
            xd = gd.inp(x, 'x%d' % q)
        items.append((dyd, xd, q % 3 != 2, q % 2 == 1))
        refs.append((dy.t() @ x, dy.sum(0)))
    dw_base = [g64(N, Kd, seed=300 + q) for q, (M, N, Kd) in enumerate(shapes)]
    db_base = [g64(N, seed=400 + q) for q, (M, N, Kd) in enumerate(shapes)]

    def launch():
        batch = []
        for q, ((dyd, xd, with_db, acc), (M, N, Kd)) in enumerate(zip(items, shapes)):
            dw = gd.out((N, Kd), 'dw%d' % q, init=dw_base[q] if acc else None)
            db = gd.out((N,), 'db%d' % q, init=db_base[q] if acc else None) if with_db else None
            batch.append((dyd, xd, dw, db, acc))
        assert K.linear_wgrad_batched_route(batch) == want, (K.linear_wgrad_batched_route(batch), want)
        assert all(K.wgrad_batchable(it[0], it[1]) for it in batch)
        K.linear_wgrad_batched(batch)
        return batch
    a, b = launch(), launch()
    gd.check()
    name = '%s %dx%d/%d' % ((want[0],) + want[1] + (want[2],))
    for q, (ia, ib) in enumerate(zip(a, b)):
        acc = ia[4]
        close(name, ia[2], refs[q][0] + (dw_base[q] if acc else 0), 'batched dw of item %d' % q)
        same_bits(ia[2], ib[2], 'batched dw of item %d' % q)
        if ia[3] is not None:
            close(name, ia[3], refs[q][1] + (db_base[q] if acc else 0), 'batched db of item %d' % q)
            same_bits(ia[3], ib[3], 'batched db of item %d' % q)


WB2 = 'wgrad_batched2'
BATCHES = [
    ([(516, 20, 20)], (WB2, (32, 32), 16)),
    ([(520, 388, 36), (516, 36, 2052), (777, 20, 132)], (WB2, (32, 32), 8)),
    ([(140, 2052, 36), (136, 36, 516), (136, 772, 36), (140, 44, 388), (140, 68, 1540), (136, 132, 388)], (WB2, (32, 32), 4)),
    ([(520, 1540, 36), (516, 36, 644), (516, 36, 1028), (520, 516, 36), (1032, 20, 100), (516, 44, 324)], (WB2, (64, 32), 16)),
    ([(516, 132, 36), (516, 2052, 36), (516, 68, 1028), (516, 20, 772)], (WB2, (64, 32), 8)),
    ([(136, 68, 1028), (136, 516, 196), (140, 324, 1028), (137, 20, 2052), (136, 132, 516), (140, 324, 260)], (WB2, (64, 32), 4)),
    ([(137, 44, 260), (136, 516, 2052), (136, 388, 900), (140, 516, 644), (136, 324, 100), (140, 100, 196)], (WB2, (64, 32), 2)),
    ([(20, 324, 196), (40, 44, 44), (20, 1540, 36), (20, 36, 1284)], (WB2, (64, 32), 2)),        # halved for rows: max M < 128
    ([(260, 388, 20), (264, 260, 644), (260, 1540, 36), (264, 260, 516), (260, 100, 1540), (264, 36, 2052)], (WB2, (64, 64), 8)),
    ([(136, 260, 2052), (136, 516, 644), (136, 644, 388), (136, 772, 516), (140, 1284, 68), (136, 324, 68)], (WB2, (64, 64), 4)),
]


@pytest.mark.parametrize('shapes,want', BATCHES, ids=['%dx%d-%dwaves-%ditems' % (w[1] + (w[2], len(s))) for s, w in BATCHES])
def test_batched_weight_gradient(shapes, want):
    run_batch(shapes, want)


def test_batched_weight_gradient_on_a_wide_parent_takes_the_older_kernel():
    """x is 40 columns of a [8, 530000] parent (17 MB): (M + 1024) x ld x 4 is past 2^31, where wgrad_batched2_kernel's signed
    byte offsets could wrap -- the batch runs on wgrad_batched_kernel."""
    run_batch([(8, 36, 40), (8, 20, 68)], ('wgrad_batched', (32, 32), 16), strided=(0, 530000))


@pytest.mark.parametrize('shapes,waves', [
    ([(136, 516, 1540), (140, 36, 68)], 4),            # 17 x 49 + 2 x 3 = 839 tiles of 32 x 32
    ([(260, 260, 1028), (264, 36, 68)], 8),            # 9 x 33 + 6 = 303
    ([(516, 68, 132), (520, 36, 68)], 16),             # 15 + 6 = 21
])
def test_batched_adam_is_wgrad_then_adam(shapes, waves):
    """wgrad_batched_adam_kernel at 4, 8 and 16 waves per tile (from 768 and 256 tiles), the way
    tests/test_kernels_gpu.py::test_linear_wgrad_batched_adam_is_wgrad_then_adam checks it: parameters and both moments bit
    for bit equal to the plain 32 x 32 arithmetic followed by mvae_adam_apply_at on the gradients the fused launch produced,
    those gradients to REL_TOL of float64, and an update-only item."""
    sizes = []
    for (M, N, Kd) in shapes:
        sizes += [N * Kd, N]
    extra = 1024 + 3
    offs, off = [], 0
    for n in sizes + [extra]:
        offs.append(off); off += (n + 3) // 4 * 4
    total = off
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8

    def arenas():
        return (g64(total, seed=900, scale=0.1).float().to(DEV), torch.zeros(total, device=DEV),
                g64(total, seed=901, scale=0.01).float().to(DEV), g64(total, seed=902, scale=0.01).abs().float().to(DEV))
    ins = [(g64(M, N, seed=100 + q), g64(M, Kd, seed=200 + q)) for q, (M, N, Kd) in enumerate(shapes)]
    results = []
    for fused in (True, False, True):
        param, grad, m, v = arenas()
        step = torch.full((1,), 6, dtype=torch.int64, device=DEV)
        coef = torch.zeros(2, device=DEV)
        o_extra = offs[-1]
        grad[o_extra:o_extra + extra] = g64(extra, seed=77).float().to(DEV)
        items = []
        for q, (M, N, Kd) in enumerate(shapes):
            ow, ob = offs[2 * q], offs[2 * q + 1]
            items.append((ins[q][0].float().to(DEV), ins[q][1].float().to(DEV), grad[ow:ow + N * Kd].view(N, Kd),
                          grad[ob:ob + N] if q == 0 else None, False))
        K.adam_prepare(step, 1, lr, b1, b2, coef)
        if fused:
            st = _lib.AdamFuse(grad.data_ptr(), param.data_ptr(), m.data_ptr(), v.data_ptr(), coef.data_ptr(), b1, b2, eps, 1.0)
            batch = items + [(None, None, grad[o_extra:o_extra + extra], None, False)]
            assert K.linear_wgrad_batched_route(batch, adam=True) == ('wgrad_batched_adam', (32, 32), waves)
            K.linear_wgrad_batched(batch, adam=st)
        else:
            grad.copy_(results[0][1])           # Adam on exactly the gradients the fused launch produced
            for lo, n in zip(offs, sizes + [extra]):
                if n == shapes[1][1] and lo == offs[3]:
                    continue                    # item 1 has no bias gradient: its parameters take no update
                hi = lo + n
                K.adam_apply_at(param[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], step, 0, lr, b1, b2, eps)
        torch.cuda.synchronize()
        results.append((param.clone(), grad.clone(), m.clone(), v.clone()))
    for a, b, c, what in zip(results[0], results[1], results[2], ('param', 'grad', 'exp_avg', 'exp_avg_sq')):
        assert torch.equal(a, b), '%s: fused launch != batch then Adam' % what
        assert torch.equal(a, c), '%s: two runs of the fused launch differ' % what
    for q, (M, N, Kd) in enumerate(shapes):
        got = results[0][1]
        e = assert_close(got[offs[2 * q]:offs[2 * q] + N * Kd].view(N, Kd), (ins[q][0].t() @ ins[q][1]).float(), 'adam-fused dw %d' % q)
        print('ROUTE-ERR %-16s %-40s %.3e (bound %.0e)' % ('wb_adam/%d' % waves, 'dw of item %d' % q, e, REL_TOL))
    assert_close(results[0][1][offs[1]:offs[1] + shapes[0][1]], ins[0][0].sum(0).float(), 'adam-fused db 0')
    p0 = arenas()[0]
    ob, N1 = offs[3], shapes[1][1]
    assert torch.equal(results[0][0][ob:ob + N1], p0[ob:ob + N1]), 'parameters behind an absent bias gradient moved'
    assert not torch.equal(results[0][0][offs[-1]:offs[-1] + extra], p0[offs[-1]:offs[-1] + extra]), 'update-only item not applied'
