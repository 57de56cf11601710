"""GPU: every kernel the training-mode BatchNorm launches choose between (csrc/norm.hip), in both directions where the
route exists, at the cheapest shape that still reaches the route's tails.  Every case

  * first asserts, through the host-only query ``kernels.bn_route`` (the route function the launch itself switches on),
    which kernel it is on -- a threshold that moves fails the case instead of quietly testing other code;
  * allocates every output full of NaN, so a region a launch skips shows;
  * is judged against a float64 reference written in plain torch below (``reference``): per group the mean, the biased
    variance, y, Swish, dx / dgamma / dbeta by the closed form, and the running statistics with the unbiased factor,
    advanced ``n_updates`` times per group in group order.

Error measure: y and dx per (group, channel) slice -- max |err| over the slice / max |ref| over the same slice, so one wrong
channel of 512 or one wrong group cannot hide behind the tensor's largest value; dgamma, dbeta, save_mean, save_invstd and
the running statistics elementwise against max |ref| of the tensor.  Bounds: util.REL_TOL = 1e-4, 1e-5 for the running
statistics.

tests/test_bn_routes_cpu.py pins the gates themselves and the launches' host-side refusals (nothing here passes an
invalid argument).
"""
import pytest
import torch
import torch.nn.functional as F

import mvae_amd
from mvae_amd import _lib
from mvae_amd import kernels as K
from util import REL_TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RUN_TOL = 1e-5
EPS, MOMENTUM = 1e-5, 0.1


def nans(*shape):
    """An output tensor no kernel has written: a region a launch skips shows as NaN (torch.empty can hand back the
    previous call's correct result)."""
    return torch.full(shape, float('nan'), device=DEV)


def shifted(t):
    """The same values one float into a larger buffer: contiguous, but not 16-byte aligned."""
    buf = torch.full((t.numel() + 1,), float('nan'), device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def hw_of(spatial):
    n = 1
    for d in spatial:
        n *= d
    return n


def swish(x):
    return x * torch.sigmoid(x)


def swish_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def inputs(G, B, C, spatial, seed=0, mean_over_std=None):
    """x [G*B, C, *spatial] with its own scale and offset per (group, channel) -- a kernel that mixes two channels or two
    groups up gets both wrong --, gamma, beta, dy and non-trivial running statistics.  ``mean_over_std``: [C] ratios of a
    channel's mean to its standard deviation (the far-from-zero cases)."""
    gen = torch.Generator(device=DEV).manual_seed(1000 + seed)

    def rn(*shape):
        return torch.randn(*shape, generator=gen, device=DEV)

    def ru(*shape):
        return torch.rand(*shape, generator=gen, device=DEV)
    noise = rn(G, B, C, hw_of(spatial))
    scale = 0.5 + 1.5 * ru(G, 1, C, 1)
    if mean_over_std is None:
        shift = rn(G, 1, C, 1)
    else:
        shift = scale * torch.as_tensor(mean_over_std, dtype=torch.float32, device=DEV).view(1, 1, C, 1)
    x = (noise * scale + shift).reshape(G * B, C, *spatial).contiguous()
    return dict(x=x, gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C), dy=rn(G * B, C, *spatial),
                rm0=0.3 * rn(C), rv0=1 + 0.2 * ru(C))


def reference(inp, G, act, n_updates, full=True):
    """float64, plain torch.  Returns y, dx [G*B, C, *spatial]; dgamma, dbeta [C]; mean, invstd [G, C]; rm, rv [C]."""
    x, gamma, beta = (inp[k].double() for k in ('x', 'gamma', 'beta'))
    GB, C = x.shape[0], x.shape[1]
    B = GB // G
    xg = x.reshape(G, B, C, -1)
    n = B * xg.shape[3]
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))          # biased
    invstd = (var + EPS).rsqrt()
    rm, rv = inp['rm0'].double().clone(), inp['rv0'].double().clone()
    unb = n / (n - 1.0) if n > 1 else 1.0
    for g in range(G):
        for _ in range(n_updates):
            rm = (1 - MOMENTUM) * rm + MOMENTUM * mean[g]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * (var[g] * unb)
    out = dict(mean=mean, invstd=invstd, rm=rm, rv=rv)
    if not full:
        return out
    xh = (xg - mean[:, None, :, None]) * invstd[:, None, :, None]
    h = gamma[None, None, :, None] * xh + beta[None, None, :, None]
    dh = inp['dy'].double().reshape(G, B, C, -1)
    if act:
        dh = dh * swish_grad(h)
    m1 = dh.mean(dim=(1, 3), keepdim=True)
    m2 = (dh * xh).mean(dim=(1, 3), keepdim=True)
    dx = (gamma[None, None, :, None] * invstd[:, None, :, None]) * (dh - m1 - xh * m2)
    out.update(y=(swish(h) if act else h).reshape(x.shape), dx=dx.reshape(x.shape),
               dgamma=(dh * xh).sum(dim=(0, 1, 3)), dbeta=dh.sum(dim=(0, 1, 3)))
    return out


def slice_err(got, ref, G):
    """max over the (group, channel) slices of  max |got - ref| over the slice / max |ref| over the slice."""
    C = ref.shape[1]
    e = (got.double() - ref).abs().reshape(G, -1, C, hw_of(ref.shape[2:])).amax(dim=(1, 3))
    d = ref.abs().reshape(G, -1, C, hw_of(ref.shape[2:])).amax(dim=(1, 3))
    return (e / d.clamp_min(1e-30)).max().item()


def elem_err(got, ref):
    assert got.shape == ref.shape
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def check(errs, bounds, what):
    """errs: {name: figure}.  Prints every figure before it asserts (NaN fails: it is not <= the bound)."""
    print('bn-route %s: %s' % (what, ' '.join('%s=%.2e' % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        bound = bounds[k] if isinstance(bounds, dict) else (RUN_TOL if k in ('rm', 'rv') else bounds)
        assert e <= bound, '%s: %s error %.3e > %.1e' % (what, k, e, bound)


def run_fwd(inp, G, act, y=True, running=True, n_updates=2, n_updates_dev=None, off=False):
    x = shifted(inp['x']) if off else inp['x']
    C = x.shape[1]
    out = dict(y=(shifted(nans(*x.shape)) if off else nans(*x.shape)) if y else None, sm=nans(G, C), si=nans(G, C),
               rm=inp['rm0'].clone() if running else None, rv=inp['rv0'].clone() if running else None)
    K.bn_train_fwd(x, inp['gamma'], inp['beta'], out['y'], out['sm'], out['si'], out['rm'], out['rv'], G, eps=EPS,
                   momentum=MOMENTUM, n_updates=n_updates, swish=act, n_updates_dev=n_updates_dev)
    return out


def run_bwd(inp, fwd, G, act, off=False, prefill=None):
    x, dy = (shifted(inp[k]) if off else inp[k] for k in ('x', 'dy'))
    C = x.shape[1]
    dx = shifted(nans(*x.shape)) if off else nans(*x.shape)
    dg, db = (nans(C), nans(C)) if prefill is None else (prefill[0].clone(), prefill[1].clone())
    K.bn_train_bwd(dy, x, inp['gamma'], inp['beta'], fwd['sm'], fwd['si'], dx, dg, db, G, swish=act,
                   accumulate=prefill is not None)
    return dict(dx=dx, dgamma=dg, dbeta=db)


def fwd_errs(out, ref, G):
    e = dict(sm=elem_err(out['sm'], ref['mean']), si=elem_err(out['si'], ref['invstd']))
    if out['y'] is not None:
        e['y'] = slice_err(out['y'], ref['y'], G)
    if out['rm'] is not None:
        e.update(rm=elem_err(out['rm'], ref['rm']), rv=elem_err(out['rv'], ref['rv']))
    return e


def bwd_errs(out, ref, G):
    return dict(dx=slice_err(out['dx'], ref['dx'], G), dgamma=elem_err(out['dgamma'], ref['dgamma']),
                dbeta=elem_err(out['dbeta'], ref['dbeta']))


# ----------------------------------------------------------------------------- one case per route and direction
# (G, B, C, spatial, forward route, backward route, what the shape reaches); 'off': x, y / dy and dx one float into a larger
# buffer.  A route of None: that direction is not run.  Every shape is the one the issue proposed: the query confirmed each.
CASES = [
    # --- two-launch, lanes along a row (never run before this file: every earlier spatial shape had HW / 4 = tx)
    (4, 3, 5, (6, 6), 'two_vec_cols', 'two_vec_cols', 'tail loop only: 9 float4 columns on 8 lanes'),
    (1, 24, 3, (28, 28), 'two_vec_cols', 'two_vec_cols', '196 columns on 128 lanes, S = 3, ragged last slice'),
    (1, 5, 2, (64, 64), 'two_vec_cols', 'two_vec_cols', 'the 4-way unrolled trip (1024 columns on 256 lanes), S = 3 ragged'),
    (4, 2, 3, (64, 64), 'two_vec_cols', 'two_vec_cols', 'the unrolled trip with groups'),
    # --- two-launch, rows in parallel
    (1, 65, 2, (16, 16), 'two_vec_rows', 'two_vec_rows', 'one row past the fused limit: S = 3, one row in the last slice'),
    (1, 2056, 1, (32, 32), 'two_vec_rows', 'two_vec_rows', 'S = 257: the second trip of bn_merge_block, two non-empty waves'),
    # --- two-launch, one element per lane
    (1, 656, 3, (5, 5), 'two_scalar', 'two_scalar', 'one row past the fused limit, odd width'),
    (2, 328, 2, (5, 5), 'two_scalar', 'two_scalar', 'one row past the halved limit of several groups'),
    (4, 16, 17, (), 'two_scalar', 'two_scalar', 'BatchNorm1d with more groups than its kernel takes'),
    (1, 513, 17, (), 'two_scalar', 'two_scalar', 'BatchNorm1d one row past its kernel'),
    (4, 8, 4, (8, 8), 'two_scalar', 'two_scalar', 'off'),
    # --- all groups in one block, float4 units: n = 16384 exactly, every register unit live
    (1, 64, 2, (16, 16), 'fused_vec_g1', 'fused_vec_g1', 'n = 16384'),
    (2, 64, 2, (16, 16), 'fused_vec_g2', 'fused_vec_g2', 'n = 16384'),
    (3, 64, 2, (16, 16), 'fused_vec_g3', 'two_vec_rows', 'n = 16384; the backward takes two groups at most'),
    (1, 3, 8, (2, 2), 'fused_vec_g1', 'fused_vec_g1', 'three float4 units in the whole block'),
    # --- all groups in one block, one element per register
    (1, 655, 2, (5, 5), 'fused_scalar_g1', 'fused_scalar_g1', 'n = 16375: the last of 16 units ragged'),
    (1, 64, 2, (16, 16), 'fused_scalar_g1', 'fused_scalar_g1', 'off'),
    (2, 327, 2, (5, 5), 'fused_scalar_gn', 'fused_scalar_gn', 'n = 8175: the last of 8 units ragged'),
    (3, 40, 3, (5, 5), 'fused_scalar_gn', 'two_scalar', 'three groups: forward only'),
    # --- BatchNorm1d columns
    (1, 512, 17, (), 'bn1d_g1', 'bn1d_g1', 'all 8 rows per thread, a ragged second column block'),
    (3, 512, 1, (), 'bn1d_gn', 'bn1d_gn', 'one column'),
    (2, 300, 40, (), 'bn1d_gn', 'bn1d_gn', 'two of three groups, ragged rows'),
    (3, 1, 16, (), 'bn1d_gn', 'bn1d_gn', 'B = 1: variance 0, unbiased factor 1'),
    # --- a block per (channel, group) slice
    (8, 65, 64, (16, 16), 'slice', 'two_vec_rows', 'C * G = 512, 65 rows on 16 per pass'),
    (8, 65, 63, (16, 16), 'two_vec_rows', None, 'its neighbour with 504 slices'),
    (1, 342, 512, (6, 8), 'two_vec_cols', None, 'HW / 4 = 12 does not divide the 1024 threads'),
    # --- shapes n / 8192 + 2 slices refused
    (1, 32, 2, (56, 56), 'two_vec_cols', 'two_vec_cols', 'S = 16'),
    (1, 64, 1, (48, 48), 'two_vec_cols', 'two_vec_cols', 'S = 22'),
    (1, 6, 2, (72, 72), 'two_vec_cols', 'two_vec_cols', 'S = 6'),
    (1, 64, 1, (41, 100), 'two_vec_cols', 'two_vec_cols', 'S = 64: HW = 4100, a row per slice'),
]


def case_id(c):
    return '%dx%dx%d%s%s' % (c[0], c[1], c[2], ''.join('x%d' % d for d in c[3]), '-off' if c[6] == 'off' else '')


def test_cases_cover_every_route_in_both_directions():
    fwd = {c[4] for c in CASES if c[4]}
    bwd = {c[5] for c in CASES if c[5]}
    names = set(_lib.BN_ROUTES.values())
    assert fwd == names
    assert bwd == names - {'fused_vec_g3', 'slice'}        # forward-only forms (norm.hip: bn_fused_kind)


@pytest.mark.parametrize('act', [True, False], ids=['swish', 'plain'])
@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_route(case, act):
    G, B, C, spatial, want_fwd, want_bwd, note = case
    off = note == 'off'
    HW = hw_of(spatial)
    inp = inputs(G, B, C, spatial, seed=CASES.index(case))
    ref = reference(inp, G, act, 2)
    assert K.bn_route(G, B, C, HW, aligned=not off)[0] == want_fwd
    fwd = run_fwd(inp, G, act, off=off)
    check(fwd_errs(fwd, ref, G), REL_TOL, '%s fwd %s' % (want_fwd, case_id(case)))
    if want_bwd is None:
        return
    assert K.bn_route(G, B, C, HW, bwd=True, aligned=not off)[0] == want_bwd
    # the backward reads the saved statistics: hand it the reference's, so a forward error is not judged twice
    saved = dict(sm=ref['mean'].float(), si=ref['invstd'].float())
    bwd = run_bwd(inp, saved, G, act, off=off)
    check(bwd_errs(bwd, ref, G), REL_TOL, '%s bwd %s' % (want_bwd, case_id(case)))


def test_slice_form_at_the_workload_slice_size():
    """n = 65536, the largest slice the form takes (all 16 float4 units of every thread live), statistics only -- the one
    way the shipped step calls it (celeba19's 18-group pass).  134 MB of input, generated and reduced on the device."""
    G, B, C, spatial = 2, 64, 256, (32, 32)
    assert K.bn_route(G, B, C, 1024) == ('slice', 1, 2)
    inp = inputs(G, B, C, spatial, seed=90)
    del inp['dy']
    ref = reference(inp, G, True, 2, full=False)
    out = run_fwd(inp, G, True, y=False)
    check(fwd_errs(out, ref, G), REL_TOL, 'slice fwd stats-only 2x64x256x32x32')


# ----------------------------------------------------------------------------- one shape per family
# forward families: all groups in one block, BatchNorm1d columns, two-launch, slice + bn_running_kernel
FWD_FAMILIES = [('fused_vec_g2', 2, 6, 5, (4, 4)), ('bn1d_gn', 3, 9, 17, ()), ('two_vec_cols', 4, 3, 5, (6, 6)),
                ('slice', 8, 65, 64, (16, 16))]
BWD_FAMILIES = [('fused_vec_g2', 2, 6, 5, (4, 4)), ('fused_scalar_g1', 1, 7, 3, (5, 5)), ('bn1d_gn', 3, 9, 17, ()),
                ('two_vec_cols', 4, 3, 5, (6, 6)), ('two_vec_rows', 3, 33, 2, (16, 16)), ('two_scalar', 4, 5, 3, (5, 5))]
FAM_IDS = lambda fams: [f[0] for f in fams]


@pytest.mark.parametrize('family', FWD_FAMILIES, ids=FAM_IDS(FWD_FAMILIES))
def test_device_side_update_count(family):
    """n_updates_dev (what the captured steps pass: graph replays vary the count) overrides n_updates: 3 on the device
    against 1 in the argument is three updates; 0 leaves the running statistics alone and y as it was."""
    route, G, B, C, spatial = family
    assert K.bn_route(G, B, C, hw_of(spatial))[0] == route
    inp = inputs(G, B, C, spatial, seed=50)
    ref = reference(inp, G, True, 3, full=False)
    count = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    out = run_fwd(inp, G, True, n_updates=1, n_updates_dev=count)
    check(dict(rm=elem_err(out['rm'], ref['rm']), rv=elem_err(out['rv'], ref['rv'])), REL_TOL, '%s n_updates_dev = 3' % route)
    one = reference(inp, G, True, 1, full=False)
    assert elem_err(out['rm'], one['rm']) > 100 * RUN_TOL        # the inputs can tell three updates from one
    count.zero_()
    again = dict(inp, rm0=out['rm'], rv0=out['rv'])
    out0 = run_fwd(again, G, True, n_updates=1, n_updates_dev=count)
    assert torch.equal(out0['rm'], out['rm']) and torch.equal(out0['rv'], out['rv'])
    assert torch.equal(out0['y'], out['y']) and torch.equal(out0['sm'], out['sm']) and torch.equal(out0['si'], out['si'])


@pytest.mark.parametrize('family', FWD_FAMILIES, ids=FAM_IDS(FWD_FAMILIES))
def test_without_running_statistics_and_statistics_only(family):
    """running_mean = running_var = NULL changes neither y nor the saved statistics; y = NULL changes neither the saved nor
    the running statistics -- bit for bit."""
    route, G, B, C, spatial = family
    assert K.bn_route(G, B, C, hw_of(spatial))[0] == route
    inp = inputs(G, B, C, spatial, seed=51)
    for act in (True, False):
        full = run_fwd(inp, G, act)
        bare = run_fwd(inp, G, act, running=False)
        assert torch.equal(bare['y'], full['y']) and torch.equal(bare['sm'], full['sm']) and torch.equal(bare['si'], full['si'])
        assert not torch.isnan(full['y']).any()
        stats = run_fwd(inp, G, act, y=False)
        assert torch.equal(stats['sm'], full['sm']) and torch.equal(stats['si'], full['si'])
        assert torch.equal(stats['rm'], full['rm']) and torch.equal(stats['rv'], full['rv'])
        neither = run_fwd(inp, G, act, y=False, running=False)
        assert torch.equal(neither['sm'], full['sm']) and torch.equal(neither['si'], full['si'])


@pytest.mark.parametrize('family', BWD_FAMILIES, ids=FAM_IDS(BWD_FAMILIES))
def test_accumulate(family):
    """MVAE_ACCUMULATE adds dgamma AND dbeta to what the buffers hold (one fp32 add per channel: bit-exact against the plain
    call's result plus the pre-fill) and still overwrites dx."""
    route, G, B, C, spatial = family
    assert K.bn_route(G, B, C, hw_of(spatial), bwd=True)[0] == route
    inp = inputs(G, B, C, spatial, seed=52)
    ref = reference(inp, G, True, 1)
    saved = dict(sm=ref['mean'].float(), si=ref['invstd'].float())
    plain = run_bwd(inp, saved, G, True)
    check(bwd_errs(plain, ref, G), REL_TOL, '%s bwd plain' % route)
    gen = torch.Generator(device=DEV).manual_seed(53)
    pre = (3 + torch.rand(C, generator=gen, device=DEV), -5 - torch.rand(C, generator=gen, device=DEV))
    acc = run_bwd(inp, saved, G, True, prefill=pre)
    assert torch.equal(acc['dgamma'], plain['dgamma'] + pre[0])
    assert torch.equal(acc['dbeta'], plain['dbeta'] + pre[1])
    assert torch.equal(acc['dx'], plain['dx'])
    want = dict(ref, dgamma=ref['dgamma'] + pre[0].double(), dbeta=ref['dbeta'] + pre[1].double())
    check(bwd_errs(acc, want, G), REL_TOL, '%s bwd accumulate' % route)


# ----------------------------------------------------------------------------- channel means far from zero
FAR = [100.0, -100.0, 100.0, -100.0]


@pytest.mark.parametrize('route,G,B,C,spatial', [('two_vec_rows', 1, 65, 4, (16, 16)), ('two_vec_cols', 1, 24, 4, (28, 28)),
                                                 ('fused_vec_g1', 1, 64, 4, (16, 16))],
                         ids=['two_vec_rows', 'two_vec_cols', 'fused_vec_g1'])
def test_channel_mean_far_from_zero(route, G, B, C, spatial):
    """x = m_c + s_c * noise with m_c / s_c = +-100: the one-pass statistics of the two-launch kernels (sums of x - p and
    (x - p)^2 around the slice's first element; norm.hip claims they lose 'a bit or two') and the two-pass statistics of the
    all-groups-in-one-block kernels.  Bound per figure: 4 x the error of fp32 F.batch_norm on the CPU against the float64
    reference on these exact inputs, never less than REL_TOL (running statistics: RUN_TOL).

    Measured on the MI355X, Swish on, fp32 CPU reference -> kernel (the backward on the kernel's own saved statistics):
      two_vec_rows  1x65x4x16x16   y 1.8e-6 -> 2.1e-6   dx 3.0e-6 -> 2.9e-6   dgamma 4.1e-6 -> 4.8e-6   dbeta 1.9e-6 -> 1.8e-6
                                   running_mean 3.6e-8 -> 3.6e-8   running_var 7.1e-8 -> 7.1e-8
      two_vec_cols  1x24x4x28x28   y 1.9e-6 -> 1.1e-6   dx 2.8e-6 -> 1.9e-6   dgamma 2.4e-6 -> 3.0e-6   dbeta 7.4e-6 -> 3.9e-6
                                   running_mean 4.5e-8 -> 4.5e-8   running_var 5.6e-8 -> 1.0e-7
      fused_vec_g1  1x64x4x16x16   y 1.5e-6 -> 3.4e-6   dx 2.1e-6 -> 5.9e-6   dgamma 1.5e-6 -> 1.2e-5   dbeta 2.1e-6 -> 4.6e-6
                                   running_mean 6.9e-8 -> 1.6e-7   running_var 2.6e-8 -> 7.6e-8
    4 x the reference's error is below the floor everywhere, so every bound is REL_TOL (RUN_TOL).  The pivot statistics hold
    their claim: the two-launch kernels are at the fp32 reference's own error.  The largest figure is the two-pass kernel's
    dgamma at 8 x the reference's (its mean is one fp32 sum of 16384 values near 100 s): 8 x below the bound.
    """
    assert K.bn_route(G, B, C, hw_of(spatial))[0] == route and K.bn_route(G, B, C, hw_of(spatial), bwd=True)[0] == route
    inp = inputs(G, B, C, spatial, seed=60, mean_over_std=FAR)
    ratio = (inp['x'].double().mean(dim=(0, 2, 3)) / inp['x'].double().std(dim=(0, 2, 3))).abs()
    assert ((ratio > 95) & (ratio < 105)).all()
    ref = reference(inp, G, True, 2)
    # the fp32 reference, on the CPU
    xc = inp['x'].cpu().requires_grad_()
    gc, bc = inp['gamma'].cpu().requires_grad_(), inp['beta'].cpu().requires_grad_()
    rmc, rvc = inp['rm0'].cpu().clone(), inp['rv0'].cpu().clone()
    for _ in range(2):
        yc = swish(F.batch_norm(xc, rmc, rvc, gc, bc, True, MOMENTUM, EPS))
    yc.backward(inp['dy'].cpu())
    cpu = dict(y=yc.detach(), dx=xc.grad, dgamma=gc.grad, dbeta=bc.grad, rm=rmc, rv=rvc)
    cpu = {k: v.to(DEV) for k, v in cpu.items()}
    base = dict(y=slice_err(cpu['y'], ref['y'], G), dx=slice_err(cpu['dx'], ref['dx'], G))
    base.update({k: elem_err(cpu[k], ref[k]) for k in ('dgamma', 'dbeta', 'rm', 'rv')})
    print('bn-route far %s fp32 CPU reference: %s' % (route, ' '.join('%s=%.2e' % kv for kv in sorted(base.items()))))
    bounds = {k: max(4 * e, RUN_TOL if k in ('rm', 'rv') else REL_TOL) for k, e in base.items()}
    bounds.update(sm=REL_TOL, si=REL_TOL)          # F.batch_norm does not return what it saved
    fwd = run_fwd(inp, G, True)
    check(fwd_errs(fwd, ref, G), bounds, 'far %s fwd' % route)
    bwd = run_bwd(inp, fwd, G, True)               # on the kernel's OWN saved statistics: the chain the step runs
    check(bwd_errs(bwd, ref, G), bounds, 'far %s bwd' % route)


# ----------------------------------------------------------------------------- eval mode
@pytest.mark.parametrize('N,C,spatial', [(4100, 257, ()), (70, 600, (5, 5)), (1050000, 1, ())],
                         ids=['4100x257', '70x600x5x5', '1050000x1'])
def test_eval_past_the_grid_cap(N, C, spatial):
    """More than 4096 x 256 elements: bn_eval_kernel's grid stride (the earlier test held 12 K)."""
    assert N * C * hw_of(spatial) > 4096 * 256
    inp = inputs(1, N, C, spatial, seed=70)
    x, gamma, beta, rm, rv = (inp[k] for k in ('x', 'gamma', 'beta', 'rm0', 'rv0'))
    shape = (1, 1, C) + (1,) * len(spatial)
    h = ((x.double() - rm.double().view(shape[1:])) * (rv.double().view(shape[1:]) + EPS).rsqrt() * gamma.double().view(shape[1:])
         + beta.double().view(shape[1:]))
    for act in (True, False):
        y = nans(*x.shape)
        K.bn_eval_fwd(x, gamma, beta, y, rm, rv, eps=EPS, swish=act)
        check(dict(y=slice_err(y, swish(h) if act else h, 1)), REL_TOL, 'eval %s act=%s' % ('x'.join(map(str, x.shape)), act))


# ----------------------------------------------------------------------------- statistics from conv records
def test_stats_merge_directly():
    """mvae_bn_stats_merge on synthetic (mean, M2) records: 70 tiles per group (a second trip of the lane loop, ragged) in
    18 groups (a second trip of the wave loop, ragged) against the equal-count merge in float64; save_* = NULL; the
    device-side update count."""
    G, tpg, C, elems = 18, 70, 5, _lib.STATS_TILE_ELEMS
    gen = torch.Generator(device=DEV).manual_seed(80)
    means = (torch.randn(G, tpg, C, generator=gen, device=DEV) * 0.5 + torch.randn(G, 1, C, generator=gen, device=DEV)
             + 3 * torch.randn(1, 1, C, generator=gen, device=DEV))
    m2s = elems * (0.5 + torch.rand(G, tpg, C, generator=gen, device=DEV))
    part = torch.stack([means, m2s], dim=3).reshape(G * tpg, C, 2).contiguous()
    rm0, rv0 = 0.3 * torch.randn(C, generator=gen, device=DEV), 1 + 0.2 * torch.rand(C, generator=gen, device=DEV)
    md, qd = means.double(), m2s.double()
    mean = md.mean(dim=1)
    var = (qd.sum(dim=1) + elems * ((md - mean[:, None]) ** 2).sum(dim=1)) / (tpg * elems)
    n = tpg * elems

    def running(n_updates):
        rm, rv = rm0.double().clone(), rv0.double().clone()
        for g in range(G):
            for _ in range(n_updates):
                rm = (1 - MOMENTUM) * rm + MOMENTUM * mean[g]
                rv = (1 - MOMENTUM) * rv + MOMENTUM * (var[g] * n / (n - 1.0))
        return rm, rv
    sm, si, rm, rv = nans(G, C), nans(G, C), rm0.clone(), rv0.clone()
    K.bn_stats_merge(part, G, sm, si, rm, rv, eps=EPS, momentum=MOMENTUM, n_updates=2)
    want = running(2)
    check(dict(sm=elem_err(sm, mean), si=elem_err(si, (var + EPS).rsqrt()), rm=elem_err(rm, want[0]), rv=elem_err(rv, want[1])),
          REL_TOL, 'stats_merge 18 groups x 70 tiles')
    # no saved statistics: the running ones are the same bits
    rm2, rv2 = rm0.clone(), rv0.clone()
    K.bn_stats_merge(part, G, None, None, rm2, rv2, eps=EPS, momentum=MOMENTUM, n_updates=2)
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv)
    # no running statistics: the saved ones are the same bits
    sm3, si3 = nans(G, C), nans(G, C)
    K.bn_stats_merge(part, G, sm3, si3, None, None, eps=EPS, momentum=MOMENTUM, n_updates=2)
    assert torch.equal(sm3, sm) and torch.equal(si3, si)
    # the device-side count: 3 against n_updates = 1, then 0
    count = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    rm4, rv4 = rm0.clone(), rv0.clone()
    K.bn_stats_merge(part, G, None, None, rm4, rv4, eps=EPS, momentum=MOMENTUM, n_updates=1, n_updates_dev=count)
    want = running(3)
    check(dict(rm=elem_err(rm4, want[0]), rv=elem_err(rv4, want[1])), REL_TOL, 'stats_merge n_updates_dev = 3')
    count.zero_()
    rm5, rv5 = rm4.clone(), rv4.clone()
    K.bn_stats_merge(part, G, None, None, rm5, rv5, eps=EPS, momentum=MOMENTUM, n_updates=1, n_updates_dev=count)
    assert torch.equal(rm5, rm4) and torch.equal(rv5, rv4)
