"""GPU: every kernel and loop of the loss launches (csrc/loss.hip: BCE row sums, categorical CE, group sums, the one-launch
ELBO) and the elementwise BCE of misc.hip, at the cheapest shape that still reaches the path's tails.  Every case

  * first asserts (the BCE cases), through the host-only query ``kernels.bce_route`` (the functions the launch and the
    kernel themselves switch on), which kernel and loop each of its rows is on -- a threshold that moves fails the case
    instead of quietly testing other code;
  * allocates every output full of NaN with a sentinel guard band behind it (and in front of it where the view is offset)
    that must stay untouched;
  * is judged against a float64 reference written in plain torch below: ``clamp(x,0) - x*t + log1p(exp(-|x|))`` and
    ``sigmoid(x) - t``, ``-log_softmax(x + 1e-6)[y]`` and ``softmax - onehot``, plain sums.

Inputs have their own scale per row and per group (mixed-up rows show); no logit is exactly 0 (asserted; the sub-gradient
test stays in test_kernels_gpu.py).  Rows fed to the sum kernels are positive (0.5 + rand, as loss rows are), so the
relative measure is well conditioned.

Error measure: row sums, ELBO entries and group sums elementwise against max |ref| of the tensor; dlogits per row -- max
|err| over the row / max |ref| over the row, so a row with a small drow cannot hide behind another; rows of a group whose
drow is 0 must be exactly zero.  Bound: util.REL_TOL = 1e-4 (the saturated rows: never less than that, see there).

tests/test_loss_routes_cpu.py pins the gates themselves and the launches' host-side refusals (nothing here passes an
invalid argument; the bad-label case is the kernel's defined NaN behaviour).

Measured on the MI355X (worst figure of each family; bound 1e-4 everywhere):
  BCE wave               rows 6.7e-8   dlogits 9.9e-8        BCE block_vec          rows 1.1e-7   dlogits 1.2e-7
  BCE block_vec_batched  rows 7.5e-8   dlogits 1.1e-7        BCE block_scalar       rows 8.4e-8   dlogits 1.2e-7
  BCE per-row routes     rows 7.0e-8   dlogits 1.0e-7        BCE transposed target  rows 8.5e-8   dlogits 9.2e-8
  CE 257x10              rows 5.7e-8   dlogits 1.3e-6        CE 257x1024            rows 9.8e-8   dlogits 6.3e-7
  CE 24x10 scale 2       rows 4.6e-8   dlogits 2.0e-7        CE 24x10 scale 30      rows 3.7e-8   dlogits 2.3e-6
  group_sums             out 9.2e-8    total 9.2e-8          bce_elem               out 7.4e-8    dx 7.3e-8   dt 4.8e-8
  elbo_reduce 513x3 3.9e-8, Lx3 4.0e-8, L+1x3 6.5e-8, 12800x3 1.7e-8, 21x70 3.4e-8, mixed 2.5e-8 (entry by entry 9.4e-8),
  1024 groups 7.2e-7 (thread 0 adds the 1024 weighted sums one after the other); one edge row at a time 1.5e-6 of the step;
  elbo_reduce_prepare 6.5e-8.  Saturated rows: see test_bce_saturated_logits.  No case came near the bound, and no kernel
  was changed for one.  Checked once against a library whose kernels drop a tail each (the last float4 group of the
  single-group loop, the last row of a spread group, of a group_sums group, the last float of the clear) or ignore the
  column stride or the label period: every mutation failed the cases that reach it.
"""
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib
from mvae_amd import kernels as K
from util import REL_TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD, SENTINEL = 64, -77.0
L = _lib.ELBO_LONG_GROUP
NAN = float('nan')


# ----------------------------------------------------------------------------- buffers
def guarded(*shape, off=0, dtype=torch.float32):
    """(view, flat): an output no kernel has written (NaN: a region a launch skips shows), ``off`` floats into a buffer of
    sentinels, with a guard band of sentinels behind it."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((off + n + GUARD,), SENTINEL, device=DEV, dtype=dtype)
    view = flat[off:off + n].view(*shape)
    view.fill_(NAN)
    assert view.data_ptr() % 16 == 4 * (off % 4) and view.is_contiguous()
    return view, flat


def guard_ok(view, flat):
    off = (view.data_ptr() - flat.data_ptr()) // flat.element_size()
    return bool((flat[:off] == SENTINEL).all()) and bool((flat[off + view.numel():] == SENTINEL).all())


def shifted(t):
    """The same values one float into a larger buffer: contiguous, but not 16-byte aligned."""
    buf = torch.full((t.numel() + 1,), NAN, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(4000 + seed)


def elem_err(got, ref):
    assert got.shape == ref.shape
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def row_err(got, ref):
    """max over the rows of  max |got - ref| over the row / max |ref| over the row; a row whose reference is all zero (the
    rows of a group with drow = 0) must be exactly zero."""
    assert got.shape == ref.shape
    e = (got.double() - ref).abs().amax(dim=1)
    d = ref.abs().amax(dim=1)
    dead = d == 0
    assert bool((got[dead] == 0).all()), 'a row whose drow is 0 is not exactly zero'
    if bool(dead.all()):
        return 0.0
    return (e[~dead] / d[~dead]).max().item()


def check(errs, bounds, what):
    """errs: {name: figure}.  Prints every figure before it asserts (NaN fails: it is not <= the bound)."""
    print('loss-route %s: %s' % (what, ' '.join('%s=%.2e' % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        bound = bounds[k] if isinstance(bounds, dict) else bounds
        assert e <= bound, '%s: %s error %.3e > %.1e' % (what, k, e, bound)


# ============================================================================= BCE row sums
# (route, P, form, (batched_trips, tail) or None, what the shape reaches).  Forms:
#   plain     logits [R, P], target [2, P] contiguous (target row r % 2); R = 5 on the wave kernel, 6 on the block kernel
#   colw      plain + column weights [groups, P]
#   celeba19  logits [A * S, B] with A = 5, S = 3, P = B; targets are column a of attrs[B, A]: target_rows = A,
#             target_div = S, strides (1, A)
#   off_x / off_t / off_d / off_w   plain (off_w: colw) with that operand one float into a larger buffer
#   trs517    plain with the two target rows 517 floats apart: row 0 aligned, row 1 not -- the route differs by row
BCE_CASES = [
    ('wave', 1, 'plain', None, 'one lane'),
    ('wave', 63, 'plain', None, 'one trip, the last lane idle'),
    ('wave', 64, 'plain', None, 'one full trip'),
    ('wave', 65, 'plain', None, 'a second trip for lane 0 alone'),
    ('wave', 511, 'plain', None, "the gate's lower side: 8 trips, the last lane idle in the last"),
    ('wave', 70, 'celeba19', None, 'strided targets with target_div'),
    ('wave', 18, 'colw', None, 'CelebA attribute rows: column weights per group'),
    ('block_vec', 512, 'plain', (0, 1), 'P / 4 = 128: half the block idle'),
    ('block_vec', 784, 'plain', (0, 1), 'MNIST: 196 groups'),
    ('block_vec', 4096, 'colw', (0, 1), 'weighted rows stay off the batched loop'),
    ('block_vec_batched', 4096, 'plain', (1, 0), 'one trip for every thread, no tail'),
    ('block_vec_batched', 4092, 'plain', (1, 1), 'P / 4 = 1023: thread 255 alone has no batched trip'),
    ('block_vec_batched', 4100, 'plain', (1, 1), 'a batched trip, then a tail for thread 0 only'),
    ('block_vec_batched', 7296, 'plain', (2, 1), 'P / 4 = 1824: a second batched trip for threads 0..31, tails for the rest'),
    ('block_scalar', 513, 'plain', None, 'P % 4 = 1'),
    ('block_scalar', 515, 'plain', None, 'P % 4 = 3'),
    ('block_scalar', 516, 'off_x', None, 'logits unaligned'),
    ('block_scalar', 516, 'off_t', None, 'target unaligned'),
    ('block_scalar', 516, 'off_d', None, 'dlogits unaligned (the forward alone stays on float4)'),
    ('block_scalar', 516, 'off_w', None, 'column weights unaligned'),
    ('block_scalar', 512, 'celeba19', None, 'celeba19 at batch 512: strided targets on the block kernel'),
    ('per_row', 516, 'trs517', None, 'target rows alternate between aligned and not'),
]
A19, S19 = 5, 3


def bce_id(c):
    return '%s-%d-%s' % (c[0], c[1], c[2])


def test_bce_cases_cover_every_route():
    assert {c[0] for c in BCE_CASES} - {'per_row'} == set(_lib.BCE_ROUTES.values())
    assert len({bce_id(c) for c in BCE_CASES}) == len(BCE_CASES)


def bce_build(P, form, seed, wave):
    """The operands of a case (the same for both groupings): logits x [R, P], the target buffer and how to address it,
    tmat [R, P] (the target of every logit, gathered by that addressing), optional column weights for up to R groups."""
    g = gen(seed)
    c19 = form == 'celeba19'
    R = A19 * S19 if c19 else (5 if wave else 6)
    scale = (1 + 0.5 * torch.arange(R, device=DEV)).unsqueeze(1)
    x = torch.randn(R, P, generator=g, device=DEV) * scale
    assert bool((x != 0).all()), 'a logit is exactly 0'
    if c19:
        tb = (torch.rand(P, A19, generator=g, device=DEV) > 0.5).float() * 0.9 + 0.05       # attrs [B, A]
        trows, div, t_rs, t_cs = A19, S19, 1, A19
    elif form == 'trs517':
        tb = torch.full((2 * 517,), NAN, device=DEV)
        tb[:P] = torch.rand(P, generator=g, device=DEV)
        tb[517:517 + P] = torch.rand(P, generator=g, device=DEV)
        trows, div, t_rs, t_cs = 2, 1, 517, 1
    else:
        tb = torch.rand(2, P, generator=g, device=DEV)
        trows, div, t_rs, t_cs = 2, 1, P, 1
    w = None
    if form in ('colw', 'off_w'):
        w = torch.rand(R, P, generator=g, device=DEV) * (1 + torch.arange(R, device=DEV)).unsqueeze(1)
    if form == 'off_x':
        x = shifted(x)
    if form == 'off_t':
        tb = shifted(tb)
    if form == 'off_w':
        w = shifted(w)
    trow = (torch.arange(R, device=DEV) // div) % trows
    offs = trow.unsqueeze(1) * t_rs + torch.arange(P, device=DEV).unsqueeze(0) * t_cs
    tmat = tb.reshape(-1)[offs].double()
    assert not bool(torch.isnan(tmat).any())
    return dict(x=x, tb=tb, w=w, tmat=tmat, trow=trow.tolist(), R=R, P=P, form=form,
                addr=dict(target_rows=trows, target_div=div, target_strides=(t_rs, t_cs)))


def bce_reference(c, rpg, drow):
    x = c['x'].double()
    R = c['R']
    grp = torch.arange(R, device=DEV) // rpg
    el = torch.clamp(x, min=0) - x * c['tmat'] + torch.log1p(torch.exp(-x.abs()))
    gr = torch.sigmoid(x) - c['tmat']
    if c['w'] is not None:
        wr = c['w'].double()[grp]
        el, gr = el * wr, gr * wr
    return el.sum(dim=1), drow.double()[grp].unsqueeze(1) * gr


def bce_routes(c, rpg, dl):
    """The route of every logits row from the pointers the kernel will see for it."""
    P, (t_rs, t_cs) = c['P'], c['addr']['target_strides']
    out = []
    for r in range(c['R']):
        ptrs = [c['x'].data_ptr() + 4 * P * r, c['tb'].data_ptr() + 4 * t_rs * c['trow'][r]]
        if c['w'] is not None:
            ptrs.append(c['w'].data_ptr() + 4 * P * (r // rpg))
        if dl is not None:
            ptrs.append(dl.data_ptr() + 4 * P * r)
        out.append(K.bce_route(P, aligned=all(p % 16 == 0 for p in ptrs), target_col_stride=t_cs, colw=c['w'] is not None))
    return out


DROW3 = (0.5, 0.0, 2.0)
DROW_ROWS = (0.5, 0.0, 2.0, 1.3, 0.0, 0.7)


def grouping(R, per_row):
    """(rows_per_group, drow): three groups with drow = (0.5, 0, 2), or a group per row."""
    if per_row:
        return 1, torch.tensor([DROW_ROWS[r % 6] * (1 + r // 6) for r in range(R)], device=DEV)
    rpg = (R + 2) // 3
    assert (R + rpg - 1) // rpg == 3
    return rpg, torch.tensor(DROW3, device=DEV)


def bce_run(c, rpg, drow, mode):
    """mode 'fused' (forward with gradient), 'fwd' (forward alone), 'bwd' (backward alone) -> (rows, dlogits, routes)"""
    R, P = c['R'], c['P']
    off = 1 if c['form'] == 'off_d' else 0
    rows, rows_flat = guarded(R) if mode != 'bwd' else (None, None)
    dl, dl_flat = guarded(R, P, off=off) if mode != 'fwd' else (None, None)
    routes = bce_routes(c, rpg, dl)
    if mode == 'bwd':
        K.bce_rowsum_bwd(c['x'], c['tb'], drow, dl, colw=c['w'], rows_per_group=rpg, **c['addr'])
    else:
        K.bce_rowsum_fwd(c['x'], c['tb'], rows, colw=c['w'], drow=drow if dl is not None else None, dlogits=dl,
                         rows_per_group=rpg, **c['addr'])
    assert rows is None or guard_ok(rows, rows_flat), 'row sums written outside [0, R)'
    assert dl is None or guard_ok(dl, dl_flat), 'dlogits written outside [R, P]'
    return rows, dl, routes


@pytest.mark.parametrize('per_row', [False, True], ids=['3groups', 'rpg1'])
@pytest.mark.parametrize('case', BCE_CASES, ids=[bce_id(c) for c in BCE_CASES])
def test_bce_route(case, per_row):
    want, P, form, trips_tail, _ = case
    c = bce_build(P, form, BCE_CASES.index(case), want == 'wave')
    rpg, drow = grouping(c['R'], per_row)
    ref_rows, ref_grad = bce_reference(c, rpg, drow)
    for mode in ('fused', 'fwd', 'bwd'):
        rows, dl, routes = bce_run(c, rpg, drow, mode)
        names = [r[0] for r in routes]
        if want == 'per_row':
            # target rows 0 (aligned) and 1 (4 bytes past a 16-byte boundary): both loops in one launch, one row each
            assert names == ['block_vec', 'block_scalar'] * 3, names
        elif form == 'off_d' and mode == 'fwd':
            assert set(names) == {'block_vec'}, names
        else:
            assert set(names) == {want}, names
            if trips_tail is not None:
                assert all(r[1:] == trips_tail for r in routes), routes
        errs = {}
        if rows is not None:
            errs['rows'] = elem_err(rows, ref_rows)
        if dl is not None:
            errs['dlogits'] = row_err(dl, ref_grad)
        check(errs, REL_TOL, 'bce %s %s %s' % (bce_id(case), 'rpg1' if per_row else '3groups', mode))


@pytest.mark.parametrize('P,form', [(65, 'plain'), (4100, 'plain'), (18, 'colw'), (512, 'celeba19')],
                         ids=['wave-65', 'block-4100', 'wave-18-colw', 'block-512-celeba19'])
def test_bce_bit_for_bit(P, form):
    """The backward alone equals the fused gradient; the row sums with dlogits and without are equal; two runs on the same
    inputs are equal -- bits."""
    c = bce_build(P, form, 50, P < _lib.BCE_BLOCK_MIN_P)
    rpg, drow = grouping(c['R'], False)
    rows_a, dl_a, _ = bce_run(c, rpg, drow, 'fused')
    rows_b, dl_b, _ = bce_run(c, rpg, drow, 'fused')
    rows_f, _, _ = bce_run(c, rpg, drow, 'fwd')
    _, dl_w, _ = bce_run(c, rpg, drow, 'bwd')
    assert not bool(torch.isnan(rows_a).any()) and not bool(torch.isnan(dl_a).any())
    assert torch.equal(rows_a, rows_b) and torch.equal(dl_a, dl_b), 'two runs on the same inputs differ'
    assert torch.equal(rows_a, rows_f), 'the row sums with dlogits and without differ'
    assert torch.equal(dl_a, dl_w), 'the backward alone differs from the fused gradient'


@pytest.mark.parametrize('P', [65, 516], ids=['wave-65', 'block-516'])
def test_bce_strided_target_equals_its_contiguous_copy(P):
    """A strided read of a transposed target [P, 2] (strides (1, 2)) against the same values contiguous: the copy sits one
    float off the float4 path, so both calls run the same one-element loop -- equal bits."""
    c = bce_build(P, 'plain', 60, P < _lib.BCE_BLOCK_MIN_P)
    rpg, drow = grouping(c['R'], False)
    scalar = 'wave' if P < _lib.BCE_BLOCK_MIN_P else 'block_scalar'
    cont = dict(c, tb=shifted(c['tb']))
    tr = dict(c, tb=c['tb'].t().contiguous(), addr=dict(target_rows=2, target_div=1, target_strides=(1, 2)))
    tmat_tr = tr['tb'].reshape(-1)[(torch.tensor(c['trow'], device=DEV).unsqueeze(1)
                                    + 2 * torch.arange(P, device=DEV).unsqueeze(0))].double()
    assert torch.equal(tmat_tr, c['tmat'])
    rows_c, dl_c, routes_c = bce_run(cont, rpg, drow, 'fused')
    rows_t, dl_t, routes_t = bce_run(tr, rpg, drow, 'fused')
    assert {r[0] for r in routes_c} == {scalar} and {r[0] for r in routes_t} == {scalar}
    assert torch.equal(rows_c, rows_t) and torch.equal(dl_c, dl_t)
    ref_rows, ref_grad = bce_reference(c, rpg, drow)
    check(dict(rows=elem_err(rows_t, ref_rows), dlogits=row_err(dl_t, ref_grad)), REL_TOL, 'bce transposed target P=%d' % P)


SATURATED = [17.0, 30.0, 88.0, 89.0, 104.0, 1e4]


@pytest.mark.parametrize('route,P', [('wave', 70), ('block_vec', 784)], ids=['wave-70', 'block_vec-784'])
def test_bce_saturated_logits(route, P):
    """Row 0 holds x in +-{17, 30, 88, 89, 104, 1e4} against t in {0, 0.3, 1} beside ordinary values (at 17 the fp32 sum
    1 + e rounds to 1, at 88 / 89 e leaves the normal range, at 104 exp2 underflows to 0); row 1 is ordinary.  Every value
    and gradient must be finite.  Bound per figure: the larger of REL_TOL and 4 x the error of the same formula in fp32
    torch on the CPU against the float64 reference on these exact inputs.

    Measured on the MI355X, fp32 CPU formula -> kernel:
      wave 2x70        rows 3.3e-8 -> 3.0e-8   dlogits 9.1e-8 -> 4.8e-8
      block_vec 2x784  rows 6.2e-8 -> 6.2e-8   dlogits 1.3e-7 -> 9.4e-8
      the 36 saturated elements on their own: values 4.6e-8, gradients 3.8e-8 (absolute, of a factor in [-1, 1])
    4 x the formula's own error is below the floor, so every bound is REL_TOL.  The kernel's log(1 + e) loses e once 1 + e
    rounds to 1 (|x| >= 17): an absolute 4e-8 per element at most -- the 36 values show nothing larger.
    """
    assert K.bce_route(P)[0] == route
    g = gen(70)
    x = torch.randn(2, P, generator=g, device=DEV) * 2
    t = torch.rand(1, P, generator=g, device=DEV)
    k = 0
    for v in SATURATED:
        for s in (1.0, -1.0):
            for tv in (0.0, 0.3, 1.0):
                x[0, k], t[0, k] = s * v, tv
                k += 1
    assert k == 36 < P and bool((x != 0).all())
    drow = torch.tensor([1.5, 0.5], device=DEV)
    xd, td = x.double(), t.double()
    ref_rows = (torch.clamp(xd, min=0) - xd * td + torch.log1p(torch.exp(-xd.abs()))).sum(dim=1)
    ref_grad = drow.double().unsqueeze(1) * (torch.sigmoid(xd) - td)
    xc, tc = x.cpu(), t.cpu()
    cpu_rows = (torch.clamp(xc, min=0) - xc * tc + torch.log1p(torch.exp(-xc.abs()))).sum(dim=1)
    cpu_grad = drow.cpu().unsqueeze(1) * (torch.sigmoid(xc) - tc)
    assert cpu_rows.dtype == torch.float32 and cpu_grad.dtype == torch.float32
    base = dict(rows=elem_err(cpu_rows.to(DEV), ref_rows), dlogits=row_err(cpu_grad.to(DEV), ref_grad))
    print('loss-route saturated %s fp32 CPU formula: %s' % (route, ' '.join('%s=%.2e' % kv for kv in sorted(base.items()))))
    bounds = {k: max(4 * e, REL_TOL) for k, e in base.items()}
    rows, rows_flat = guarded(2)
    dl, dl_flat = guarded(2, P)
    K.bce_rowsum_fwd(x, t, rows, drow=drow, dlogits=dl, rows_per_group=1, target_rows=1)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(dl).all())
    assert guard_ok(rows, rows_flat) and guard_ok(dl, dl_flat)
    check(dict(rows=elem_err(rows, ref_rows), dlogits=row_err(dl, ref_grad)), bounds, 'saturated %s' % route)
    # the saturated elements on their own: value and gradient of each against float64, relative to that element's own size
    # where it is not tiny (the 36 span 1e-45 .. 1e4: a tensor-wide maximum would hide all but two of them)
    el_ref = (torch.clamp(xd, min=0) - xd * td + torch.log1p(torch.exp(-xd.abs())))[0, :36]
    one, one_flat = guarded(36)
    K.bce_rowsum_fwd(x[0, :36].reshape(36, 1).contiguous(), t[0, :36].reshape(36, 1).contiguous(), one, rows_per_group=1,
                     target_rows=36)
    assert guard_ok(one, one_flat) and bool(torch.isfinite(one).all())
    el_err = ((one.double() - el_ref).abs() / el_ref.abs().clamp_min(1.0)).max().item()
    gr_err = ((dl[0, :36].double() - ref_grad[0, :36]).abs()).max().item() / 1.5          # |sigmoid - t| <= 1
    check(dict(elements=el_err, gradients=gr_err), REL_TOL, 'saturated %s, the 36 elements' % route)


# ============================================================================= categorical CE
CE_CASES = [(257, 10, 2.0), (5, 1, 2.0), (257, 1024, 2.0), (24, 10, 2.0), (24, 10, 30.0)]
_CE = {}


def ce_case(R, Kc, scale):
    """Inputs and the float64 reference of a case, computed once and shared (never modified)."""
    key = (R, Kc, scale)
    if key not in _CE:
        g = gen(100 + R + Kc)
        rpg, label_rows = (R + 1) // 2, R // 2              # two groups; the label table repeats with its own period
        x = torch.randn(R, Kc, generator=g, device=DEV) * scale * (1 + 0.25 * (torch.arange(R, device=DEV) % 3)).unsqueeze(1)
        y = torch.randint(0, Kc, (label_rows,), generator=g, device=DEV)
        if scale > 10:
            # Logits this far apart put softmax within 2^-24 of a one-hot row.  Where the label IS the arg-max, the whole
            # gradient row p - onehot is then below the spacing of fp32 at 1 (p_label rounds to 1): a measure relative to
            # that row's own maximum has no meaning there, in any fp32 evaluation of the formula.  The labels of this case
            # are drawn among the classes that are the arg-max of none of their rows: every row's gradient then holds an
            # entry of at least 1 / K in size, and the loss rows are the large ones (lse - x[label] up to hundreds).
            rows_of = torch.arange(R, device=DEV) % label_rows
            banned = torch.zeros(label_rows, Kc, dtype=torch.bool, device=DEV)
            banned[rows_of, x.argmax(dim=1)] = True
            score = torch.rand(label_rows, Kc, generator=g, device=DEV)
            score[banned] = -1.0
            y = score.argmax(dim=1)
            assert not bool(banned[torch.arange(label_rows, device=DEV), y].any())
        drow = torch.tensor([0.7, 0.0], device=DEV)
        yr = y[torch.arange(R, device=DEV) % label_rows]
        lsm = torch.log_softmax(x.double() + 1e-6, dim=1)
        rows = -lsm.gather(1, yr.unsqueeze(1)).squeeze(1)
        onehot = torch.zeros(R, Kc, dtype=torch.float64, device=DEV).scatter_(1, yr.unsqueeze(1), 1.0)
        grad = drow.double()[torch.arange(R, device=DEV) // rpg].unsqueeze(1) * (lsm.exp() - onehot)
        _CE[key] = dict(x=x, y=y, drow=drow, rpg=rpg, label_rows=label_rows, rows=rows, grad=grad)
    return _CE[key]


@pytest.mark.parametrize('R,Kc,scale', CE_CASES, ids=['%dx%d-s%d' % c for c in CE_CASES])
def test_ce(R, Kc, scale):
    """ce_kernel past one block (R = 257), at K = 1 (loss and gradient exactly zero) and K = 1024, logits scaled by 2 and by
    30; ce_bwd alone equals the fused gradient; dlogits = None leaves the rows' bits alone."""
    c = ce_case(R, Kc, scale)
    kw = dict(rows_per_group=c['rpg'], label_rows=c['label_rows'])
    rows, rows_flat = guarded(R)
    dl, dl_flat = guarded(R, Kc)
    K.ce_fwd(c['x'], c['y'], rows, drow=c['drow'], dlogits=dl, **kw)
    rows2, rows2_flat = guarded(R)
    K.ce_fwd(c['x'], c['y'], rows2, **kw)
    dl2, dl2_flat = guarded(R, Kc)
    K.ce_bwd(c['x'], c['y'], c['drow'], dl2, **kw)
    for v, f in ((rows, rows_flat), (dl, dl_flat), (rows2, rows2_flat), (dl2, dl2_flat)):
        assert guard_ok(v, f)
    assert torch.equal(rows, rows2), 'the rows with dlogits and without differ'
    assert torch.equal(dl, dl2) and not bool(torch.isnan(dl).any()), 'ce_bwd alone differs from the fused gradient'
    if Kc == 1:
        assert bool((c['rows'] == 0).all()) and bool((c['grad'] == 0).all())
        assert bool((rows == 0).all()) and bool((dl == 0).all())
        return
    check(dict(rows=elem_err(rows, c['rows']), dlogits=row_err(dl, c['grad'])), REL_TOL, 'ce %dx%d scale %g' % (R, Kc, scale))


def test_ce_flags_a_bad_label():
    """Labels -1 and K on the stand-alone entries: a NaN row and a NaN gradient row each, every other row finite (what
    test_linear_with_categorical_term_flags_a_bad_label asserts of the folded launch)."""
    R, Kc = 8, 10
    x = torch.randn(R, Kc, generator=gen(120), device=DEV) * 2
    y = torch.tensor([0, 3, 10, 9, -1, 2, 5, 7], device=DEV)
    bad = torch.tensor([False, False, True, False, True, False, False, False], device=DEV)
    rows, rows_flat = guarded(R)
    dl, dl_flat = guarded(R, Kc)
    K.ce_fwd(x, y, rows, drow=torch.ones(1, device=DEV), dlogits=dl)
    dl2, dl2_flat = guarded(R, Kc)
    K.ce_bwd(x, y, torch.ones(1, device=DEV), dl2)
    assert guard_ok(rows, rows_flat) and guard_ok(dl, dl_flat) and guard_ok(dl2, dl2_flat)
    assert torch.equal(torch.isnan(rows), bad)
    for d in (dl, dl2):
        assert torch.equal(torch.isnan(d).all(dim=1), bad) and bool(torch.isfinite(d[~bad]).all())
    assert torch.equal(dl[~bad], dl2[~bad])
    yr = y[~bad]
    lsm = torch.log_softmax(x[~bad].double() + 1e-6, dim=1)
    check(dict(rows=elem_err(rows[~bad], -lsm.gather(1, yr.unsqueeze(1)).squeeze(1))), REL_TOL, 'ce good rows beside bad labels')


# ============================================================================= group sums
def sum_rows(G, rpg, seed):
    """Positive rows (0.5 + rand) with their own scale per group."""
    return ((0.5 + torch.rand(G, rpg, generator=gen(seed), device=DEV))
            * (1 + torch.arange(G, device=DEV)).unsqueeze(1)).reshape(-1).contiguous()


@pytest.mark.parametrize('G', [1, 7])
@pytest.mark.parametrize('rpg', [1024, 1025, 3000])
def test_group_sums(rpg, G):
    """group_sums_kernel at one full trip of its 1024 threads, one element past it, and a ragged third trip; coef = None;
    either destination None (the other's bits unchanged); accumulate = the plain result + the pre-fill, bit for bit."""
    rows = sum_rows(G, rpg, 200 + rpg + G)
    coef = torch.tensor([0.5, 1e-3, 2.0, 1.0, 0.25, 3.0, 0.7][:G], device=DEV)
    sums = rows.double().reshape(G, rpg).sum(dim=1)
    out, out_flat = guarded(G)
    tot, tot_flat = guarded(1)
    K.group_sums(rows, coef, out, tot, G, rpg)
    ref = sums * coef.double()
    errs = dict(out=elem_err(out, ref), total=elem_err(tot, ref.sum().reshape(1)))
    out_n, out_n_flat = guarded(G)
    tot_n, tot_n_flat = guarded(1)
    K.group_sums(rows, None, out_n, tot_n, G, rpg)
    errs.update(out_nocoef=elem_err(out_n, sums), total_nocoef=elem_err(tot_n, sums.sum().reshape(1)))
    check(errs, REL_TOL, 'group_sums %d x %d' % (G, rpg))
    out_only, out_only_flat = guarded(G)
    K.group_sums(rows, coef, out_only, None, G, rpg)
    tot_only, tot_only_flat = guarded(1)
    K.group_sums(rows, coef, None, tot_only, G, rpg)
    assert torch.equal(out_only, out) and torch.equal(tot_only, tot)
    pre_out = 3 + torch.rand(G, generator=gen(1), device=DEV)
    pre_tot = -5 - torch.rand(1, generator=gen(2), device=DEV)
    acc_out, acc_out_flat = guarded(G)
    acc_tot, acc_tot_flat = guarded(1)
    acc_out.copy_(pre_out)
    acc_tot.copy_(pre_tot)
    K.group_sums(rows, coef, acc_out, acc_tot, G, rpg, accumulate=True)
    assert torch.equal(acc_out, pre_out + out) and torch.equal(acc_tot, pre_tot + tot)
    for v, f in ((out, out_flat), (tot, tot_flat), (out_n, out_n_flat), (tot_n, tot_n_flat), (out_only, out_only_flat),
                 (tot_only, tot_only_flat), (acc_out, acc_out_flat), (acc_tot, acc_tot_flat)):
        assert guard_ok(v, f)


# ============================================================================= the one-launch ELBO
def elbo_part(groups, rpg, first=0, coef=True, term_of=None, seed=0):
    """(rows, coef, term_of, first_term, groups, rows_per_group) as kernels.elbo_reduce takes it."""
    rows = sum_rows(groups, rpg, 300 + seed)
    cf = (0.25 + torch.rand(groups, generator=gen(400 + seed), device=DEV)) if coef else None
    return (rows, cf, term_of, first, groups, rpg)


def elbo_reference(parts, T):
    ref = torch.zeros(T + 1, dtype=torch.float64, device=DEV)
    for rows, cf, term_of, first, groups, rpg in parts:
        s = rows.double()[:groups * rpg].reshape(groups, rpg).sum(dim=1)
        if cf is not None:
            s = s * cf.double()
        term = term_of.long() if term_of is not None else first + torch.arange(groups, device=DEV)
        ref.index_add_(0, term, s)
        ref[T] += s.sum()
    return ref


def elbo_run(parts, T, zero=None, prepare=None):
    """-> (elbo [T + 1], counter after the launch).  prepare: (step_dev, coef2) -> mvae_elbo_reduce_prepare."""
    elbo, elbo_flat = guarded(T + 1)
    ctr = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    if prepare is None:
        K.elbo_reduce(parts, elbo, T, zero=zero, counter_dev=ctr, counter_inc=3)
    else:
        K.elbo_reduce_prepare(parts, elbo, T, prepare[0], 1, 1e-3, 0.9, 0.999, prepare[1], zero=zero, counter_dev=ctr,
                              counter_inc=3)
    assert guard_ok(elbo, elbo_flat), 'elbo written outside [0, T]'
    assert ctr.item() == 8, 'the counter advances by counter_inc, once'
    return elbo


def term_table(groups, T, seed):
    return torch.randint(0, T, (groups,), generator=gen(500 + seed), device=DEV).int()


def mixed_parts():
    """A spread part, a 21-group part of 70 rows (the round-robin turn of the 16 waves wraps), a 40-group part, and a table
    of ready sums with term_of and coef = None: 4 parts, 113 groups, T = 40."""
    return [elbo_part(2, L + 1, first=3, seed=10), elbo_part(21, 70, first=19, seed=11), elbo_part(40, 5, seed=12),
            elbo_part(50, 1, coef=False, term_of=term_table(50, 40, 13), seed=13)], 40


ELBO_CASES = {
    '513x3': lambda: ([elbo_part(3, 513, seed=1)], 3),                   # a second trip of lane_sum, one row in it
    'Lx3': lambda: ([elbo_part(3, L, seed=2)], 3),                       # the longest group one wave sums alone
    'L+1x3': lambda: ([elbo_part(3, L + 1, seed=3)], 3),                 # spread: waves 11..15 empty, wave 10 ragged
    '12800x3': lambda: ([elbo_part(3, 12800, seed=4)], 3),               # the MNIST batch-512 partials: 512 x 25
    '21x70': lambda: ([elbo_part(21, 70, seed=5)], 21),                  # more groups than waves, none spread
    'mixed': mixed_parts,
    '1024 groups': lambda: ([elbo_part(24, 37, first=8, seed=6),         # every thread of block 0 holds a group
                             elbo_part(1000, 1, term_of=term_table(1000, 40, 7), seed=7)], 40),
}


@pytest.mark.parametrize('case', sorted(ELBO_CASES))
def test_elbo_reduce(case):
    parts, T = ELBO_CASES[case]()
    spread = [p[5] > L for p in parts]
    assert any(spread) == (case in ('L+1x3', '12800x3', 'mixed'))
    ref = elbo_reference(parts, T)
    elbo = elbo_run(parts, T)
    check(dict(elbo=elem_err(elbo, ref), total=abs(elbo[T].item() - ref[T].item()) / ref[T].item()), REL_TOL,
          'elbo_reduce %s' % case)
    again = elbo_run(parts, T)
    assert torch.equal(elbo, again), 'two runs on the same inputs differ'


@pytest.mark.parametrize('case', ['513x3', 'Lx3', 'L+1x3', '12800x3'])
def test_elbo_every_row_counts(case):
    """One row of 12800 is 8e-5 of its group's sum: the bound above cannot see a row that a wave's stretch or a trip of
    lane_sum leaves out.  So: the first and the last row of every 64 rows of the last group (the ends of every stretch a
    wave or a trip can be given), one at a time, grows by 1000 x the group's scale, and the group's entry must move by
    coef x that -- judged relative to the step, at the same bound."""
    parts, T = ELBO_CASES[case]()
    rows, cf, _, _, groups, rpg = parts[0]
    base = elbo_run(parts, T)
    g = groups - 1
    step = 1000.0 * groups
    edges = sorted({0, rpg - 1} | {k for k in range(64, rpg, 64)} | {k - 1 for k in range(64, rpg, 64)})
    work = rows.clone()
    moved = []
    for i in edges:
        work[g * rpg + i] += step
        moved.append(elbo_run([(work,) + tuple(parts[0][1:])], T))
        work[g * rpg + i] = rows[g * rpg + i]
    assert torch.equal(work, rows)
    moved = torch.stack(moved).double()
    want = step * cf[g].double().item()
    err = ((moved[:, g] - base[g].double()) - want).abs().max().item() / want
    err_total = ((moved[:, T] - base[T].double()) - want).abs().max().item() / want
    others = (moved[:, :g] - base[:g].double()).abs().max().item()
    assert others == 0.0, 'a row of the last group moved another group'
    check(dict(step=err, step_total=err_total), REL_TOL, 'elbo_reduce %s, %d edge rows one at a time' % (case, len(edges)))


def test_elbo_mixes_up_no_groups():
    """Every term of the mixed launch on its own: a group that lands on the wrong term, or a spread group whose waves' sums
    are added to a neighbour's, moves single entries by far more than the bound."""
    parts, T = mixed_parts()
    ref = elbo_reference(parts, T)
    elbo = elbo_run(parts, T)
    rel = ((elbo.double() - ref).abs() / ref.abs().clamp_min(1e-30))
    assert bool((ref[:T] > 0).all())
    check(dict(worst_term=rel.max().item()), REL_TOL, 'elbo_reduce mixed, entry by entry')


@pytest.mark.parametrize('zero_n,off', [(4099, 1), (4099, 0), (1048583, 0), (3, 0)],
                         ids=['4099-unaligned', '4099', '1048583', '3'])
def test_elbo_zero_clear(zero_n, off):
    """The `zero` clear of every block: one float off 16 bytes (the one-element loop for everything, two blocks), 4099 (1024
    float4 stores and a 3-float tail), 1,048,583 (262,145 float4 stores on the 256-block cap: a second grid-stride trip of
    one store, then the tail), 3 (no float4 store at all).  Everything cleared, the guard bands untouched, the sums as
    without the clear."""
    parts, T = [elbo_part(3, 37, seed=20)], 3
    plain = elbo_run(parts, T)
    flat = torch.full((off + zero_n + GUARD,), SENTINEL, device=DEV)
    zero = flat[off:off + zero_n]
    zero.fill_(3.0)
    assert zero.data_ptr() % 16 == 4 * off
    elbo = elbo_run(parts, T, zero=zero)
    assert torch.equal(elbo, plain)
    assert int(torch.count_nonzero(zero).item()) == 0, 'not everything was cleared'
    assert guard_ok(zero, flat), 'the clear wrote outside zero[0, zero_n)'


@pytest.mark.parametrize('case', ['L+1x3', '21x70', 'mixed'])
def test_elbo_reduce_prepare_where_wave_15_has_sums_of_its_own(case):
    """mvae_elbo_reduce_prepare on a spread part and on more than 16 groups (the last thread of block 0 does Adam's
    bookkeeping, then its wave's sums): the ELBO bits of mvae_elbo_reduce, step and coefficients those of
    mvae_adam_prepare."""
    parts, T = ELBO_CASES[case]()
    want = elbo_run(parts, T)
    for start in (0, 999):
        step_w = torch.full((1,), start, dtype=torch.int64, device=DEV)
        coef_w = torch.full((2,), NAN, device=DEV)
        K.adam_prepare(step_w, 1, 1e-3, 0.9, 0.999, coef_w)
        step_g = torch.full((1,), start, dtype=torch.int64, device=DEV)
        coef_g, coef_flat = guarded(2)
        got = elbo_run(parts, T, prepare=(step_g, coef_g))
        assert torch.equal(got, want) and not bool(torch.isnan(got).any())
        assert step_g.item() == step_w.item() == start + 1
        assert torch.equal(coef_g, coef_w) and not bool(torch.isnan(coef_g).any())
        assert guard_ok(coef_g, coef_flat)
    check(dict(elbo=elem_err(got, elbo_reference(parts, T))), REL_TOL, 'elbo_reduce_prepare %s' % case)


# ============================================================================= elementwise BCE (misc.hip)
_ELEM = {}


def elem_case(n):
    if n not in _ELEM:
        g = gen(600 + n % 1000)
        x = torch.randn(n, generator=g, device=DEV) * 3
        t = torch.rand(n, generator=g, device=DEV)
        go = torch.randn(n, generator=g, device=DEV)
        assert bool((x != 0).all())
        xd, td, gd = x.double(), t.double(), go.double()
        _ELEM[n] = dict(x=x, t=t, g=go, out=torch.clamp(xd, min=0) - xd * td + torch.log1p(torch.exp(-xd.abs())),
                        dx=gd * (torch.sigmoid(xd) - td), dt=-gd * xd)
    return _ELEM[n]


@pytest.mark.parametrize('n', [1, 257, 8192 * 256 + 5], ids=['1', '257', 'past-the-grid-cap'])
def test_bce_elem(n):
    """mvae_bce_elem_fwd / _bwd at one element, a ragged second block, and 5 elements past 8192 blocks of 256 (the grid
    stride); dx only, dt only, both -- the same bits."""
    c = elem_case(n)
    out, out_flat = guarded(n)
    K.bce_elem_fwd(c['x'], c['t'], out)
    dx, dx_flat = guarded(n)
    dt, dt_flat = guarded(n)
    K.bce_elem_bwd(c['x'], c['t'], c['g'], dx, dt)
    dx1, dx1_flat = guarded(n)
    K.bce_elem_bwd(c['x'], c['t'], c['g'], dx1, None)
    dt1, dt1_flat = guarded(n)
    K.bce_elem_bwd(c['x'], c['t'], c['g'], None, dt1)
    for v, f in ((out, out_flat), (dx, dx_flat), (dt, dt_flat), (dx1, dx1_flat), (dt1, dt1_flat)):
        assert guard_ok(v, f)
    assert torch.equal(dx1, dx) and torch.equal(dt1, dt)
    check(dict(out=elem_err(out, c['out']), dx=elem_err(dx, c['dx']), dt=elem_err(dt, c['dt'])), REL_TOL, 'bce_elem n=%d' % n)
