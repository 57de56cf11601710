"""GPU: the segmented BCE-with-logits row sums (csrc/loss_multi.hip, mvae_bce_multi_fwd / _bwd) against a float64
evaluation of the same formula on the CPU:

    rowsum[r]        = sum_s weight_s * sum_p bce(logits_s[r, p], target_s[r % target_rows, p])
    dlogits_s[r, p]  = drow[r / rows_per_group] * weight_s * (sigmoid(x) - t)

Bar: util.REL_TOL (1e-4 of max |ref|).  Shapes: one full chunk (P = 4096), the vision step's six segments (rows of
49,152 elements: twelve chunks, three per colour segment), the scalar path (P % 4 != 0: P = 5, 1030, 3 inside one
chunk, P = 4099 and 8190 across a chunk boundary), views 4 bytes off an aligned buffer, ragged float4 tails; R = 1, 3 and
21 = 7 groups x 3 with rows_per_group = target_rows = 3.  Every dlogits is followed by a guard band that must stay
untouched."""
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import kernels as K
from util import REL_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD, SENTINEL = 64, -77.0
VISION_P = (12288, 4096, 4096, 4096, 12288, 12288)


def _buffer(rows, P, offset, fill=None, generator=None, scale=1.0):
    """A [rows, P] device view, 4 bytes past a 16-byte boundary when ``offset``, followed by a guard band; returns
    (view, the whole flat buffer)."""
    off = 1 if offset else 0
    flat = torch.full((off + rows * P + GUARD,), SENTINEL, dtype=torch.float32)
    if fill is not None:
        flat[off:off + rows * P] = fill(rows * P, generator) * scale
    flat = flat.to(DEV)
    view = flat[off:off + rows * P].view(rows, P)
    assert view.data_ptr() % 16 == (4 if offset else 0)
    return view, flat


def _randn(n, g):
    return torch.randn(n, generator=g)


def _rand(n, g):
    return torch.rand(n, generator=g)


def make_case(Ps, R, weights, offset=False, seed=0):
    rpg = trows = 3 if R % 3 == 0 else 1
    g = torch.Generator().manual_seed(1000 + seed + R)
    segs = []
    for P, w in zip(Ps, weights):
        x, _ = _buffer(R, P, offset, _randn, g, scale=3.0)
        t, _ = _buffer(trows, P, offset, _rand, g)
        d, dflat = _buffer(R, P, offset)
        segs.append({'x': x, 't': t, 'd': d, 'dflat': dflat, 'w': w, 'P': P})
    drow = torch.randn(R // rpg, generator=g).to(DEV)
    return segs, drow, rpg, trows


def reference(segs, drow, rpg, trows):
    R = segs[0]['x'].shape[0]
    rows = torch.zeros(R, dtype=torch.float64)
    grads = []
    dr = drow.double().cpu().repeat_interleave(rpg).unsqueeze(1)
    for s in segs:
        x = s['x'].double().cpu()
        t = s['t'].double().cpu().repeat(R // trows, 1)
        rows += s['w'] * (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum(dim=1)
        grads.append(dr * s['w'] * (torch.sigmoid(x) - t))
    return rows, grads


def table(segs, with_grad=True, skip=None):
    return [(s['x'], s['t'], s['d'] if (with_grad and i != skip) else None, s['w']) for i, s in enumerate(segs)]


def guards_untouched(segs):
    for i, s in enumerate(segs):
        n = s['d'].numel()
        off = (s['d'].data_ptr() - s['dflat'].data_ptr()) // 4
        assert bool((s['dflat'][:off] == SENTINEL).all()) and bool((s['dflat'][off + n:] == SENTINEL).all()), \
            'segment %d: bytes outside dlogits were written' % i


CASES = {
    'one_full_chunk': ((4096,), (1.0,), False),
    'vision_six': (VISION_P, (1.0 / 6,) * 6, False),
    'scalar_path': ((5, 1030, 3), (1.0, 1.0, 1.0), False),
    'scalar_across_chunks': ((4099, 8190), (0.5, 2.0), False),
    'offset_views': ((4096, 8200, 64), (1.0, 1.0, 1.0), True),
    'non_unit_weights': ((4096, 260, 12288), (0.25, -1.5, 3.0), False),
}


@pytest.mark.parametrize('R', [1, 3, 21])
@pytest.mark.parametrize('case', sorted(CASES))
def test_forward_with_fused_gradient_matches_float64(case, R):
    Ps, weights, offset = CASES[case]
    segs, drow, rpg, trows = make_case(Ps, R, weights, offset, seed=sorted(CASES).index(case))
    ref_rows, ref_grads = reference(segs, drow, rpg, trows)
    rows = torch.full((R + GUARD,), SENTINEL, device=DEV)
    K.bce_multi_fwd(table(segs), rows[:R], drow=drow, rows_per_group=rpg)
    torch.cuda.synchronize()
    e = assert_close(rows[:R], ref_rows, 'row sums')
    assert bool((rows[R:] == SENTINEL).all()), 'row sums written past R'
    for s, ref in zip(segs, ref_grads):
        e = max(e, assert_close(s['d'], ref, 'dlogits P=%d' % s['P']))
    guards_untouched(segs)
    print('%s R=%d: worst rel err %.2e (bar %.0e)' % (case, R, e, REL_TOL))


def test_two_forward_runs_are_bit_equal_and_bwd_alone_equals_the_fused_gradient():
    segs, drow, rpg, trows = make_case(VISION_P, 21, (1.0 / 6,) * 6, seed=7)
    rows_a, rows_b = torch.empty(21, device=DEV), torch.empty(21, device=DEV)
    K.bce_multi_fwd(table(segs), rows_a, drow=drow, rows_per_group=rpg)
    fused = [s['d'].clone() for s in segs]
    for s in segs:
        s['d'].fill_(SENTINEL)
    K.bce_multi_fwd(table(segs, with_grad=False), rows_b, rows_per_group=rpg)
    assert torch.equal(rows_a, rows_b), 'two runs on the same inputs differ'
    assert all(bool((s['d'] == SENTINEL).all()) for s in segs), 'a forward without dlogits wrote a gradient'
    K.bce_multi_bwd(table(segs), drow, rows_per_group=rpg)
    for s, f in zip(segs, fused):
        assert torch.equal(s['d'], f), 'bwd alone differs from the fused gradient (P=%d)' % s['P']
    guards_untouched(segs)


def test_segment_without_dlogits_and_forward_without_drow():
    segs, drow, rpg, trows = make_case((4096, 1030, 8192), 21, (1.0, 2.0, 0.5), seed=8)
    ref_rows, ref_grads = reference(segs, drow, rpg, trows)
    rows = torch.empty(21, device=DEV)
    K.bce_multi_fwd(table(segs, skip=1), rows, drow=drow, rows_per_group=rpg)       # segment 1: dlogits = NULL
    assert_close(rows, ref_rows, 'row sums')
    assert bool((segs[1]['dflat'] == SENTINEL).all()), 'the segment without dlogits was written'
    for i in (0, 2):
        assert_close(segs[i]['d'], ref_grads[i], 'dlogits %d' % i)
    K.bce_multi_bwd(table(segs, skip=0), drow, rows_per_group=rpg)                  # gradient only, segment 0 skipped
    assert_close(segs[1]['d'], ref_grads[1], 'dlogits 1 (bwd)')
    guards_untouched(segs)
    for s in segs:
        s['d'].fill_(SENTINEL)
    rows2 = torch.empty(21, device=DEV)
    K.bce_multi_fwd(table(segs), rows2, drow=None, rows_per_group=rpg)              # drow_dev = NULL: no gradient
    assert torch.equal(rows2, rows)
    assert all(bool((s['dflat'] == SENTINEL).all()) for s in segs), 'a forward without drow wrote a gradient'


def test_equals_six_single_launches_summed():
    segs, drow, rpg, trows = make_case(VISION_P, 21, (1.0 / 6,) * 6, seed=9)
    rows = torch.empty(21, device=DEV)
    K.bce_multi_fwd(table(segs), rows, drow=drow, rows_per_group=rpg)
    total = torch.zeros(21, dtype=torch.float64)
    for s in segs:
        one = torch.empty(21, device=DEV)
        d = torch.empty_like(s['x'])
        K.bce_rowsum_fwd(s['x'].contiguous(), s['t'].contiguous(), one, drow=drow, dlogits=d, rows_per_group=rpg,
                         target_rows=trows)
        total += s['w'] * one.double().cpu()
        assert_close(s['d'], s['w'] * d.double().cpu(), 'dlogits vs mvae_bce_rowsum_fwd (P=%d)' % s['P'])
    assert_close(rows, total, 'row sums vs six mvae_bce_rowsum_fwd launches')
