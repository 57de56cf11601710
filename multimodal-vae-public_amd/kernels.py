"""Tensor-level launchers over the C ABI (one python function per ``mvae_*`` entry point).

Everything here is enqueue-only on ``torch.cuda.current_stream()``: no host sync, no
allocation other than the cached scratch buffer, so a whole train step can be captured into
a hipGraph (``torch.cuda.CUDAGraph``).  PyTorch is used for device memory and streams only.
Tensors must live on the GPU, be fp32 (labels int64) and contiguous unless noted.
"""
import ctypes

import torch

from . import _lib
from ._lib import ACCUMULATE, ACT_SWISH, check

_WS = {}          # device index -> list of scratch tensors (old ones kept alive for captured graphs)
_WS_MIN_BYTES = 64 << 20


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('multimodal-vae-public_amd: the HIP path needs GPU tensors (got %s); '
                               'there is no CPU fallback' % t.device)


def _f32c(*tensors):
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError('expected a contiguous float32 tensor, got %s %s contiguous=%s'
                               % (t.dtype, tuple(t.shape), t.is_contiguous()))


def workspace(nbytes, device):
    """Scratch for split reductions.  Grows by allocating a new buffer; earlier buffers stay
    alive because captured graphs may hold their addresses."""
    # one scratch per (device, stream): engine branches on different streams run concurrently
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    bufs = _WS.setdefault(key, [])
    if not bufs or bufs[-1].numel() * 4 < nbytes:
        n = max(int(nbytes), _WS_MIN_BYTES)
        bufs.append(torch.empty((n + 3) // 4, dtype=torch.float32, device=device))
    return bufs[-1]


def _ws_args(nbytes, device):
    ws = workspace(nbytes, device)
    return _ptr(ws), ctypes.c_size_t(ws.numel() * 4)


# ---------------------------------------------------------------------------- Linear
def linear_fwd(x, w, bias, pre=None, act=None, mask=None, mask_scale=1.0, ldx=None, ldy=None):
    """pre[M,N] = x.w^T + b ; act = swish(pre) * mask*scale.  x may be a row-strided view (ldx)."""
    _need_gpu(x, w, bias, pre, act, mask)
    M, K = x.shape
    N = w.shape[0]
    ldx = ldx if ldx is not None else x.stride(0)
    out = pre if pre is not None else act
    ldy = ldy if ldy is not None else out.stride(0)
    ws, wsb = _ws_args(_lib.lib().mvae_gemm_ws_bytes(M, N, K), x.device)
    check(_lib.lib().mvae_linear_fwd(_ptr(x), ldx, _ptr(w), _ptr(bias), _ptr(pre), _ptr(act), ldy,
                                     _ptr(mask), mask_scale, M, N, K, ws, wsb, _stream()), 'mvae_linear_fwd')


def bce_partials(N):
    """Partial sums per row that ``linear_bce_fwd`` writes for N columns."""
    return (N + 31) // 32


def linear_bce_fwd(x, w, bias, target, drow, dlogits, partial, rows_per_group, target_rows, logits=None):
    """Last Linear of a decoder + its Bernoulli term: dlogits[M,N] and partial[M, bce_partials(N)] (a row's
    term = the sum of its partials); the logits are stored only when ``logits`` is given."""
    _need_gpu(x, w, bias, target, drow, dlogits, partial, logits)
    M, K = x.shape
    N = w.shape[0]
    if target.dim() != 2 or target.stride(1) != 1 or target.shape[1] != N or target.shape[0] < target_rows:
        raise RuntimeError('target must be [>= target_rows, N] with unit column stride')
    if partial.numel() < M * bce_partials(N) or not partial.is_contiguous():
        raise RuntimeError('partial must hold M * ceil(N / 32) floats')
    if logits is not None and logits.stride() != dlogits.stride():
        raise RuntimeError('logits and dlogits must share a layout')
    check(_lib.lib().mvae_linear_bce_fwd(_ptr(x), x.stride(0), _ptr(w), _ptr(bias), _ptr(target), target_rows,
                                         target.stride(0), _ptr(drow), rows_per_group, _ptr(dlogits),
                                         dlogits.stride(0), _ptr(logits), _ptr(partial), M, N, K, _stream()),
          'mvae_linear_bce_fwd')


def linear_ce_fwd(x, w, bias, label, drow, dlogits, row, rows_per_group, label_rows, logits=None):
    """Last Linear of a decoder (N <= 32 classes) + its categorical term: row[M] and dlogits[M,N]."""
    _need_gpu(x, w, bias, label, drow, dlogits, row, logits)
    M, K = x.shape
    N = w.shape[0]
    if label.dtype != torch.int64 or not label.is_contiguous() or label.numel() < label_rows:
        raise RuntimeError('label must be a contiguous int64 vector of at least label_rows entries')
    if logits is not None and logits.stride() != dlogits.stride():
        raise RuntimeError('logits and dlogits must share a layout')
    check(_lib.lib().mvae_linear_ce_fwd(_ptr(x), x.stride(0), _ptr(w), _ptr(bias), _ptr(label), label_rows,
                                        _ptr(drow), rows_per_group, _ptr(dlogits), dlogits.stride(0), _ptr(logits),
                                        _ptr(row), M, N, K, _stream()), 'mvae_linear_ce_fwd')


def linear_dgrad(dy, w, dx, pre_in=None, mask=None, mask_scale=1.0, accumulate=False):
    _need_gpu(dy, w, dx, pre_in, mask)
    M, N = dy.shape
    K = w.shape[1]
    ws, wsb = _ws_args(_lib.lib().mvae_gemm_ws_bytes(M, K, N), dy.device)
    check(_lib.lib().mvae_linear_dgrad(_ptr(dy), dy.stride(0), _ptr(w), _ptr(dx), dx.stride(0),
                                       _ptr(pre_in), _ptr(mask), mask_scale, M, N, K,
                                       ACCUMULATE if accumulate else 0, ws, wsb, _stream()), 'mvae_linear_dgrad')


def linear_wgrad(dy, x, dw, db=None, accumulate=False):
    _need_gpu(dy, x, dw, db)
    M, N = dy.shape
    K = x.shape[1]
    nbytes = _lib.lib().mvae_gemm_ws_bytes(N, K, M)
    ws, wsb = _ws_args(nbytes, dy.device)
    check(_lib.lib().mvae_linear_wgrad(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dw), _ptr(db),
                                       M, N, K, ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_linear_wgrad')


def wgrad_batchable(dy, x):
    """Whether mvae_linear_wgrad_batched takes this problem (see include/mvae_hip.h)."""
    M, N = dy.shape
    K = x.shape[1]
    tiles = ((N + 31) // 32) * ((K + 31) // 32)
    return (tiles <= 2048 and M <= 4096 and M * dy.stride(0) * 4 < (1 << 32) and M * x.stride(0) * 4 < (1 << 32)
            and dy.stride(1) == 1 and x.stride(1) == 1)


def linear_wgrad_batched(items, adam=None):
    """items: [(dy[M,N], x[M,K], dw[N,K], db[N] or None, accumulate)] -- the weight gradients of several Linear
    layers in ONE launch (mvae_linear_wgrad_batched); more than WGRAD_BATCH_MAX items go out in several.
    ``adam`` (an ``_lib.AdamFuse``, see ``optim.FusedAdam.fuse_record``): the launch also applies Adam to the
    parameters behind these gradients (mvae_linear_wgrad_batched_adam); an item (None, None, g, None, False) is a
    finished flat gradient that only takes the update."""
    items = list(items)
    for lo in range(0, len(items), _lib.WGRAD_BATCH_MAX):
        chunk = items[lo:lo + _lib.WGRAD_BATCH_MAX]
        arr = (_lib.WgradItem * len(chunk))()
        for q, (dy, x, dw, db, acc) in enumerate(chunk):
            if dy is None:
                if adam is None:
                    raise RuntimeError('update-only items need adam=')
                _need_gpu(dw); _f32c(dw)
                arr[q] = _lib.WgradItem(None, 0, None, 0, _ptr(dw), None, 0, 0, dw.numel(), 0)
                continue
            _need_gpu(dy, x, dw, db); _f32c(dw, db)
            M, N = dy.shape
            if x.shape[0] != M or tuple(dw.shape) != (N, x.shape[1]):
                raise RuntimeError('wgrad item %d: shapes %s %s %s' % (q, tuple(dy.shape), tuple(x.shape), tuple(dw.shape)))
            arr[q] = _lib.WgradItem(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dw), _ptr(db), M, N,
                                    x.shape[1], ACCUMULATE if acc else 0)
        if adam is not None:
            check(_lib.lib().mvae_linear_wgrad_batched_adam(arr, len(chunk), ctypes.byref(adam), _stream()),
                  'mvae_linear_wgrad_batched_adam')
        else:
            check(_lib.lib().mvae_linear_wgrad_batched(arr, len(chunk), _stream()), 'mvae_linear_wgrad_batched')


def linear_route(op, M, N, K, G=1, ld_a=None, ld_b=None, gs_a=None, gs_b=None, aligned=True, form='other', db=False,
                 ws_bytes=None):
    """(route, splits, finish) of the Linear launch ``op`` (a key of ``_lib.LINEAR_OPS``) on M rows, N output and K input
    features -- the name of the kernel instantiation it takes (``_lib.LINEAR_ROUTES``), the number of partials of a split
    reduction (1: none) and the launch that sums them (``_lib.LINEAR_FINISH``, None: none).  Host only
    (mvae_linear_route: the route function the launch itself switches on).  ``ld_a``, ``ld_b``: the launch's two leading
    dimensions in the order of its argument list (default: dense); ``gs_a``, ``gs_b``: the group strides of its two input
    operands (default: dense [G, rows, width] activations, dense weights); ``aligned``: the input operands are 16-byte
    aligned; ``form`` (forward): 'pre+act', 'act' (no mask) or 'other'; ``db`` (weight gradient): with a bias gradient;
    ``ws_bytes``: the scratch the launch gets, by default what the wrappers here pass before anything asked for more
    (``_WS_MIN_BYTES``), 0 for none.  Raises where the launch would refuse the arguments."""
    dense = {'fwd': (K, N, M * K, N * K), 'bce_fwd': (K, N, 0, 0), 'ce_fwd': (K, N, 0, 0),
             'dgrad': (N, K, M * N, N * K), 'wgrad': (N, K, M * N, M * K)}[op]
    ld_a, ld_b, gs_a, gs_b = (d if v is None else v for v, d in zip((ld_a, ld_b, gs_a, gs_b), dense))
    sp, fin = ctypes.c_int(1), ctypes.c_int(0)
    rc = _lib.lib().mvae_linear_route(_lib.LINEAR_OPS[op], G, M, N, K, ld_a, ld_b, gs_a, gs_b, 1 if aligned else 0,
                                      _lib.LINEAR_FORMS[form], 1 if db else 0,
                                      _WS_MIN_BYTES if ws_bytes is None else int(ws_bytes), ctypes.byref(sp),
                                      ctypes.byref(fin))
    if rc <= 0:
        check(rc if rc < 0 else -1, 'mvae_linear_route')
    return _lib.LINEAR_ROUTES[rc], sp.value, _lib.LINEAR_FINISH[fin.value]


def linear_wgrad_batched_route(items, adam=False):
    """(route, (tile rows, tile columns), waves per tile) of one batched weight-gradient launch.  ``items``: tensors as for
    ``linear_wgrad_batched`` (on any device: nothing is read), or plain (M, N, K, lddy, ldx, with_db, accumulate) tuples;
    at most WGRAD_BATCH_MAX of them.  Host only (mvae_linear_wgrad_batched_route).  Raises where the launch would refuse
    the table."""
    items = list(items)
    arr = (_lib.WgradItem * max(len(items), 1))()
    for q, it in enumerate(items):
        if len(it) == 7:      # stand-in pointers: distinct, 16-byte aligned, never dereferenced
            M, N, K, lddy, ldx, with_db, acc = it
            base = (q + 1) << 24
            arr[q] = _lib.WgradItem(base, lddy, base + 16, ldx, base + 32, base + 48 if with_db else None, M, N, K,
                                    ACCUMULATE if acc else 0)
        else:
            dy, x, dw, db, acc = it
            if dy is None:
                arr[q] = _lib.WgradItem(None, 0, None, 0, _ptr(dw), None, 0, 0, dw.numel(), 0)
            else:
                arr[q] = _lib.WgradItem(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dw), _ptr(db), dy.shape[0],
                                        dy.shape[1], x.shape[1], ACCUMULATE if acc else 0)
    tm, tn, kw = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mvae_linear_wgrad_batched_route(arr, len(items), 1 if adam else 0, ctypes.byref(tm), ctypes.byref(tn),
                                                    ctypes.byref(kw))
    if rc <= 0:
        check(rc if rc < 0 else -1, 'mvae_linear_wgrad_batched_route')
    return _lib.LINEAR_ROUTES[rc], (tm.value, tn.value), kw.value


# ---------------------------------------------------------------------------- grouped Linear
# G problems of one shape per launch: activations are [G, rows, width] tensors, parameters are
# (tensor of group 0, stride in floats to the same tensor of the next group) -- the experts' slices
# of the parameter arena.
def _g3(t, name):
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) < t.shape[1] * t.stride(1):
        raise RuntimeError('%s must be a [groups, rows, width] tensor with unit column stride' % name)
    return t


def linear_fwd_grouped(x, w0, w_gs, b0, b_gs, pre=None, act=None):
    _need_gpu(x, w0, b0, pre, act)
    G, M, K = _g3(x, 'x').shape
    N = w0.shape[0]
    out = _g3(pre if pre is not None else act, 'output')
    if pre is not None and act is not None and (act.stride() != pre.stride()):
        raise RuntimeError('pre and act must share a layout')
    ws, wsb = _ws_args(G * _lib.lib().mvae_gemm_ws_bytes(M, N, K), x.device)
    check(_lib.lib().mvae_linear_fwd_grouped(_ptr(x), x.stride(1), x.stride(0), _ptr(w0), w_gs, _ptr(b0), b_gs,
                                             _ptr(pre), _ptr(act), out.stride(1), out.stride(0), G, M, N, K,
                                             ws, wsb, _stream()), 'mvae_linear_fwd_grouped')


def linear_fwd_grouped_shared(x, G, w0, w_gs, b0, b_gs, pre=None, act=None):
    """``linear_fwd_grouped`` for G groups that all read the SAME input ``x`` [rows, width] (unit column stride): the
    group stride of x is 0, which is what a single group already passes -- every loader of the grouped forward forms
    ``x + group * stride`` and only reads through it.  The outputs are [G, rows, N] as usual.  (The first layer of
    celeba19's attribute decoders on one batch of z.)"""
    _need_gpu(x, w0, b0, pre, act)
    M, K = _rows2d(x, 'x').shape
    N = w0.shape[0]
    out = _g3(pre if pre is not None else act, 'output')
    if out.shape[0] != int(G) or out.shape[1] != M or out.shape[2] != N:
        raise RuntimeError('output must be [%d, %d, %d], got %s' % (G, M, N, tuple(out.shape)))
    if pre is not None and act is not None and (act.stride() != pre.stride()):
        raise RuntimeError('pre and act must share a layout')
    ws, wsb = _ws_args(int(G) * _lib.lib().mvae_gemm_ws_bytes(M, N, K), x.device)
    check(_lib.lib().mvae_linear_fwd_grouped(_ptr(x), x.stride(0), 0, _ptr(w0), w_gs, _ptr(b0), b_gs, _ptr(pre), _ptr(act),
                                             out.stride(1), out.stride(0), int(G), M, N, K, ws, wsb, _stream()),
          'mvae_linear_fwd_grouped')


def linear_dgrad_grouped(dy, w0, w_gs, dx, pre_in=None, accumulate=False):
    _need_gpu(dy, w0, dx, pre_in)
    G, M, N = _g3(dy, 'dy').shape
    K = w0.shape[1]
    _g3(dx, 'dx')
    if pre_in is not None and (not pre_in.is_contiguous() or pre_in.shape != (G, M, K)):
        raise RuntimeError('pre_in must be a contiguous [G, M, K] tensor')
    ws, wsb = _ws_args(G * _lib.lib().mvae_gemm_ws_bytes(M, K, N), dy.device)
    check(_lib.lib().mvae_linear_dgrad_grouped(_ptr(dy), dy.stride(1), dy.stride(0), _ptr(w0), w_gs, _ptr(dx),
                                               dx.stride(1), dx.stride(0), _ptr(pre_in), M * K, G, M, N, K,
                                               ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_linear_dgrad_grouped')


def linear_wgrad_grouped(dy, x, dw0, dw_gs, db0=None, db_gs=0, accumulate=False):
    _need_gpu(dy, x, dw0, db0)
    G, M, N = _g3(dy, 'dy').shape
    K = _g3(x, 'x').shape[2]
    ws, wsb = _ws_args(G * _lib.lib().mvae_gemm_ws_bytes(N, K, M), dy.device)
    check(_lib.lib().mvae_linear_wgrad_grouped(_ptr(dy), dy.stride(1), dy.stride(0), _ptr(x), x.stride(1),
                                               x.stride(0), _ptr(dw0), dw_gs, _ptr(db0), db_gs, G, M, N, K,
                                               ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_linear_wgrad_grouped')


# ---- pairs: two same-shaped Linear problems anywhere in memory as ONE grouped launch (G = 2); the group
#      stride is the pointer difference modulo 2^64.  MNIST's image and text decoders share their first
#      three layer shapes (mnist/model.py:96-104,137-145): pairing them halves those launches.
_U64 = (1 << 64) - 1


def _pair_stride(a, what):
    a0, a1 = a
    if (a0 is None) != (a1 is None):
        raise RuntimeError('%s: both or neither of a pair' % what)
    if a0 is None:
        return 0
    if a0.shape != a1.shape or a0.stride() != a1.stride() or a0.dtype != torch.float32 or a1.dtype != torch.float32:
        raise RuntimeError('%s: the two problems of a pair must share shape, strides and dtype' % what)
    d = a1.data_ptr() - a0.data_ptr()
    if d % 4:
        raise RuntimeError('%s: misaligned pair' % what)
    return (d // 4) & _U64


def _rows2d(t, what):
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError('%s must be [rows, width] with unit column stride' % what)
    return t


def linear_fwd_pair(x, w, b, pre, act):
    """(x0, x1), (w0, w1), (b0, b1), (pre0, pre1), (act0, act1): pre_g = x_g.w_g^T + b_g, act = swish."""
    _need_gpu(*x, *w, *b, *pre, *act)
    M, K = _rows2d(x[0], 'x').shape
    N = w[0].shape[0]
    out = pre if pre[0] is not None else act
    if pre[0] is not None and act[0] is not None and pre[0].stride() != act[0].stride():
        raise RuntimeError('pre and act must share a layout')
    if _pair_stride(pre, 'pre') != _pair_stride(act, 'act') and pre[0] is not None and act[0] is not None:
        raise RuntimeError('pre and act pairs must be laid out alike')
    ws, wsb = _ws_args(2 * _lib.lib().mvae_gemm_ws_bytes(M, N, K), x[0].device)
    check(_lib.lib().mvae_linear_fwd_grouped(_ptr(x[0]), x[0].stride(0), _pair_stride(x, 'x'), _ptr(w[0]),
                                             _pair_stride(w, 'w'), _ptr(b[0]), _pair_stride(b, 'bias'),
                                             _ptr(pre[0]), _ptr(act[0]), _rows2d(out[0], 'out').stride(0),
                                             _pair_stride(out, 'out'), 2, M, N, K, ws, wsb, _stream()),
          'mvae_linear_fwd_grouped')


def linear_dgrad_pair(dy, w, dx, pre_in=(None, None), accumulate=False):
    _need_gpu(*dy, *w, *dx, *pre_in)
    M, N = _rows2d(dy[0], 'dy').shape
    K = w[0].shape[1]
    if pre_in[0] is not None and not (pre_in[0].is_contiguous() and pre_in[0].shape == (M, K)):
        raise RuntimeError('pre_in must be contiguous [M, K]')
    ws, wsb = _ws_args(2 * _lib.lib().mvae_gemm_ws_bytes(M, K, N), dy[0].device)
    check(_lib.lib().mvae_linear_dgrad_grouped(_ptr(dy[0]), dy[0].stride(0), _pair_stride(dy, 'dy'), _ptr(w[0]),
                                               _pair_stride(w, 'w'), _ptr(dx[0]), _rows2d(dx[0], 'dx').stride(0),
                                               _pair_stride(dx, 'dx'), _ptr(pre_in[0]), _pair_stride(pre_in, 'pre_in'),
                                               2, M, N, K, ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_linear_dgrad_grouped')


def linear_wgrad_pair(dy, x, dw, db=(None, None), accumulate=False):
    _need_gpu(*dy, *x, *dw, *db)
    M, N = _rows2d(dy[0], 'dy').shape
    K = _rows2d(x[0], 'x').shape[1]
    ws, wsb = _ws_args(2 * _lib.lib().mvae_gemm_ws_bytes(N, K, M), dy[0].device)
    check(_lib.lib().mvae_linear_wgrad_grouped(_ptr(dy[0]), dy[0].stride(0), _pair_stride(dy, 'dy'), _ptr(x[0]),
                                               x[0].stride(0), _pair_stride(x, 'x'), _ptr(dw[0]),
                                               _pair_stride(dw, 'dw'), _ptr(db[0]), _pair_stride(db, 'db'), 2, M, N, K,
                                               ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_linear_wgrad_grouped')


def embedding_swish_fwd_grouped(idx, w0, w_gs, act):
    """idx: float [R, G] ({0,1} columns, celeba19's attrs); act [G, R, width] contiguous."""
    _need_gpu(idx, w0, act)
    if idx.dtype != torch.float32 or idx.dim() != 2 or idx.stride(1) != 1 or not act.is_contiguous():
        raise RuntimeError('grouped embedding wants a float [rows, groups] index and a contiguous output')
    R, G = idx.shape
    check(_lib.lib().mvae_embedding_swish_fwd_grouped(_ptr(idx), idx.stride(0), 1, _ptr(w0), w_gs, _ptr(act),
                                                      act.stride(0), G, R, w0.shape[0], w0.shape[1], _stream()),
          'mvae_embedding_swish_fwd_grouped')


def embedding_swish_bwd_grouped(idx, w0, w_gs, dact, dw0, accumulate=False):
    _need_gpu(idx, w0, dact, dw0)
    if idx.dtype != torch.float32 or idx.dim() != 2 or idx.stride(1) != 1 or not dact.is_contiguous():
        raise RuntimeError('grouped embedding wants a float [rows, groups] index and a contiguous gradient')
    R, G = idx.shape
    check(_lib.lib().mvae_embedding_swish_bwd_grouped(_ptr(idx), idx.stride(0), 1, _ptr(w0), w_gs, _ptr(dact),
                                                      dact.stride(0), _ptr(dw0), G, R, w0.shape[0], w0.shape[1],
                                                      ACCUMULATE if accumulate else 0, _stream()),
          'mvae_embedding_swish_bwd_grouped')


# ---------------------------------------------------------------------------- Conv 4x4
def _conv_call(name, a, b, c, d, B, Cin, H, W, Cout, stride, pad, repack=False, wr=None):
    if repack and wr is not None:       # the caller made the repacked copy already (conv_repack_batched): w = NULL
        _need_gpu(wr); _f32c(wr)
        check(getattr(_lib.lib(), name)(_ptr(a), None, _ptr(c), _ptr(d), B, Cin, H, W, Cout, stride, pad,
                                        _ptr(wr), wr.numel() * 4, _stream()), name)
    elif repack:    # dgrad-form launches repack the weights (Cout*Cin*16 floats) into scratch first
        ws, wsb = _ws_args(Cout * Cin * 16 * 4, a.device)
        check(getattr(_lib.lib(), name)(_ptr(a), _ptr(b), _ptr(c), _ptr(d), B, Cin, H, W, Cout, stride, pad,
                                        ws, wsb, _stream()), name)
    else:
        check(getattr(_lib.lib(), name)(_ptr(a), _ptr(b), _ptr(c), _ptr(d), B, Cin, H, W, Cout, stride, pad,
                                        _stream()), name)


def conv2d_fwd(x, w, pre, act, stride, pad):
    _need_gpu(x, w, pre, act); _f32c(x, w, pre, act)
    B, Cin, H, W = x.shape
    _conv_call('mvae_conv2d_k4_fwd', x, w, pre, act, B, Cin, H, W, w.shape[0], stride, pad)


def conv2d_dgrad(dy, w, dx, pre_in, stride, pad, wr=None):
    _need_gpu(dy, w, dx, pre_in); _f32c(dy, w, dx, pre_in)
    B, Cin, H, W = dx.shape
    _conv_call('mvae_conv2d_k4_dgrad', dy, w, dx, pre_in, B, Cin, H, W, w.shape[0], stride, pad, repack=True, wr=wr)


def conv_repack_floats(transposed, w, B, Cin, H, W, Cout, stride, pad):
    """Floats of the repacked weight copy a Conv2d data gradient (transposed False) / ConvTranspose2d forward
    (True) of this geometry reads, or 0 when that launch reads ``w`` itself (include/mvae_hip.h)."""
    return int(_lib.lib().mvae_conv_k4_repack_floats(1 if transposed else 0, _ptr(w), B, Cin, H, W, Cout, stride, pad))


def conv_repack_batched(items):
    """items: [(w, wr, transposed, Cin, Cout, stride, pad)] -- all repacked copies in one launch (16 per launch)."""
    items = list(items)
    for lo in range(0, len(items), _lib.REPACK_MAX):
        chunk = items[lo:lo + _lib.REPACK_MAX]
        arr = (_lib.RepackItem * len(chunk))()
        for q, (w, wr, tr, Cin, Cout, s, p) in enumerate(chunk):
            _need_gpu(w, wr); _f32c(w, wr)
            if wr.numel() < Cin * Cout * 16:
                raise RuntimeError('repack buffer too small')
            arr[q] = _lib.RepackItem(_ptr(w), _ptr(wr), 1 if tr else 0, Cin, Cout, s, p)
        check(_lib.lib().mvae_conv_k4_repack_batched(arr, len(chunk), _stream()), 'mvae_conv_k4_repack_batched')


def conv_route(op, B, Cin, H, W, Cout, stride, pad, ws_bytes=None):
    """(route, splits) of the launch ``op`` (a key of ``_lib.CONV_OPS``) on this geometry -- B, Cin, H, W, Cout as that
    launch's own arguments, i.e. the module's channels and its INPUT map: the name of the kernel it takes
    (``_lib.CONV_ROUTES``) and the number of partials its finish launch sums (1: none).  Host only (mvae_conv_k4_route:
    the decision function the launch itself switches on, for 16-byte-aligned operands).  ``ws_bytes``: the scratch the
    launch gets, by default what the wrappers here pass before anything asked for more (``_WS_MIN_BYTES``).  Raises
    where the launch would refuse the arguments."""
    n = ctypes.c_int(1)
    rc = _lib.lib().mvae_conv_k4_route(_lib.CONV_OPS[op], B, Cin, H, W, Cout, stride, pad,
                                       _WS_MIN_BYTES if ws_bytes is None else int(ws_bytes), ctypes.byref(n))
    if rc <= 0:
        check(rc if rc < 0 else -1, 'mvae_conv_k4_route')
    return _lib.CONV_ROUTES[rc], n.value


def conv2d_wgrad(dy, x, dw, stride, pad, accumulate=False):
    _need_gpu(dy, x, dw); _f32c(dy, x, dw)
    B, Cin, H, W = x.shape
    Cout = dw.shape[0]
    nbytes = _lib.lib().mvae_gemm_ws_bytes(Cout, Cin * 16, B * dy.shape[2] * dy.shape[3])
    ws, wsb = _ws_args(nbytes, dy.device)
    check(_lib.lib().mvae_conv2d_k4_wgrad(_ptr(dy), _ptr(x), _ptr(dw), B, Cin, H, W, Cout, stride, pad,
                                          ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_conv2d_k4_wgrad')


def convT2d_fwd(x, w, pre, act, stride, pad, wr=None):
    """x[B,Cin,H,W], w[Cin,Cout,4,4] -> [B,Cout,(H-1)s-2p+4, ...]"""
    _need_gpu(x, w, pre, act); _f32c(x, w, pre, act)
    B, Cin, H, W = x.shape
    _conv_call('mvae_convT2d_k4_fwd', x, w, pre, act, B, Cin, H, W, w.shape[1], stride, pad, repack=True, wr=wr)


def convT2d_stats_tiles(x, w, stride, pad):
    """Records the statistics-only launch would write for ConvTranspose2d(w)(x), 0 if the shape is not covered."""
    B, Cin, H, W = x.shape
    return int(_lib.lib().mvae_convT2d_k4_stats_tiles(B, Cin, H, W, w.shape[1], stride, pad))


def convT2d_fwd_stats(x, w, stride, pad, wr=None):
    """ConvTranspose2d(w)(x) WITHOUT storing it: returns part [tiles, Cout, 2] = (mean, M2) of every 512-element
    column tile per output channel (mvae_convT2d_k4_fwd_stats), for ``bn_stats_merge``.  ``wr``: the repacked
    weight copy made ahead (conv_repack_batched)."""
    _need_gpu(x, w, wr); _f32c(x, w, wr)
    B, Cin, H, W = x.shape
    Cout = w.shape[1]
    tiles = convT2d_stats_tiles(x, w, stride, pad)
    if tiles <= 0:
        raise RuntimeError('statistics-only transposed conv: shape %s -> %d channels not covered' % (tuple(x.shape), Cout))
    part = torch.empty(tiles, Cout, 2, dtype=torch.float32, device=x.device)
    if wr is not None:
        ws, wsb, wp = _ptr(wr), wr.numel() * 4, None
    else:
        ws, wsb = _ws_args(Cin * Cout * 16 * 4, x.device)
        wp = _ptr(w)
    check(_lib.lib().mvae_convT2d_k4_fwd_stats(_ptr(x), wp, _ptr(part), part.numel(), B, Cin, H, W, Cout, stride, pad,
                                               ws, wsb, _stream()), 'mvae_convT2d_k4_fwd_stats')
    return part


def bn_stats_merge(part, G, save_mean, save_invstd, running_mean, running_var, eps=1e-5, momentum=0.1, n_updates=1,
                   n_updates_dev=None):
    """Saved + running BatchNorm statistics of G groups from the records of ``convT2d_fwd_stats``."""
    _need_gpu(part, save_mean, save_invstd, running_mean, running_var)
    _f32c(part, save_mean, save_invstd, running_mean, running_var)
    tiles, C = part.shape[0], part.shape[1]
    check(_lib.lib().mvae_bn_stats_merge(_ptr(part), tiles, _lib.STATS_TILE_ELEMS, G, C, _ptr(save_mean), _ptr(save_invstd),
                                         _ptr(running_mean), _ptr(running_var), eps, momentum, n_updates,
                                         _ptr(n_updates_dev), _stream()), 'mvae_bn_stats_merge')


def convT2d_dgrad(dy, w, dx, pre_in, stride, pad):
    _need_gpu(dy, w, dx, pre_in); _f32c(dy, w, dx, pre_in)
    B, Cin, H, W = dx.shape
    _conv_call('mvae_convT2d_k4_dgrad', dy, w, dx, pre_in, B, Cin, H, W, w.shape[1], stride, pad)


def convT2d_wgrad(dy, x, dw, stride, pad, accumulate=False):
    _need_gpu(dy, x, dw); _f32c(dy, x, dw)
    B, Cin, H, W = x.shape
    Cout = dw.shape[1]
    nbytes = _lib.lib().mvae_gemm_ws_bytes(Cin, Cout * 16, B * H * W)
    ws, wsb = _ws_args(nbytes, dy.device)
    check(_lib.lib().mvae_convT2d_k4_wgrad(_ptr(dy), _ptr(x), _ptr(dw), B, Cin, H, W, Cout, stride, pad,
                                           ACCUMULATE if accumulate else 0, ws, wsb, _stream()),
          'mvae_convT2d_k4_wgrad')


# ---------------------------------------------------------------------------- general stride-2 convs (K17)
def conv_gen_supported(transposed, B, Cin, H, W, Cout, ks, stride, pad):
    """Whether the general stride-2 family (csrc/conv_gen.hip) runs this geometry -- B, Cin, H, W, Cout as the
    forward launch's own arguments.  Host only: the predicate the launches themselves apply."""
    return bool(_lib.lib().mvae_conv_gen_supported(1 if transposed else 0, B, Cin, H, W, Cout, ks, stride, pad))


def _gen_ws(op, dev, B, Cin, H, W, Cout, ks, stride, pad):
    nbytes = _lib.lib().mvae_conv_gen_ws_bytes(_lib.CONV_OPS[op], B, Cin, H, W, Cout, ks, stride, pad)
    return _ws_args(nbytes, dev)


def conv2d_gen_fwd(x, w, pre, act, stride, pad):
    """x[B,Cin,H,W], w[Cout,Cin,ks,ks] -> [B,Cout,(H+2p-ks)//2+1, ...]"""
    _need_gpu(x, w, pre, act); _f32c(x, w, pre, act)
    B, Cin, H, W = x.shape
    check(_lib.lib().mvae_conv2d_gen_fwd(_ptr(x), _ptr(w), _ptr(pre), _ptr(act), B, Cin, H, W, w.shape[0], w.shape[2],
                                         stride, pad, _stream()), 'mvae_conv2d_gen_fwd')


def conv2d_gen_dgrad(dy, w, dx, pre_in, stride, pad):
    _need_gpu(dy, w, dx, pre_in); _f32c(dy, w, dx, pre_in)
    B, Cin, H, W = dx.shape
    ws, wsb = _gen_ws('conv_dgrad', dy.device, B, Cin, H, W, w.shape[0], w.shape[2], stride, pad)
    check(_lib.lib().mvae_conv2d_gen_dgrad(_ptr(dy), _ptr(w), _ptr(dx), _ptr(pre_in), B, Cin, H, W, w.shape[0], w.shape[2],
                                           stride, pad, ws, wsb, _stream()), 'mvae_conv2d_gen_dgrad')


def conv2d_gen_wgrad(dy, x, dw, stride, pad, accumulate=False):
    _need_gpu(dy, x, dw); _f32c(dy, x, dw)
    B, Cin, H, W = x.shape
    Cout, ks = dw.shape[0], dw.shape[2]
    ws, wsb = _gen_ws('conv_wgrad', dy.device, B, Cin, H, W, Cout, ks, stride, pad)
    check(_lib.lib().mvae_conv2d_gen_wgrad(_ptr(dy), _ptr(x), _ptr(dw), B, Cin, H, W, Cout, ks, stride, pad,
                                           ACCUMULATE if accumulate else 0, ws, wsb, _stream()), 'mvae_conv2d_gen_wgrad')


def convT2d_gen_fwd(x, w, pre, act, stride, pad):
    """x[B,Cin,H,W], w[Cin,Cout,ks,ks] -> [B,Cout,(H-1)*2-2p+ks, ...]"""
    _need_gpu(x, w, pre, act); _f32c(x, w, pre, act)
    B, Cin, H, W = x.shape
    ws, wsb = _gen_ws('convT_fwd', x.device, B, Cin, H, W, w.shape[1], w.shape[2], stride, pad)
    check(_lib.lib().mvae_convT2d_gen_fwd(_ptr(x), _ptr(w), _ptr(pre), _ptr(act), B, Cin, H, W, w.shape[1], w.shape[2],
                                          stride, pad, ws, wsb, _stream()), 'mvae_convT2d_gen_fwd')


def convT2d_gen_dgrad(dy, w, dx, pre_in, stride, pad):
    _need_gpu(dy, w, dx, pre_in); _f32c(dy, w, dx, pre_in)
    B, Cin, H, W = dx.shape
    check(_lib.lib().mvae_convT2d_gen_dgrad(_ptr(dy), _ptr(w), _ptr(dx), _ptr(pre_in), B, Cin, H, W, w.shape[1], w.shape[2],
                                            stride, pad, _stream()), 'mvae_convT2d_gen_dgrad')


def convT2d_gen_wgrad(dy, x, dw, stride, pad, accumulate=False):
    _need_gpu(dy, x, dw); _f32c(dy, x, dw)
    B, Cin, H, W = x.shape
    Cout, ks = dw.shape[1], dw.shape[2]
    ws, wsb = _gen_ws('convT_wgrad', dy.device, B, Cin, H, W, Cout, ks, stride, pad)
    check(_lib.lib().mvae_convT2d_gen_wgrad(_ptr(dy), _ptr(x), _ptr(dw), B, Cin, H, W, Cout, ks, stride, pad,
                                            ACCUMULATE if accumulate else 0, ws, wsb, _stream()), 'mvae_convT2d_gen_wgrad')


# ---------------------------------------------------------------------------- BatchNorm
def bn_train_fwd(x, gamma, beta, y, save_mean, save_invstd, running_mean, running_var, G,
                 eps=1e-5, momentum=0.1, n_updates=1, swish=True, n_updates_dev=None):
    """x [G*B, C, *spatial]; save_* [G, C].  ``n_updates_dev``: device int32[1] overriding
    ``n_updates`` (celeba19: how many terms of this step contain the image)."""
    _need_gpu(x, gamma, beta, y, save_mean, save_invstd, running_mean, running_var)
    _f32c(x, gamma, beta, y, save_mean, save_invstd, running_mean, running_var)
    GB, C = x.shape[0], x.shape[1]
    HW = x.numel() // (GB * C)
    B = GB // G
    nbytes = _lib.lib().mvae_bn_ws_bytes(G, C, B * HW)
    ws, wsb = _ws_args(nbytes, x.device)
    check(_lib.lib().mvae_bn_train_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(save_mean),
                                       _ptr(save_invstd), _ptr(running_mean), _ptr(running_var),
                                       G, B, C, HW, eps, momentum, n_updates, _ptr(n_updates_dev),
                                       ACT_SWISH if swish else 0,
                                       ws, wsb, _stream()), 'mvae_bn_train_fwd')


def bn_train_bwd(dy, x, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta, G, swish=True,
                 accumulate=False):
    _need_gpu(dy, x, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta)
    _f32c(dy, x, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta)
    GB, C = x.shape[0], x.shape[1]
    HW = x.numel() // (GB * C)
    B = GB // G
    nbytes = _lib.lib().mvae_bn_ws_bytes(G, C, B * HW)
    ws, wsb = _ws_args(nbytes, x.device)
    flags = (ACT_SWISH if swish else 0) | (ACCUMULATE if accumulate else 0)
    check(_lib.lib().mvae_bn_train_bwd(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(save_mean),
                                       _ptr(save_invstd), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                       G, B, C, HW, flags, ws, wsb, _stream()), 'mvae_bn_train_bwd')


def bn_route(G, B, C, HW, bwd=False, aligned=True):
    """(route, slices, launches) of ``bn_train_fwd`` (``bwd=True``: ``bn_train_bwd``) on G groups of B rows, C channels
    and HW spatial positions (1: BatchNorm1d) -- the name of the kernel it takes (``_lib.BN_ROUTES``), the batch slices S
    per (group, channel) of the two-launch routes (1 for the others) and the number of kernel launches ('slice': 2, the
    call with running statistics).  ``aligned``: x, y / dy and dx are all 16-byte aligned.  Host only (mvae_bn_route: the
    route function the launch itself switches on).  Raises where the launch would refuse the shape."""
    sl, ln = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mvae_bn_route(1 if bwd else 0, G, B, C, HW, 1 if aligned else 0, ctypes.byref(sl), ctypes.byref(ln))
    if rc <= 0:
        check(rc if rc < 0 else -1, 'mvae_bn_route')
    return _lib.BN_ROUTES[rc], sl.value, ln.value


def bn_eval_fwd(x, gamma, beta, y, running_mean, running_var, eps=1e-5, swish=True):
    _need_gpu(x, gamma, beta, y, running_mean, running_var)
    _f32c(x, gamma, beta, y, running_mean, running_var)
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // (N * C)
    check(_lib.lib().mvae_bn_eval_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(running_mean),
                                      _ptr(running_var), N, C, HW, eps, ACT_SWISH if swish else 0,
                                      _stream()), 'mvae_bn_eval_fwd')


# ---------------------------------------------------------------------------- elementwise / embedding
def reparam_fwd(mu, logvar, eps, z):
    """z = eps * exp(logvar / 2) + mu (mnist/model.py:29-35), elementwise."""
    _need_gpu(mu, logvar, eps, z); _f32c(mu, logvar, eps, z)
    check(_lib.lib().mvae_reparam_fwd(_ptr(mu), _ptr(logvar), _ptr(eps), _ptr(z), mu.numel(), _stream()),
          'mvae_reparam_fwd')


def sigmoid_fwd(x, y):
    _need_gpu(x, y); _f32c(x, y)
    check(_lib.lib().mvae_sigmoid_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), 'mvae_sigmoid_fwd')


def affine_fwd(x, scale, shift, y):
    """y = x * scale + shift with scale / shift of ``period`` = scale.numel() elements repeated along x."""
    _need_gpu(x, scale, shift, y); _f32c(x, scale, shift, y)
    if scale.numel() != shift.numel() or x.numel() % scale.numel():
        raise RuntimeError('affine_fwd: scale/shift must have equal sizes dividing x')
    check(_lib.lib().mvae_affine_fwd(_ptr(x), _ptr(scale), _ptr(shift), _ptr(y), x.numel(), scale.numel(),
                                     _stream()), 'mvae_affine_fwd')


def swish_fwd(x, y):
    _need_gpu(x, y); _f32c(x, y)
    check(_lib.lib().mvae_swish_fwd(_ptr(x), _ptr(y), x.numel(), _stream()), 'mvae_swish_fwd')


def swish_bwd(dy, x, dx):
    _need_gpu(dy, x, dx); _f32c(dy, x, dx)
    check(_lib.lib().mvae_swish_bwd(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), _stream()), 'mvae_swish_bwd')


def _index_kind(idx):
    """0 = contiguous int64 labels; s > 0 = fp32 {0,1} values with element stride s (a column of
    attrs[B,18] has s = 18)."""
    if idx.dim() != 1:
        raise RuntimeError('embedding index must be 1-D')
    if idx.dtype == torch.int64:
        if idx.numel() > 1 and idx.stride(0) != 1:
            raise RuntimeError('int64 embedding index must be contiguous')
        return 0
    if idx.dtype == torch.float32:
        return max(int(idx.stride(0)), 1)
    raise RuntimeError('embedding index must be int64 or float32, got %s' % idx.dtype)


def block_gather(src, idx_dev, dst, block_elems):
    _need_gpu(src, idx_dev, dst); _f32c(src, dst)
    check(_lib.lib().mvae_block_gather(_ptr(src), _ptr(idx_dev), _ptr(dst), idx_dev.numel(), block_elems,
                                       _stream()), 'mvae_block_gather')


def block_scatter_add(src, idx_dev, dst, n_dst, block_elems):
    _need_gpu(src, idx_dev, dst); _f32c(src, dst)
    check(_lib.lib().mvae_block_scatter_add(_ptr(src), _ptr(idx_dev), _ptr(dst), idx_dev.numel(), n_dst,
                                            block_elems, _stream()), 'mvae_block_scatter_add')


def scatter_sums(vals, coef, idx_dev, out, total, accumulate_total=True):
    _need_gpu(vals, coef, idx_dev, out, total); _f32c(vals, coef, out, total)
    check(_lib.lib().mvae_scatter_sums(_ptr(vals), _ptr(coef), _ptr(idx_dev), _ptr(out), _ptr(total),
                                       vals.numel(), ACCUMULATE if accumulate_total else 0, _stream()),
          'mvae_scatter_sums')


def embedding_swish_fwd(idx, w, act):
    _need_gpu(idx, w, act); _f32c(w, act)
    check(_lib.lib().mvae_embedding_swish_fwd(_ptr(idx), _index_kind(idx), _ptr(w), _ptr(act), idx.numel(),
                                              w.shape[0], w.shape[1], _stream()),
          'mvae_embedding_swish_fwd')


def embedding_swish_bwd(idx, w, dact, dw, accumulate=False):
    _need_gpu(idx, w, dact, dw); _f32c(w, dact, dw)
    check(_lib.lib().mvae_embedding_swish_bwd(_ptr(idx), _index_kind(idx), _ptr(w), _ptr(dact), _ptr(dw),
                                              idx.numel(), w.shape[0], w.shape[1],
                                              ACCUMULATE if accumulate else 0, _stream()),
          'mvae_embedding_swish_bwd')


# ---------------------------------------------------------------------------- PoE / KL
def _experts(mus, lvs):
    ex = _lib.Experts()
    for i, (m, v) in enumerate(zip(mus, lvs)):
        ex.mu[i] = m.data_ptr()
        ex.logvar[i] = v.data_ptr()
    return ex


def _expert_ld(mus, lvs):
    if len(mus) > _lib.MAX_EXPERTS:
        raise RuntimeError('at most %d experts' % _lib.MAX_EXPERTS)
    ld = mus[0].stride(0) if mus else 0
    for t in list(mus) + list(lvs):
        _need_gpu(t)
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != ld:
            raise RuntimeError('expert mu/logvar must be fp32 [B,D] views with unit column stride and '
                               'a common row stride')
    return ld


_ALL_EXPERTS = {}


def all_experts_mask(n_experts, device):
    """Device mask [1] with the low ``n_experts`` bits set -- the kernel reads it as uint32, the tensor is int32 with
    the same bits ((1 << 32) - 1 does not fit torch.int32: MVAE_MAX_EXPERTS = 32 experts is the all-ones word, -1)."""
    if not 1 <= n_experts <= _lib.MAX_EXPERTS:
        raise RuntimeError('1..%d experts, got %d' % (_lib.MAX_EXPERTS, n_experts))
    capturing = torch.cuda.is_current_stream_capturing()
    key = (n_experts, str(device))
    if not capturing and key in _ALL_EXPERTS:
        return _ALL_EXPERTS[key]          # read-only: one fill launch per (count, device), not one per model() call
    bits = (1 << n_experts) - 1
    m = torch.full((1,), bits - (1 << 32) if bits >= (1 << 31) else bits, dtype=torch.int32, device=device)
    m._mvae_mask_ok = m._version          # non-empty by construction: _check_no_prior_masks need not read it back
    if not capturing:                     # (a tensor filled under capture only has its contents after a replay)
        _ALL_EXPERTS[key] = m
    return m


def _check_no_prior_masks(masks_dev, variant, n_experts):
    """MVAE_POE_NO_PRIOR: a term whose mask selects no expert is an empty product (0 / 0 precision: NaN mu, inf
    logvar, no error from the launch -- the C side cannot see a device mask).  Host-built masks are checked here;
    masks that only exist on the device (a captured graph's tables) are the caller's to keep non-empty."""
    if not str(variant).endswith('-noprior') or masks_dev.numel() > 64 or torch.cuda.is_current_stream_capturing():
        return
    # the read-back below is a blocking device-to-host copy: pay it once per mask tensor CONTENT, never per launch
    # (every model() call on the drop-in surface paid it for a mask that is non-empty by construction)
    if getattr(masks_dev, '_mvae_mask_ok', None) == masks_dev._version:
        return
    live = (1 << n_experts) - 1
    for t, m in enumerate(masks_dev.tolist()):
        if (m & live) == 0:
            raise RuntimeError('PoE without the built-in prior: term %d selects no expert (mask %#x)' % (t, m & 0xffffffff))
    try:
        masks_dev._mvae_mask_ok = masks_dev._version
    except AttributeError:
        pass


def poe_fwd(mus, lvs, masks_dev, noise, mu, logvar, z, kl, variant):
    """mus/lvs: per-expert [B,D] (possibly column slices of a [B,2D] head); masks_dev int32/uint32 [T]."""
    ld = _expert_ld(mus, lvs)
    _need_gpu(masks_dev, noise, mu, logvar, z, kl); _f32c(noise, mu, logvar, z, kl)
    T, B, D = mu.shape
    ex = _experts(mus, lvs)
    _check_no_prior_masks(masks_dev, variant, len(mus))
    check(_lib.lib().mvae_poe_fwd(ctypes.byref(ex), ld, len(mus), _ptr(masks_dev), T, _ptr(noise), _ptr(mu),
                                  _ptr(logvar), _ptr(z), _ptr(kl), B, D, _lib.POE_VARIANT[variant],
                                  _stream()), 'mvae_poe_fwd')


def poe_fwd_draw(mus, lvs, masks_dev, noise_out, seed, counter_dev, counter_offset, mu, logvar, z, kl, variant):
    """``poe_fwd`` drawing its own eps: the values ``philox_fill(noise_out, seed, counter_dev, counter_offset)`` would
    have written, generated in the launch and stored to ``noise_out`` for the backward."""
    ld = _expert_ld(mus, lvs)
    _need_gpu(masks_dev, noise_out, counter_dev, mu, logvar, z, kl); _f32c(noise_out, mu, logvar, z, kl)
    T, B, D = mu.shape
    ex = _experts(mus, lvs)
    check(_lib.lib().mvae_poe_fwd_draw(ctypes.byref(ex), ld, len(mus), _ptr(masks_dev), T, _ptr(noise_out), seed,
                                       _ptr(counter_dev), int(counter_offset), _ptr(mu), _ptr(logvar), _ptr(z),
                                       _ptr(kl), B, D, _lib.POE_VARIANT[variant], _stream()), 'mvae_poe_fwd_draw')


def poe_bwd(mus, lvs, masks_dev, noise, mu, logvar, dz, dmu, dlogvar, dkl, g_mus, g_lvs, variant,
            dkl_per_term=False):
    """dkl: [T,B] row gradients of the KL output, or with dkl_per_term a [T] table (beta/B)."""
    ld = _expert_ld(mus, lvs)
    ldg = _expert_ld(g_mus, g_lvs)
    _need_gpu(masks_dev, noise, mu, logvar, dz, dmu, dlogvar, dkl)
    _f32c(noise, mu, logvar, dz, dmu, dlogvar, dkl)
    T, B, D = mu.shape
    ex = _experts(mus, lvs)
    gr = _lib.ExpertGrads()
    for i, (m, v) in enumerate(zip(g_mus, g_lvs)):
        gr.dmu[i] = m.data_ptr()
        gr.dlogvar[i] = v.data_ptr()
    check(_lib.lib().mvae_poe_bwd(ctypes.byref(ex), ld, len(mus), _ptr(masks_dev), T, _ptr(noise), _ptr(mu),
                                  _ptr(logvar), _ptr(dz), _ptr(dmu), _ptr(dlogvar), _ptr(dkl),
                                  1 if dkl_per_term else 0, ctypes.byref(gr), ldg, B, D, _lib.POE_VARIANT[variant], _stream()),
          'mvae_poe_bwd')


def poe_bwd_split(mus, lvs, masks_dev, noise, mu, logvar, dz_a, slots_a, dz_b, slots_b, dkl, g_mus, g_lvs, variant,
                  dkl_per_term=False):
    """poe_bwd with the latent gradient in two buffers: dz of term t = dz_a[slots_a[t]] + dz_b[slots_b[t]]
    (slot -1: not in that buffer); dz_* are [n_slots, B, D]."""
    ld = _expert_ld(mus, lvs)
    ldg = _expert_ld(g_mus, g_lvs)
    _need_gpu(masks_dev, noise, mu, logvar, dz_a, dz_b, dkl)
    _f32c(noise, mu, logvar, dz_a, dz_b, dkl)
    T, B, D = mu.shape
    if len(slots_a) != T or len(slots_b) != T:
        raise RuntimeError('one slot per term')
    for dz, slots in ((dz_a, slots_a), (dz_b, slots_b)):
        if dz.numel() != (max(slots) + 1) * B * D:
            raise RuntimeError('latent-gradient buffer does not match its slots')
    ex = _experts(mus, lvs)
    gr = _lib.ExpertGrads()
    for i, (m, v) in enumerate(zip(g_mus, g_lvs)):
        gr.dmu[i] = m.data_ptr()
        gr.dlogvar[i] = v.data_ptr()
    sa = (ctypes.c_int * T)(*[int(x) for x in slots_a])
    sb = (ctypes.c_int * T)(*[int(x) for x in slots_b])
    check(_lib.lib().mvae_poe_bwd_split(ctypes.byref(ex), ld, len(mus), _ptr(masks_dev), T, _ptr(noise), _ptr(mu),
                                        _ptr(logvar), _ptr(dz_a), sa, _ptr(dz_b), sb, _ptr(dkl),
                                        1 if dkl_per_term else 0, ctypes.byref(gr), ldg, B, D,
                                        _lib.POE_VARIANT[variant], _stream()), 'mvae_poe_bwd_split')


def _ragged_tables(mus, lvs, erow_dev, masks_dev, slot_dev, B):
    """Checks shared by the ragged PoE launchers -> (Experts, ld, n_rows array).  ``mus`` / ``lvs`` hold None for an
    expert no row has."""
    E = len(mus)
    if not 1 <= E <= _lib.MAX_EXPERTS or len(lvs) != E:
        raise RuntimeError('1..%d experts' % _lib.MAX_EXPERTS)
    live = [(m, v) for m, v in zip(mus, lvs) if m is not None and m.shape[0] > 0]
    ld = _expert_ld([m for m, _ in live], [v for _, v in live])
    for t, shape in ((erow_dev, (E, B)), (slot_dev, (masks_dev.numel(), B))):
        _need_gpu(t)
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError('ragged PoE: index table must be contiguous int32 %s, got %s %s'
                               % (shape, t.dtype, tuple(t.shape)))
    _need_gpu(masks_dev)
    ex = _lib.Experts()
    n_rows = (ctypes.c_int * E)()
    for e, (m, v) in enumerate(zip(mus, lvs)):
        if m is None or m.shape[0] == 0:
            continue
        if v is None or v.shape != m.shape:
            raise RuntimeError('ragged PoE: expert %d has mu %s and logvar %s' % (e, tuple(m.shape),
                                                                                 None if v is None else tuple(v.shape)))
        ex.mu[e], ex.logvar[e], n_rows[e] = m.data_ptr(), v.data_ptr(), m.shape[0]
    return ex, ld, n_rows


def poe_ragged_fwd(mus, lvs, erow_dev, masks_dev, slot_dev, R, noise, mu, logvar, z, kl, variant, B, draw=None):
    """PoE on a batch whose rows have different experts (include/mvae_hip.h, K29).  mus/lvs: per-expert compact
    [n_e, D] views (None: no row has the expert); erow_dev int32 [E, B]; slot_dev int32 [T, B]; outputs compact with at
    least R rows.  noise dense [T, B, D] (read), or with ``draw = (seed, counter_dev, counter_offset)`` written."""
    ex, ld, n_rows = _ragged_tables(mus, lvs, erow_dev, masks_dev, slot_dev, B)
    _need_gpu(noise, mu, logvar, z, kl); _f32c(noise, mu, logvar, z, kl)
    T, D = masks_dev.numel(), mu.shape[1]
    for t, n in ((mu, R * D), (logvar, R * D), (z, R * D), (kl, R), (noise, T * B * D)):
        if t is not None and t.numel() < n:
            raise RuntimeError('ragged PoE: a buffer of %d elements where %d are needed' % (t.numel(), n))
    if ld == 0:
        ld = D          # no expert has a row: the prior alone
    seed, counter_dev, counter_offset = draw if draw is not None else (0, None, 0)
    _need_gpu(counter_dev)
    check(_lib.lib().mvae_poe_ragged_fwd(ctypes.byref(ex), ld, len(mus), n_rows, _ptr(erow_dev), _ptr(masks_dev), T,
                                         _ptr(slot_dev), int(R), _ptr(noise), 1 if draw is not None else 0, int(seed),
                                         _ptr(counter_dev), int(counter_offset), _ptr(mu), _ptr(logvar), _ptr(z),
                                         _ptr(kl), B, D, _lib.POE_VARIANT[variant], _stream()), 'mvae_poe_ragged_fwd')


def poe_ragged_bwd(mus, lvs, erow_dev, masks_dev, slot_dev, R, noise, mu, logvar, dz, dmu, dlogvar, dkl, g_mus, g_lvs,
                   variant, B):
    """Backward of ``poe_ragged_fwd``: dz / dmu / dlogvar [R, D], dkl [R] (any None) -> every element of the experts'
    compact gradient views g_mus / g_lvs (None where the expert has no row)."""
    ex, ld, n_rows = _ragged_tables(mus, lvs, erow_dev, masks_dev, slot_dev, B)
    live = [(m, v) for m, v in zip(g_mus, g_lvs) if m is not None and m.shape[0] > 0]
    ldg = _expert_ld([m for m, _ in live], [v for _, v in live])
    _need_gpu(noise, mu, logvar, dz, dmu, dlogvar, dkl); _f32c(noise, mu, logvar, dz, dmu, dlogvar, dkl)
    T, D = masks_dev.numel(), mu.shape[1]
    for t, n in ((mu, R * D), (logvar, R * D), (dz, R * D), (dmu, R * D), (dlogvar, R * D), (dkl, R),
                 (noise, T * B * D)):
        if t is not None and t.numel() < n:
            raise RuntimeError('ragged PoE: a buffer of %d elements where %d are needed' % (t.numel(), n))
    gr = _lib.ExpertGrads()
    for e, (m, v) in enumerate(zip(g_mus, g_lvs)):
        if n_rows[e] == 0:
            continue
        if m is None or v is None or m.shape[0] != n_rows[e] or v.shape != m.shape:
            raise RuntimeError('ragged PoE: gradient views of expert %d do not match its %d rows' % (e, n_rows[e]))
        gr.dmu[e], gr.dlogvar[e] = m.data_ptr(), v.data_ptr()
    if ld == 0:
        ld = ldg = D
    check(_lib.lib().mvae_poe_ragged_bwd(ctypes.byref(ex), ld, len(mus), n_rows, _ptr(erow_dev), _ptr(masks_dev), T,
                                         _ptr(slot_dev), int(R), _ptr(noise), _ptr(mu), _ptr(logvar), _ptr(dz),
                                         _ptr(dmu), _ptr(dlogvar), _ptr(dkl), ctypes.byref(gr), ldg, B, D,
                                         _lib.POE_VARIANT[variant], _stream()), 'mvae_poe_ragged_bwd')


def kl_rows_fwd(mu, logvar, kl):
    _need_gpu(mu, logvar, kl); _f32c(mu, logvar, kl)
    check(_lib.lib().mvae_kl_rows_fwd(_ptr(mu), _ptr(logvar), _ptr(kl), mu.shape[0], mu.shape[1], _stream()),
          'mvae_kl_rows_fwd')


def kl_rows_bwd(mu, logvar, dkl, dmu, dlogvar):
    _need_gpu(mu, logvar, dkl, dmu, dlogvar); _f32c(mu, logvar, dkl, dmu, dlogvar)
    check(_lib.lib().mvae_kl_rows_bwd(_ptr(mu), _ptr(logvar), _ptr(dkl), _ptr(dmu), _ptr(dlogvar),
                                      mu.shape[0], mu.shape[1], _stream()), 'mvae_kl_rows_bwd')


# ---------------------------------------------------------------------------- losses
def bce_rowsum_fwd(logits, target, rowsum, colw=None, drow=None, dlogits=None, rows_per_group=None,
                   target_rows=None, target_div=1, target_strides=None):
    """logits [R,P]; target [target_rows,P] broadcast over row groups; optional fused gradient."""
    _need_gpu(logits, target, rowsum, colw, drow, dlogits); _f32c(logits, target, rowsum, colw, drow, dlogits)
    R, P = logits.shape
    t_rs, t_cs = target_strides if target_strides is not None else (P, 1)
    check(_lib.lib().mvae_bce_rowsum_fwd(_ptr(logits), _ptr(target), _ptr(colw), _ptr(rowsum), _ptr(drow),
                                         _ptr(dlogits), R, P, rows_per_group or R,
                                         target_rows or target.shape[0], target_div, t_rs, t_cs, _stream()),
          'mvae_bce_rowsum_fwd')


def bce_rowsum_bwd(logits, target, drow, dlogits, colw=None, rows_per_group=None, target_rows=None,
                   target_div=1, target_strides=None):
    _need_gpu(logits, target, drow, dlogits, colw); _f32c(logits, target, drow, dlogits, colw)
    R, P = logits.shape
    t_rs, t_cs = target_strides if target_strides is not None else (P, 1)
    check(_lib.lib().mvae_bce_rowsum_bwd(_ptr(logits), _ptr(target), _ptr(colw), _ptr(drow), _ptr(dlogits),
                                         R, P, rows_per_group or R, target_rows or target.shape[0],
                                         target_div, t_rs, t_cs, _stream()), 'mvae_bce_rowsum_bwd')


def bce_route(P, aligned=True, target_col_stride=1, colw=False):
    """(route, batched_trips, tail) of a row of P logits in ``bce_rowsum_fwd`` / ``bce_rowsum_bwd`` -- the name of the kernel
    and loop it takes (``_lib.BCE_ROUTES``), the four-group trips thread 0 of the block kernel makes and whether any thread
    makes a single-group trip (both 0 off the float4 path).  ``aligned``: the row's logits, target, column weights and
    dlogits are all 16-byte aligned; ``colw``: the call has column weights.  Host only (mvae_bce_route: the functions the
    launch and the kernel themselves switch on).  Raises where the launch would refuse P or the stride."""
    trips, tail = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().mvae_bce_route(P, target_col_stride, 1 if aligned else 0, 1 if colw else 0, ctypes.byref(trips),
                                   ctypes.byref(tail))
    if rc <= 0:
        check(rc if rc < 0 else -1, 'mvae_bce_route')
    return _lib.BCE_ROUTES[rc], trips.value, tail.value


def _bce_segs(segs, R):
    """[(logits [R,P], target [target_rows,P], dlogits [R,P] or None, weight)] -> (mvae_bce_seg table, target_rows)"""
    if not 0 < len(segs) <= _lib.BCE_MULTI_MAX:
        raise RuntimeError('1..%d BCE segments per launch' % _lib.BCE_MULTI_MAX)
    arr = (_lib.BceSeg * len(segs))()
    target_rows = segs[0][1].shape[0]
    for s, (logits, target, dlogits, weight) in enumerate(segs):
        _need_gpu(logits, target, dlogits); _f32c(logits, target, dlogits)
        P = logits.shape[-1]
        if logits.dim() != 2 or logits.shape[0] != R or tuple(target.shape) != (target_rows, P) or (
                dlogits is not None and dlogits.shape != logits.shape):
            raise RuntimeError('BCE segment %d: logits %s, target %s, dlogits %s for R = %d, target_rows = %d'
                               % (s, tuple(logits.shape), tuple(target.shape),
                                  None if dlogits is None else tuple(dlogits.shape), R, target_rows))
        arr[s] = _lib.BceSeg(_ptr(logits), _ptr(target), _ptr(dlogits), int(P), float(weight))
    return arr, target_rows


def bce_multi_fwd(segs, rowsum, drow=None, rows_per_group=None):
    """rowsum[r] = sum_s weight_s * sum_p bce(logits_s[r,p], target_s[r % target_rows, p]) for the segments
    [(logits, target, dlogits or None, weight)] in ONE launch (+ the small launch that adds the partials); with
    ``drow`` [R / rows_per_group] the segments that carry ``dlogits`` get their gradient in the same pass."""
    R = segs[0][0].shape[0]
    arr, target_rows = _bce_segs(segs, R)
    _need_gpu(rowsum, drow); _f32c(rowsum, drow)
    nbytes = _lib.lib().mvae_bce_multi_ws_bytes(arr, len(segs), R)
    ws, ws_bytes = _ws_args(nbytes, segs[0][0].device)
    check(_lib.lib().mvae_bce_multi_fwd(arr, len(segs), _ptr(rowsum), _ptr(drow), R, rows_per_group or R, target_rows,
                                        ws, ws_bytes, _stream()), 'mvae_bce_multi_fwd')


def bce_multi_bwd(segs, drow, rows_per_group=None):
    """The gradient of ``bce_multi_fwd`` alone: dlogits_s[r,p] = drow[r / rows_per_group] * weight_s * dbce/dx."""
    R = segs[0][0].shape[0]
    arr, target_rows = _bce_segs(segs, R)
    _need_gpu(drow); _f32c(drow)
    check(_lib.lib().mvae_bce_multi_bwd(arr, len(segs), _ptr(drow), R, rows_per_group or R, target_rows, _stream()),
          'mvae_bce_multi_bwd')


def ce_fwd(logits, label, row, drow=None, dlogits=None, rows_per_group=None, label_rows=None):
    _need_gpu(logits, label, row, drow, dlogits); _f32c(logits, row, drow, dlogits)
    if label.dtype != torch.int64 or not label.is_contiguous():
        raise RuntimeError('labels must be contiguous int64')
    R, K = logits.shape
    check(_lib.lib().mvae_ce_fwd(_ptr(logits), _ptr(label), _ptr(row), _ptr(drow), _ptr(dlogits), R, K,
                                 rows_per_group or R, label_rows or label.shape[0], _stream()),
          'mvae_ce_fwd')


def ce_bwd(logits, label, drow, dlogits, rows_per_group=None, label_rows=None):
    _need_gpu(logits, label, drow, dlogits); _f32c(logits, drow, dlogits)
    R, K = logits.shape
    check(_lib.lib().mvae_ce_bwd(_ptr(logits), _ptr(label), _ptr(drow), _ptr(dlogits), R, K,
                                 rows_per_group or R, label_rows or label.shape[0], _stream()),
          'mvae_ce_bwd')


def _indexed_args(logits, target, rowmap, coef, out, dlogits, what):
    """Shapes of the indexed row sums (include/mvae_hip.h, K30): logits [R, P], rowmap int32 [R], coef / out [R]."""
    _need_gpu(logits, target, rowmap, coef, out, dlogits); _f32c(logits, coef, out, dlogits)
    R = logits.shape[0]
    if logits.dim() != 2 or rowmap.dtype != torch.int32 or not rowmap.is_contiguous() or rowmap.numel() != R or not \
            target.is_contiguous():
        raise RuntimeError('%s: logits [R, P], a contiguous int32 row map [R] and contiguous targets; got %s, %s %s'
                           % (what, tuple(logits.shape), rowmap.dtype, tuple(rowmap.shape)))
    for t in (coef, out):
        if t is not None and t.numel() != R:
            raise RuntimeError('%s: %d per-row values for %d rows' % (what, t.numel(), R))
    if dlogits is not None and dlogits.shape != logits.shape:
        raise RuntimeError('%s: dlogits %s for logits %s' % (what, tuple(dlogits.shape), tuple(logits.shape)))
    return R


def bce_rows_indexed_fwd(logits, target, rowmap, rowsum, coef=None, dlogits=None):
    """rowsum[r] = coef[r] * sum_p bce(logits[r, p], target[rowmap[r], p]); target [B, P] in batch order; with
    ``dlogits`` the gradient coef[r] * dbce/dx in the same pass."""
    R = _indexed_args(logits, target, rowmap, coef, rowsum, dlogits, 'bce_rows_indexed_fwd')
    _f32c(target)
    if target.dim() != 2 or target.shape[1] != logits.shape[1]:
        raise RuntimeError('bce_rows_indexed_fwd: target %s for logits %s' % (tuple(target.shape), tuple(logits.shape)))
    check(_lib.lib().mvae_bce_rows_indexed_fwd(_ptr(logits), _ptr(target), _ptr(rowmap), _ptr(coef), _ptr(rowsum),
                                               _ptr(dlogits), R, logits.shape[1], target.shape[0], _stream()),
          'mvae_bce_rows_indexed_fwd')


def bce_rows_indexed_bwd(logits, target, rowmap, drow, dlogits):
    """dlogits[r, p] = drow[r] * dbce/dx (drow None: 1)."""
    R = _indexed_args(logits, target, rowmap, drow, None, dlogits, 'bce_rows_indexed_bwd')
    _f32c(target)
    if target.dim() != 2 or target.shape[1] != logits.shape[1]:
        raise RuntimeError('bce_rows_indexed_bwd: target %s for logits %s' % (tuple(target.shape), tuple(logits.shape)))
    check(_lib.lib().mvae_bce_rows_indexed_bwd(_ptr(logits), _ptr(target), _ptr(rowmap), _ptr(drow), _ptr(dlogits), R,
                                               logits.shape[1], target.shape[0], _stream()),
          'mvae_bce_rows_indexed_bwd')


def ce_rows_indexed_fwd(logits, label, rowmap, row, coef=None, dlogits=None):
    """row[r] = coef[r] * -log_softmax(logits[r, :] + 1e-6)[label[rowmap[r]]]; label int64 [B] in batch order."""
    R = _indexed_args(logits, label, rowmap, coef, row, dlogits, 'ce_rows_indexed_fwd')
    if label.dtype != torch.int64 or label.dim() != 1:
        raise RuntimeError('labels must be contiguous int64 [B]')
    check(_lib.lib().mvae_ce_rows_indexed_fwd(_ptr(logits), _ptr(label), _ptr(rowmap), _ptr(coef), _ptr(row),
                                              _ptr(dlogits), R, logits.shape[1], label.shape[0], _stream()),
          'mvae_ce_rows_indexed_fwd')


def ce_rows_indexed_bwd(logits, label, rowmap, drow, dlogits):
    R = _indexed_args(logits, label, rowmap, drow, None, dlogits, 'ce_rows_indexed_bwd')
    if label.dtype != torch.int64 or label.dim() != 1:
        raise RuntimeError('labels must be contiguous int64 [B]')
    check(_lib.lib().mvae_ce_rows_indexed_bwd(_ptr(logits), _ptr(label), _ptr(rowmap), _ptr(drow), _ptr(dlogits), R,
                                              logits.shape[1], label.shape[0], _stream()), 'mvae_ce_rows_indexed_bwd')


def group_sums(rows, coef, out, total, G, rows_per_group, accumulate=False):
    """out[g] (+)= coef[g] * sum(rows[g*rpg:(g+1)*rpg]); total[0] (+)= their sum."""
    _need_gpu(rows, coef, out, total); _f32c(rows, coef, out, total)
    check(_lib.lib().mvae_group_sums(_ptr(rows), _ptr(coef), _ptr(out), _ptr(total), G, rows_per_group,
                                     ACCUMULATE if accumulate else 0, _stream()), 'mvae_group_sums')


def _elbo_parts(parts):
    if not 0 < len(parts) <= _lib.ELBO_MAX_PARTS:
        raise RuntimeError('1..%d ELBO parts per launch' % _lib.ELBO_MAX_PARTS)
    arr = (_lib.ElboPart * len(parts))()
    for q, (rows, coef, term_of, first, groups, rpg) in enumerate(parts):
        _need_gpu(rows, coef, term_of); _f32c(rows, coef)
        if rows.numel() < groups * rpg:
            raise RuntimeError('ELBO part %d: %d values for %d x %d' % (q, rows.numel(), groups, rpg))
        arr[q] = _lib.ElboPart(_ptr(rows), _ptr(coef), _ptr(term_of), int(first), int(groups), int(rpg))
    return arr


def elbo_reduce(parts, elbo, T, zero=None, counter_dev=None, counter_inc=0):
    """parts: [(rows, coef or None, term_of or None, first_term, groups, rows_per_group)] -- see
    mvae_elbo_reduce in include/mvae_hip.h.  Overwrites elbo[0..T]."""
    arr = _elbo_parts(parts)
    _need_gpu(elbo, zero, counter_dev); _f32c(elbo, zero)
    check(_lib.lib().mvae_elbo_reduce(arr, len(parts), _ptr(elbo), int(T), _ptr(zero),
                                      0 if zero is None else zero.numel(), _ptr(counter_dev), int(counter_inc),
                                      _stream()), 'mvae_elbo_reduce')


def elbo_reduce_prepare(parts, elbo, T, step_dev, delta, lr, beta1, beta2, coef2, zero=None, counter_dev=None,
                        counter_inc=0):
    """``elbo_reduce`` and ``adam_prepare(step_dev, delta, lr, beta1, beta2, coef2)`` in one launch
    (mvae_elbo_reduce_prepare)."""
    arr = _elbo_parts(parts)
    _need_gpu(elbo, zero, counter_dev, step_dev, coef2); _f32c(elbo, zero, coef2)
    check(_lib.lib().mvae_elbo_reduce_prepare(arr, len(parts), _ptr(elbo), int(T), _ptr(zero),
                                              0 if zero is None else zero.numel(), _ptr(counter_dev),
                                              int(counter_inc), _ptr(step_dev), int(delta), lr, beta1, beta2,
                                              _ptr(coef2), _stream()), 'mvae_elbo_reduce_prepare')


# ---------------------------------------------------------------------------- noise / optimiser
def philox_fill(out, seed, counter_dev, offset=0, keep_prob=None):
    """Standard normal (keep_prob None) or Bernoulli(keep_prob) draws at launch index *counter_dev + offset;
    the counter is NOT advanced (the fused step does that once per step in elbo_reduce)."""
    _need_gpu(out, counter_dev); _f32c(out)
    check(_lib.lib().mvae_philox_fill(_ptr(out), out.numel(), 0 if keep_prob is None else 1,
                                      0.0 if keep_prob is None else float(keep_prob), seed, _ptr(counter_dev),
                                      int(offset), _stream()), 'mvae_philox_fill')



def randn_(out, seed, counter_dev):
    _need_gpu(out, counter_dev); _f32c(out)
    check(_lib.lib().mvae_randn(_ptr(out), out.numel(), seed, _ptr(counter_dev), _stream()), 'mvae_randn')


def bernoulli_(out, keep_prob, seed, counter_dev):
    _need_gpu(out, counter_dev); _f32c(out)
    check(_lib.lib().mvae_bernoulli(_ptr(out), out.numel(), keep_prob, seed, _ptr(counter_dev), _stream()),
          'mvae_bernoulli')


def adam_step(param, grad, exp_avg, exp_avg_sq, step_dev, lr, beta1=0.9, beta2=0.999, eps=1e-8,
              grad_scale=1.0):
    _need_gpu(param, grad, exp_avg, exp_avg_sq, step_dev); _f32c(param, grad, exp_avg, exp_avg_sq)
    check(_lib.lib().mvae_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                    lr, beta1, beta2, eps, grad_scale, _ptr(step_dev), _stream()),
          'mvae_adam_step')


def adam_apply(param, grad, exp_avg, exp_avg_sq, step_dev, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """Adam on (a range of) the arena at step *step_dev + 1, without advancing the counter."""
    _need_gpu(param, grad, exp_avg, exp_avg_sq, step_dev); _f32c(param, grad, exp_avg, exp_avg_sq)
    check(_lib.lib().mvae_adam_apply(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                     lr, beta1, beta2, eps, grad_scale, _ptr(step_dev), _stream()),
          'mvae_adam_apply')


def adam_apply_at(param, grad, exp_avg, exp_avg_sq, step_dev, step_add, lr, beta1=0.9, beta2=0.999, eps=1e-8,
                  grad_scale=1.0):
    """Adam at step *step_dev + step_add, counter untouched (step_add 0: it was advanced earlier in the step)."""
    _need_gpu(param, grad, exp_avg, exp_avg_sq, step_dev); _f32c(param, grad, exp_avg, exp_avg_sq)
    check(_lib.lib().mvae_adam_apply_at(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                        lr, beta1, beta2, eps, grad_scale, _ptr(step_dev), int(step_add), _stream()),
          'mvae_adam_apply_at')


def adam_apply_coef(param, grad, exp_avg, exp_avg_sq, coef2, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    """``adam_apply_at(..., step_add=0)`` with the step's bias-correction factors read from ``coef2`` (``adam_prepare``)."""
    _need_gpu(param, grad, exp_avg, exp_avg_sq, coef2); _f32c(param, grad, exp_avg, exp_avg_sq, coef2)
    check(_lib.lib().mvae_adam_apply_coef(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                          _ptr(coef2), beta1, beta2, eps, grad_scale, _stream()), 'mvae_adam_apply_coef')


def adam_prepare(step_dev, delta, lr, beta1, beta2, coef2):
    """*step_dev += delta; coef2[0:2] = Adam's two bias-correction factors at the new step (mvae_adam_prepare)."""
    _need_gpu(step_dev, coef2); _f32c(coef2)
    check(_lib.lib().mvae_adam_prepare(_ptr(step_dev), int(delta), lr, beta1, beta2, _ptr(coef2), _stream()),
          'mvae_adam_prepare')


def trace_marker(tag=0):
    """An empty kernel on the current stream (tools/step_by_shape.py splits a rocprofv3 kernel trace at these)."""
    check(_lib.lib().mvae_trace_marker(int(tag), _stream()), 'mvae_trace_marker')


def counter_add(counter_dev, delta):
    _need_gpu(counter_dev)
    check(_lib.lib().mvae_counter_add(_ptr(counter_dev), int(delta), _stream()), 'mvae_counter_add')


def fill_(out, value):
    _need_gpu(out); _f32c(out)
    check(_lib.lib().mvae_fill(_ptr(out), out.numel(), float(value), _stream()), 'mvae_fill')


def ingest(image_src, image_dst, label_src, label_dst, table_host, table_dst):
    """One launch: image and label batch to their static (graph-visible) buffers, the pinned host table block to
    its device block.  ``table_host`` is a pinned CPU tensor the kernel reads directly."""
    _need_gpu(image_src, image_dst, label_src, label_dst, table_dst)
    if not table_host.is_pinned():
        raise RuntimeError('ingest: the table source must be pinned host memory')
    for a, b in ((image_src, image_dst), (label_src, label_dst), (table_host, table_dst)):
        if a.dtype != b.dtype or a.numel() != b.numel() or not (a.is_contiguous() and b.is_contiguous()):
            raise RuntimeError('ingest: source and destination must be contiguous and alike')
    check(_lib.lib().mvae_ingest(_ptr(image_src), _ptr(image_dst), image_src.numel(),
                                 _ptr(label_src), _ptr(label_dst), label_src.numel() * label_src.element_size(),
                                 _ptr(table_host), _ptr(table_dst), table_host.numel() * table_host.element_size(),
                                 _stream()), 'mvae_ingest')


def ingest_ok(image_src, image_dst, label_src, label_dst):
    """Whether ``ingest`` takes this batch (else: plain copies)."""
    return (image_src.is_cuda and label_src.is_cuda and image_src.dtype == torch.float32 == image_dst.dtype
            and label_src.dtype == label_dst.dtype and image_src.is_contiguous() and label_src.is_contiguous()
            and image_src.numel() == image_dst.numel() and label_src.numel() == label_dst.numel()
            and image_src.numel() % 4 == 0 and (label_src.numel() * label_src.element_size()) % 4 == 0
            and image_src.data_ptr() % 16 == 0 and image_dst.data_ptr() % 16 == 0)


def dropout_fanout_fwd(h, masks, out, scale):
    """h [B,N], masks [G,B,N] -> out [G*B,N]"""
    _need_gpu(h, masks, out); _f32c(h, masks, out)
    G, B, N = masks.shape
    check(_lib.lib().mvae_dropout_fanout_fwd(_ptr(h), _ptr(masks), _ptr(out), scale, G, B, N, _stream()),
          'mvae_dropout_fanout_fwd')


def dropout_fanin_bwd(dout, masks, dh, scale):
    _need_gpu(dout, masks, dh); _f32c(dout, masks, dh)
    G, B, N = masks.shape
    check(_lib.lib().mvae_dropout_fanin_bwd(_ptr(dout), _ptr(masks), _ptr(dh), scale, G, B, N, _stream()),
          'mvae_dropout_fanin_bwd')


def bce_elem_fwd(logits, target, out):
    _need_gpu(logits, target, out); _f32c(logits, target, out)
    check(_lib.lib().mvae_bce_elem_fwd(_ptr(logits), _ptr(target), _ptr(out), logits.numel(), _stream()),
          'mvae_bce_elem_fwd')


def bce_elem_bwd(logits, target, g, dlogits, dtarget=None):
    _need_gpu(logits, target, g, dlogits, dtarget); _f32c(logits, target, g, dlogits, dtarget)
    check(_lib.lib().mvae_bce_elem_bwd(_ptr(logits), _ptr(target), _ptr(g), _ptr(dlogits), _ptr(dtarget),
                                       logits.numel(), _stream()), 'mvae_bce_elem_bwd')


# ---------------------------------------------------------------------------- GRU text stacks (MultiMNIST)
def _rows(t, what, width=None):
    """[rows, width] fp32 GPU view with unit column stride (a column range of a wider buffer is fine)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1):
        raise RuntimeError('%s must be a float32 [rows, width] GPU view with unit column stride' % what)
    if width is not None and t.shape[1] != width:
        raise RuntimeError('%s: width %d, expected %d' % (what, t.shape[1], width))
    return t


def gru_cell_fwd(gi, gh, h_prev, h_new, gates=None):
    B, H = _rows(h_prev, 'h_prev').shape
    _rows(gi, 'gi', 3 * H); _rows(gh, 'gh', 3 * H); _rows(h_new, 'h_new', H)
    if gates is not None:
        _need_gpu(gates); _f32c(gates)
    check(_lib.lib().mvae_gru_cell_fwd(_ptr(gi), gi.stride(0), _ptr(gh), gh.stride(0), _ptr(h_prev), h_prev.stride(0),
                                       _ptr(h_new), h_new.stride(0), _ptr(gates), B, H, _stream()), 'mvae_gru_cell_fwd')


def gru_cell_bwd(dh_new, dh_extra, gates, h_prev, dgi, dgh, dh_prev):
    B, H = _rows(h_prev, 'h_prev').shape
    _rows(dh_new, 'dh_new', H)
    if dh_extra is not None:
        _rows(dh_extra, 'dh_extra', H)
    _need_gpu(gates, dgi, dgh, dh_prev); _f32c(gates, dgi, dgh, dh_prev)
    check(_lib.lib().mvae_gru_cell_bwd(_ptr(dh_new), dh_new.stride(0), _ptr(dh_extra),
                                       0 if dh_extra is None else dh_extra.stride(0), _ptr(gates), _ptr(h_prev),
                                       h_prev.stride(0), _ptr(dgi), _ptr(dgh), _ptr(dh_prev), B, H, _stream()),
          'mvae_gru_cell_bwd')


def _idx64(idx):
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1):
        raise RuntimeError('embedding index must be a 1-D int64 GPU tensor (a column of text[B, L] is fine)')
    return max(int(idx.stride(0)), 1)


def embedding_fwd(idx, w, out, swish=False):
    _need_gpu(w); _f32c(w)
    R, width = _rows(out, 'out', w.shape[1]).shape
    check(_lib.lib().mvae_embedding_fwd(_ptr(idx), _idx64(idx), _ptr(w), _ptr(out), out.stride(0), idx.numel(),
                                        w.shape[0], width, ACT_SWISH if swish else 0, _stream()), 'mvae_embedding_fwd')


def embedding_bwd(idx, w, dout, dw, swish=False, accumulate=False):
    _need_gpu(w, dw); _f32c(w, dw)
    _rows(dout, 'dout', w.shape[1])
    flags = (ACT_SWISH if swish else 0) | (ACCUMULATE if accumulate else 0)
    check(_lib.lib().mvae_embedding_bwd(_ptr(idx), _idx64(idx), _ptr(w), _ptr(dout), dout.stride(0), _ptr(dw),
                                        idx.numel(), w.shape[0], w.shape[1], flags, _stream()), 'mvae_embedding_bwd')


def copy2d(src, dst, mask=None, scale=1.0, accumulate=False):
    rows, cols = _rows(src, 'src').shape
    _rows(dst, 'dst', cols)
    if mask is not None:
        _rows(mask, 'mask', cols)
    check(_lib.lib().mvae_copy2d(_ptr(src), src.stride(0), _ptr(dst), dst.stride(0), _ptr(mask),
                                 0 if mask is None else mask.stride(0), float(scale), rows, cols,
                                 ACCUMULATE if accumulate else 0, _stream()), 'mvae_copy2d')


def argmax_rows(x, out):
    R, K_ = _rows(x, 'x').shape
    if not (out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() == R):
        raise RuntimeError('argmax_rows wants a contiguous int64 GPU output of one entry per row')
    check(_lib.lib().mvae_argmax_rows(_ptr(x), x.stride(0), _ptr(out), R, K_, _stream()), 'mvae_argmax_rows')


# ---------------------------------------------------------------------------- whole-sequence TextDecoder (MultiMNIST)
def gru_dec_seq_supported(B, H, D, n_chars, L):
    """Whether the one-launch decoder kernels take this geometry (host-only query, no GPU needed)."""
    return bool(_lib.lib().mvae_gru_dec_seq_supported(int(B), int(H), int(D), int(n_chars), int(L)))


def _shaped(t, shape, what, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise RuntimeError('%s must be a contiguous %s GPU tensor of shape %s (got %s %s)'
                           % (what, dtype, tuple(shape), t.dtype, tuple(t.shape)))
    return t


def _dec_weights(w_emb, p0, p1, w_h2o, b_h2o, H, D, n_chars):
    _shaped(w_emb, (n_chars, H), 'embed.weight')
    for (w_ih, w_hh, b_ih, b_hh), kx, l in ((p0, H + D, 0), (p1, H, 1)):
        _shaped(w_ih, (3 * H, kx), 'weight_ih_l%d' % l); _shaped(w_hh, (3 * H, H), 'weight_hh_l%d' % l)
        _shaped(b_ih, (3 * H,), 'bias_ih_l%d' % l); _shaped(b_hh, (3 * H,), 'bias_hh_l%d' % l)
    _shaped(w_h2o, (n_chars, H + D), 'h2o.weight'); _shaped(b_h2o, (n_chars,), 'h2o.bias')


def gru_dec_seq_fwd(z, hz, w_emb, p0, p1, w_h2o, b_h2o, masks, mask_scale, words, tape, fed, sos):
    """All ``L`` greedy steps of the 2-layer GRU decoder in one launch.  ``p0`` / ``p1`` = (w_ih, w_hh, b_ih, b_hh) of the
    layers; ``masks`` [L, B, H] or None; ``tape`` = (xcat_all, h0_all, h1_all, d0_all, ocat_all, gates0, gates1) or None;
    ``fed`` [L, B] int64 or None."""
    B, D = z.shape
    H = hz.shape[1]
    _, L, n_chars = words.shape
    _shaped(z, (B, D), 'z'); _shaped(hz, (B, H), 'hz'); _shaped(words, (B, L, n_chars), 'words')
    _dec_weights(w_emb, p0, p1, w_h2o, b_h2o, H, D, n_chars)
    if masks is not None:
        _shaped(masks, (L, B, H), 'masks')
    if tape is not None:
        for t, shape, what in zip(tape, ((L, B, H + D), (L + 1, B, H), (L + 1, B, H), (L, B, H), (L, B, H + D),
                                         (L, B, 4 * H), (L, B, 4 * H)),
                                  ('xcat_all', 'h0_all', 'h1_all', 'd0_all', 'ocat_all', 'gates0', 'gates1')):
            _shaped(t, shape, what)
    if fed is not None:
        _shaped(fed, (L, B), 'fed', torch.int64)
    tp = [_ptr(t) for t in tape] if tape is not None else [None] * 7
    check(_lib.lib().mvae_gru_dec_seq_fwd(_ptr(z), _ptr(hz), _ptr(w_emb), _ptr(p0[0]), _ptr(p0[1]), _ptr(p0[2]),
                                          _ptr(p0[3]), _ptr(p1[0]), _ptr(p1[1]), _ptr(p1[2]), _ptr(p1[3]), _ptr(w_h2o),
                                          _ptr(b_h2o), _ptr(masks), float(mask_scale), _ptr(words), *tp, _ptr(fed),
                                          B, H, D, n_chars, L, int(sos), _stream()), 'mvae_gru_dec_seq_fwd')


def gru_dec_seq_bwd(dwords, p0, p1, w_h2o, masks, mask_scale, h0_all, h1_all, gates0, gates1, dgi0_all, dgh0_all,
                    dgi1_all, dgh1_all, demb_all, dlog_all, dhz, dz):
    """The reverse recurrence of ``gru_dec_seq_fwd`` in one launch: the pre-activation gradients of every step
    (time-stacked), the embedding and logit gradients, and the direct parts of dhz / dz.  No weight gradients."""
    B, L, n_chars = dwords.shape
    H = dhz.shape[1]
    D = dz.shape[1]
    _shaped(dwords, (B, L, n_chars), 'dwords'); _shaped(dhz, (B, H), 'dhz'); _shaped(dz, (B, D), 'dz')
    for (w_ih, w_hh), kx, l in ((p0[:2], H + D, 0), (p1[:2], H, 1)):
        _shaped(w_ih, (3 * H, kx), 'weight_ih_l%d' % l); _shaped(w_hh, (3 * H, H), 'weight_hh_l%d' % l)
    _shaped(w_h2o, (n_chars, H + D), 'h2o.weight')
    if masks is not None:
        _shaped(masks, (L, B, H), 'masks')
    _shaped(h0_all, (L + 1, B, H), 'h0_all'); _shaped(h1_all, (L + 1, B, H), 'h1_all')
    _shaped(gates0, (L, B, 4 * H), 'gates0'); _shaped(gates1, (L, B, 4 * H), 'gates1')
    for t, what in ((dgi0_all, 'dgi0_all'), (dgh0_all, 'dgh0_all'), (dgi1_all, 'dgi1_all'), (dgh1_all, 'dgh1_all')):
        _shaped(t, (L, B, 3 * H), what)
    _shaped(demb_all, (L, B, H), 'demb_all'); _shaped(dlog_all, (L, B, n_chars), 'dlog_all')
    check(_lib.lib().mvae_gru_dec_seq_bwd(_ptr(dwords), _ptr(p0[0]), _ptr(p0[1]), _ptr(p1[0]), _ptr(p1[1]), _ptr(w_h2o),
                                          _ptr(masks), float(mask_scale), _ptr(h0_all), _ptr(h1_all), _ptr(gates0),
                                          _ptr(gates1), _ptr(dgi0_all), _ptr(dgh0_all), _ptr(dgi1_all), _ptr(dgh1_all),
                                          _ptr(demb_all), _ptr(dlog_all), _ptr(dhz), _ptr(dz), B, H, D, n_chars, L,
                                          _stream()), 'mvae_gru_dec_seq_bwd')


# ---------------------------------------------------------------------------- whole-sequence TextEncoder (MultiMNIST)
def gru_enc_seq_supported(B, H, P, n_chars, L, bidirectional):
    """Whether the one-launch encoder kernels take this geometry (host-only query, no GPU needed).  ``P`` is the width
    of ``h2p``'s output, 2 * n_latents."""
    return bool(_lib.lib().mvae_gru_enc_seq_supported(int(B), int(H), int(P), int(n_chars), int(L),
                                                      1 if bidirectional else 0))


def _enc_cell_weights(p, H, sfx, with_bias=True):
    _shaped(p[0], (3 * H, H), 'weight_ih_l0' + sfx); _shaped(p[1], (3 * H, H), 'weight_hh_l0' + sfx)
    if with_bias:
        _shaped(p[2], (3 * H,), 'bias_ih_l0' + sfx); _shaped(p[3], (3 * H,), 'bias_hh_l0' + sfx)


def gru_enc_seq_fwd(x, w_emb, pf, pr, w_h2p, b_h2p, out, tape):
    """The whole TextEncoder in one launch: ``x`` [B, L] int64 -> ``out`` [B, P].  ``pf`` / ``pr`` = (w_ih, w_hh, b_ih,
    b_hh) of the forward / reverse direction (``pr`` None: unidirectional); ``tape`` = (e_all, h_all, gates, gates_r,
    s, idx_all) with ``gates_r`` None exactly when ``pr`` is, or None: nothing but ``out`` is written."""
    B, L = x.shape
    n_chars, H = w_emb.shape
    P = w_h2p.shape[0]
    _shaped(x, (B, L), 'text', torch.int64); _shaped(w_emb, (n_chars, H), 'embed.weight')
    _enc_cell_weights(pf, H, '')
    if pr is not None:
        _enc_cell_weights(pr, H, '_reverse')
    _shaped(w_h2p, (P, H), 'h2p.weight'); _shaped(b_h2p, (P,), 'h2p.bias'); _shaped(out, (B, P), 'out')
    tp = [None] * 6
    if tape is not None:
        e_all, h_all, gates, gates_r, s, idx_all = tape
        _shaped(e_all, (L, B, H), 'e_all'); _shaped(h_all, (L + 1, B, H), 'h_all'); _shaped(gates, (L, B, 4 * H), 'gates')
        if (gates_r is None) != (pr is None):
            raise RuntimeError('gates_r goes with the reverse direction: both or neither')
        if gates_r is not None:
            _shaped(gates_r, (B, 4 * H), 'gates_r')
        _shaped(s, (B, H), 's'); _shaped(idx_all, (L, B), 'idx_all', torch.int64)
        tp = [_ptr(t) for t in tape]
    rp = [_ptr(t) for t in pr] if pr is not None else [None] * 4
    check(_lib.lib().mvae_gru_enc_seq_fwd(_ptr(x), _ptr(w_emb), _ptr(pf[0]), _ptr(pf[1]), _ptr(pf[2]), _ptr(pf[3]), *rp,
                                          _ptr(w_h2p), _ptr(b_h2p), _ptr(out), *tp, B, H, P, n_chars, L, _stream()),
          'mvae_gru_enc_seq_fwd')


def gru_enc_seq_bwd(dout, w_h2p, pf, pr, n_chars, h_all, gates, gates_r, dgi_all, dgh_all, dgi_r, dgh_r, de_all):
    """The reverse recurrence of ``gru_enc_seq_fwd`` in one launch: the time-stacked pre-activation gradients of the
    forward direction, those of the reverse direction's one cell (``pr``, ``gates_r``, ``dgi_r``, ``dgh_r``: all or
    none) and the gradient of the gathered embeddings.  No weight gradients."""
    B, P = dout.shape
    L, _, H = de_all.shape
    _shaped(dout, (B, P), 'dout'); _shaped(w_h2p, (P, H), 'h2p.weight')
    _enc_cell_weights(pf, H, '', with_bias=False)
    _shaped(h_all, (L + 1, B, H), 'h_all'); _shaped(gates, (L, B, 4 * H), 'gates')
    _shaped(dgi_all, (L, B, 3 * H), 'dgi_all'); _shaped(dgh_all, (L, B, 3 * H), 'dgh_all'); _shaped(de_all, (L, B, H), 'de_all')
    rev = (pr, gates_r, dgi_r, dgh_r)
    if any(t is None for t in rev) and not all(t is None for t in rev):
        raise RuntimeError('the reverse direction (parameters, gates_r, dgi_r, dgh_r): all or none')
    if pr is not None:
        _enc_cell_weights(pr, H, '_reverse', with_bias=False)
        _shaped(gates_r, (B, 4 * H), 'gates_r'); _shaped(dgi_r, (B, 3 * H), 'dgi_r'); _shaped(dgh_r, (B, 3 * H), 'dgh_r')
    check(_lib.lib().mvae_gru_enc_seq_bwd(_ptr(dout), _ptr(w_h2p), _ptr(pf[0]), _ptr(pf[1]),
                                          _ptr(pr[0]) if pr is not None else None, _ptr(h_all), _ptr(gates),
                                          _ptr(gates_r), _ptr(dgi_all), _ptr(dgh_all), _ptr(dgi_r), _ptr(dgh_r),
                                          _ptr(de_all), B, H, P, int(n_chars), L, _stream()), 'mvae_gru_enc_seq_bwd')


# ---------------------------------------------------------------------------- importance-weighted log-likelihood (K20)
def iw_draw(mu, logvar, z, lw, eps=None, seed=0, counter_dev=None, counter_offset=0, eps_out=None):
    """``z[Kc, B, D] = mu + exp(0.5 logvar) * eps`` and the density-ratio rows ``lw[Kc, B]`` (mvae_iw_draw).  ``mu`` /
    ``logvar`` are [B, D] with unit column stride and a common row stride (column ranges of a heads buffer qualify).
    ``eps`` [Kc, B, D] replays a host draw; without it the launch generates what ``philox_fill(seed, counter_dev,
    counter_offset)`` would write for a [Kc, B, D] array and (optionally) stores it to ``eps_out``."""
    _need_gpu(mu, logvar, z, lw, eps, counter_dev, eps_out); _f32c(z, lw, eps, eps_out)
    if z.dim() != 3 or mu.dim() != 2 or mu.shape != logvar.shape or tuple(z.shape[1:]) != tuple(mu.shape):
        raise RuntimeError('iw_draw: mu / logvar [B, D] and z [Kc, B, D]; got %s, %s, %s'
                           % (tuple(mu.shape), tuple(logvar.shape), tuple(z.shape)))
    Kc, B, D = z.shape
    for t in (mu, logvar):
        if t.dtype != torch.float32 or (D > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) != mu.stride(0)):
            raise RuntimeError('iw_draw: mu and logvar must be float32 with unit column stride and one row stride')
    ld = mu.stride(0) if B > 1 else max(D, mu.stride(0))
    if lw.numel() != Kc * B:
        raise RuntimeError('iw_draw: lw holds %d values for %d x %d rows' % (lw.numel(), Kc, B))
    for t, what in ((eps, 'eps'), (eps_out, 'eps_out')):
        if t is not None and t.numel() != z.numel():
            raise RuntimeError('iw_draw: %s holds %d values for z of %d' % (what, t.numel(), z.numel()))
    if eps is None and (counter_dev is None or counter_dev.dtype != torch.int64):
        raise RuntimeError('iw_draw: the device draw needs an int64 launch counter on the GPU')
    check(_lib.lib().mvae_iw_draw(_ptr(mu), _ptr(logvar), int(ld), _ptr(eps), int(seed), _ptr(counter_dev),
                                  int(counter_offset), _ptr(eps_out), _ptr(z), _ptr(lw), Kc, B, D, _stream()),
          'mvae_iw_draw')


def iw_accumulate(lw, terms, state, out=None, finish_k=0):
    """Fold the chunk ``lw[Kc, B]`` minus its reconstruction rows into ``state[B, 2]`` (running maximum, running sum of
    exp(. - maximum); start it at (-inf, 0)) -- mvae_iw_accumulate.  ``terms``: up to two ``(rows, rows_per_sample)``
    pairs of loss rows (-log p) in the same sample-major order.  ``finish_k`` = the total number of samples folded so
    far, this chunk included, also writes ``out[b] = logsumexp - log(finish_k)``."""
    _need_gpu(lw, state, out); _f32c(lw, state, out)
    if lw.dim() != 2 or tuple(state.shape) != (lw.shape[1], 2):
        raise RuntimeError('iw_accumulate: lw [Kc, B] and state [B, 2]; got %s and %s' % (tuple(lw.shape), tuple(state.shape)))
    Kc, B = lw.shape
    terms = list(terms)
    if len(terms) > 2:
        raise RuntimeError('iw_accumulate: at most two reconstruction terms per launch')
    args = []
    for rows, rps in terms:
        _need_gpu(rows); _f32c(rows)
        if int(rps) < 1 or rows.numel() != Kc * B * int(rps):
            raise RuntimeError('iw_accumulate: a term holds %d rows for %d x %d samples of %d' % (rows.numel(), Kc, B, rps))
        args += [_ptr(rows), int(rps)]
    args += [None, 0] * (2 - len(terms))
    if finish_k and (out is None or out.numel() != B):
        raise RuntimeError('iw_accumulate: finish needs out [B]')
    check(_lib.lib().mvae_iw_accumulate(_ptr(lw), *args, _ptr(state), _ptr(out), Kc, B, int(finish_k), _stream()),
          'mvae_iw_accumulate')


def iw_score_multi(lw, segs, state, out=None, finish_k=0):
    """The chunk ``lw[Kc, B]`` and the segments ``[(logits [Kc * B, P_s], target [B, P_s])]`` of one decoder pass folded
    into ``state[S + 1, B, 2]``: state s takes ``lw - rec_s`` (the marginal of segment s), state S takes ``lw - (rec_0 +
    ... + rec_{S-1})`` (the joint), ``rec_s`` the BCE-with-logits row sums -- mvae_iw_score_multi (K24).  Start every
    state at (-inf, 0); ``finish_k`` as in ``iw_accumulate``, with ``out`` [S + 1, B]."""
    _need_gpu(lw, state, out); _f32c(lw, state, out)
    segs = [tuple(sg) for sg in segs]
    if lw.dim() != 2 or tuple(state.shape) != (len(segs) + 1, lw.shape[1], 2):
        raise RuntimeError('iw_score_multi: lw [Kc, B] and state [S + 1, B, 2] for S segments; got %s and %s for %d'
                           % (tuple(lw.shape), tuple(state.shape), len(segs)))
    Kc, B = lw.shape
    if any(len(sg) != 2 or sg[1].shape[0] != B for sg in segs):
        raise RuntimeError('iw_score_multi: a segment is (logits [Kc * B, P], target [B, P])')
    arr, _ = _bce_segs([(logits, target, None, 1.0) for logits, target in segs], Kc * B)
    if finish_k and (out is None or tuple(out.shape) != (len(segs) + 1, B)):
        raise RuntimeError('iw_score_multi: finish needs out [S + 1, B]')
    nbytes = _lib.lib().mvae_iw_score_multi_ws_bytes(arr, len(segs), Kc * B)
    ws, ws_bytes = _ws_args(nbytes, lw.device)
    check(_lib.lib().mvae_iw_score_multi(arr, len(segs), _ptr(lw), _ptr(state), _ptr(out), Kc, B, int(finish_k), ws,
                                         ws_bytes, _stream()), 'mvae_iw_score_multi')


# ---------------------------------------------------------------------------- many one-logit modalities (K25)
def heads_bce_rows(h, w0, w_gs, b0, b_gs, target, rec, logits_out=None, target_rows=None):
    """The last layer of G one-logit heads fused with its Bernoulli term (mvae_heads_bce_rows): ``rec[g, r] =
    bce(h[g, r] . w_g + bias_g, target[r % target_rows, g])``.  ``h`` [G, R, H] with unit column stride (the post-Swish
    output of the third grouped Linear); ``w0`` / ``b0``: the weight row (H values) and the bias of group 0, ``w_gs`` /
    ``b_gs`` the strides in floats to the next group's; ``target`` float {0, 1} [>= target_rows, >= G] with unit column
    stride (a column range of a wider matrix qualifies), by default all its rows; ``rec`` and the optional ``logits_out``
    [G, R] with unit column stride."""
    _need_gpu(h, w0, b0, target, rec, logits_out)
    G, R, H = _g3(h, 'h').shape
    for t, name in ((h, 'h'), (w0, 'w0'), (b0, 'b0'), (target, 'target'), (rec, 'rec'), (logits_out, 'logits_out')):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError('heads_bce_rows: %s must be float32, got %s' % (name, t.dtype))
    if w0.numel() != H or not w0.is_contiguous() or b0.numel() != 1:
        raise RuntimeError('heads_bce_rows: w0 holds the %d weights and b0 the bias of group 0; got %s and %s'
                           % (H, tuple(w0.shape), tuple(b0.shape)))
    if target_rows is None:
        target_rows = target.shape[0] if target.dim() == 2 else 0
    if target.dim() != 2 or target.shape[1] < G or (target.shape[1] > 1 and target.stride(1) != 1) \
            or not 1 <= int(target_rows) <= target.shape[0]:
        raise RuntimeError('heads_bce_rows: target must be [>= target_rows, >= %d] with unit column stride, got %s'
                           % (G, tuple(target.shape)))
    ldt = target.stride(0) if target.shape[0] > 1 else max(G, target.stride(0))
    for t, name in ((rec, 'rec'), (logits_out, 'logits_out')):
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (G, R) or (R > 1 and t.stride(1) != 1)
                              or (G > 1 and t.stride(0) < R)):
            raise RuntimeError('heads_bce_rows: %s must be [%d, %d] with unit column stride' % (name, G, R))
    check(_lib.lib().mvae_heads_bce_rows(_ptr(h), h.stride(1), h.stride(0), _ptr(w0), int(w_gs), _ptr(b0), int(b_gs),
                                         _ptr(target), int(target_rows), int(ldt), _ptr(rec), rec.stride(0),
                                         _ptr(logits_out), logits_out.stride(0) if logits_out is not None else 0,
                                         G, R, H, _stream()), 'mvae_heads_bce_rows')


def iw_fold_rows(lw, rec, sel, state, out=None, finish_k=0):
    """The chunk ``lw[Kc, B]`` and the existing loss rows ``rec`` [rows, >= Kc * B] (unit column stride; -log p in
    ``lw``'s sample-major order) folded into ``state[S + 1, B, 2]`` (mvae_iw_fold_rows, K25): state j takes ``lw -
    rec[sel[j]]``, state S takes ``lw - (rec[sel[0]] + ... + rec[sel[S-1]])`` (the joint).  ``sel``: up to
    ``_lib.IW_FOLD_MAX`` row indices of ``rec`` (host ints), None for all rows in order.  Start every state at (-inf, 0);
    ``finish_k`` as in ``iw_accumulate``, with ``out`` [S + 1, B]."""
    _need_gpu(lw, rec, state, out); _f32c(lw, state, out)
    if rec.dtype != torch.float32 or rec.dim() != 2 or (rec.shape[1] > 1 and rec.stride(1) != 1):
        raise RuntimeError('iw_fold_rows: rec must be float32 [rows, >= Kc * B] with unit column stride')
    sel = list(range(rec.shape[0])) if sel is None else [int(s) for s in sel]
    S = len(sel)
    if not 1 <= S <= _lib.IW_FOLD_MAX or any(not 0 <= s < rec.shape[0] for s in sel):
        raise RuntimeError('iw_fold_rows: sel must name 1 to %d of the %d rows of rec, got %s'
                           % (_lib.IW_FOLD_MAX, rec.shape[0], sel))
    if lw.dim() != 2 or tuple(state.shape) != (S + 1, lw.shape[1], 2):
        raise RuntimeError('iw_fold_rows: lw [Kc, B] and state [S + 1, B, 2] for S rows; got %s and %s for %d'
                           % (tuple(lw.shape), tuple(state.shape), S))
    Kc, B = lw.shape
    if rec.shape[1] < Kc * B:
        raise RuntimeError('iw_fold_rows: a row of rec holds %d values for %d x %d samples' % (rec.shape[1], Kc, B))
    rec_ss = rec.stride(0) if rec.shape[0] > 1 else max(Kc * B, rec.stride(0))
    if finish_k and (out is None or tuple(out.shape) != (S + 1, B)):
        raise RuntimeError('iw_fold_rows: finish needs out [S + 1, B]')
    check(_lib.lib().mvae_iw_fold_rows(_ptr(rec), rec_ss, (ctypes.c_int * S)(*sel), S, _ptr(lw), _ptr(state), _ptr(out),
                                       Kc, B, int(finish_k), _stream()), 'mvae_iw_fold_rows')


# ---------------------------------------------------------------------------- PoE of per-row expert selections (K27)
def poe_table_check(table, state, img_heads=None, img_row=None):
    """The host checks of ``poe_table_draw`` on the selection itself, before anything is uploaded or launched: returns
    (state int8 [C, A], img_row int32 [C] or None) as contiguous HOST tensors.  ``ValueError`` names the first defect."""
    if table.dim() != 3 or table.shape[1] != 2 or table.shape[2] % 2 or table.dtype != torch.float32:
        raise ValueError('poe_table_draw: table must be float32 [A, 2, 2D] (expert, input value, mu then logvar), '
                         'got %s %s' % (table.dtype, tuple(table.shape)))
    A, D = table.shape[0], table.shape[2] // 2
    if not 1 <= A <= _lib.POE_TABLE_MAX_A:
        raise ValueError('poe_table_draw: the kernel supports 1 to %d experts in the table, got %d'
                         % (_lib.POE_TABLE_MAX_A, A))
    if D < 1 or A * 4 * D >= 2 ** 31 - 1:
        raise ValueError('poe_table_draw: table of %d experts x %d latents is empty or too large' % (A, D))
    if not torch.is_tensor(state) or state.is_cuda:
        raise ValueError('poe_table_draw: state must be a HOST tensor (it is validated here, then uploaded)')
    if state.dim() != 2 or state.shape[1] != A or state.shape[0] < 1 or state.dtype.is_floating_point \
            or state.dtype == torch.bool:
        raise ValueError('poe_table_draw: state must be an integer tensor [C >= 1, %d], got %s %s'
                         % (A, state.dtype, tuple(state.shape)))
    bad = ((state < -1) | (state > 1)).nonzero()
    if bad.numel():
        c, a = (int(v) for v in bad[0])
        raise ValueError('poe_table_draw: state[%d, %d] = %d is outside {-1 (absent), 0, 1}' % (c, a, int(state[c, a])))
    C = state.shape[0]
    if img_heads is not None and (img_heads.dim() != 2 or img_heads.shape[0] < 1 or img_heads.shape[1] != 2 * D
                                  or img_heads.dtype != torch.float32 or (D > 0 and img_heads.stride(1) != 1)):
        raise ValueError('poe_table_draw: img_heads must be float32 [rows >= 1, %d] with unit column stride, got %s %s'
                         % (2 * D, img_heads.dtype, tuple(img_heads.shape)))
    if img_row is not None:
        if not torch.is_tensor(img_row) or img_row.is_cuda or img_row.dim() != 1 or img_row.shape[0] != C \
                or img_row.dtype.is_floating_point or img_row.dtype == torch.bool:
            raise ValueError('poe_table_draw: img_row must be a HOST integer tensor [%d]' % C)
        rows = img_heads.shape[0] if img_heads is not None else 0
        bad = ((img_row < -1) | (img_row >= max(rows, 0))) & (img_row != -1)
        if bool(bad.any()):
            c = int(bad.nonzero()[0])
            if img_heads is None:
                raise ValueError('poe_table_draw: img_row[%d] = %d names an image row but img_heads is None'
                                 % (c, int(img_row[c])))
            raise ValueError('poe_table_draw: img_row[%d] = %d is outside [-1, %d)' % (c, int(img_row[c]), rows))
        img_row = img_row.to(torch.int32).contiguous()
    elif img_heads is not None:
        raise ValueError('poe_table_draw: img_heads without img_row (which row does each condition use?)')
    return state.to(torch.int8).contiguous(), img_row


def poe_table_draw(table, state, mu, logvar, z=None, img_heads=None, img_row=None, eps=None, seed=0, counter_dev=None,
                   counter_offset=0, eps_out=None):
    """The posterior of C condition rows that each select their own experts, and n draws from each, in one launch
    (mvae_poe_table_draw, K27; PoE variant B with the N(0, 1) prior built in, experts in the order ``infer`` stacks them).

    ``table`` float32 [A, 2, 2D] on the GPU: ``table[a, v]`` = the head of expert a for input value v, mu in the first D
    columns and logvar in the last D.  ``state`` HOST integer [C, A]: -1 absent, 0 / 1 selects ``table[a, state]``;
    ``img_heads`` [rows, 2D] (unit column stride, any row stride) or None with ``img_row`` HOST integer [C]: the image row
    of each condition or -1.  Both are validated on the host (``poe_table_check``) and then uploaded.  Outputs: ``mu``,
    ``logvar`` [C, D] and ``z`` [n, C, D]; ``z=None`` is n = 0 (the posterior only).  ``eps`` [n, C, D] replays a draw;
    without it the launch generates what ``philox_fill(seed, counter_dev, counter_offset)`` would write for an [n, C, D]
    array and (optionally) stores it to ``eps_out``."""
    state, img_row = poe_table_check(table, state, img_heads, img_row)
    A, D = table.shape[0], table.shape[2] // 2
    C = state.shape[0]
    if tuple(mu.shape) != (C, D) or tuple(logvar.shape) != (C, D):
        raise ValueError('poe_table_draw: mu and logvar must be [%d, %d], got %s and %s'
                         % (C, D, tuple(mu.shape), tuple(logvar.shape)))
    n = 0
    if z is not None:
        if z.dim() != 3 or tuple(z.shape[1:]) != (C, D) or z.shape[0] < 1:
            raise ValueError('poe_table_draw: z must be [n >= 1, %d, %d], got %s' % (C, D, tuple(z.shape)))
        n = z.shape[0]
    for t, what in ((eps, 'eps'), (eps_out, 'eps_out')):
        if t is not None and (z is None or tuple(t.shape) != tuple(z.shape)):
            raise ValueError('poe_table_draw: %s must have the shape of z%s' % (what, '' if z is None else ' %s' % (tuple(z.shape),)))
    if n > 8 * 65535:
        raise ValueError('poe_table_draw: at most %d draws per launch, got %d' % (8 * 65535, n))
    if n and eps is None and (counter_dev is None or counter_dev.dtype != torch.int64):
        raise ValueError('poe_table_draw: the device draw needs an int64 launch counter on the GPU')
    _need_gpu(table, mu, logvar, z, img_heads, eps, counter_dev, eps_out); _f32c(table, mu, logvar, z, eps, eps_out)
    dev = table.device
    state_dev = state.to(dev)
    row_dev = img_row.to(dev) if img_heads is not None else None
    ld = 0
    if img_heads is not None:
        ld = img_heads.stride(0) if img_heads.shape[0] > 1 else max(2 * D, img_heads.stride(0))
    check(_lib.lib().mvae_poe_table_draw(_ptr(table), A, _ptr(state_dev), _ptr(img_heads), int(ld),
                                         img_heads.shape[0] if img_heads is not None else 0, _ptr(row_dev), _ptr(eps),
                                         int(seed), _ptr(counter_dev), int(counter_offset), _ptr(eps_out), _ptr(mu),
                                         _ptr(logvar), _ptr(z), n, C, D, _stream()), 'mvae_poe_table_draw')


# ---------------------------------------------------------------------------- MultiMNIST dataset builder
MM_DIGIT,MM_CANVAS, MM_MAX_DIGITS, MM_PLAN_STRIDE = 28, 50, 4, 17     # MVAE_MM_* of include/mvae_hip.h
MM_WMIN, MM_WMAX, MM_KSIZE = 7, 50, 9
_MM_TABLES = {}       # device -> (kk int32 [44, 50, 9], bounds int32 [44, 50, 2]), built once


def multimnist_validate_plan(plan, n_bank):
    """Host check of a compose plan (int32 [M, 17]: n, then four records (bank index, w, top, left)); returns it as a
    contiguous int32 array.  ``ValueError`` names the first defect: the kernel is never given an out-of-range plan."""
    import numpy as np
    plan = np.ascontiguousarray(plan)
    if plan.ndim != 2 or plan.shape[1] != MM_PLAN_STRIDE or plan.shape[0] < 1 or plan.dtype.kind not in 'iu':
        raise ValueError('plan must be an integer array [M >= 1, %d], got %s %s' % (MM_PLAN_STRIDE, plan.dtype, plan.shape))
    plan = plan.astype(np.int64)
    if int(n_bank) < 1:
        raise ValueError('the digit bank is empty')
    n = plan[:, 0]
    if ((n < 0) | (n > MM_MAX_DIGITS)).any():
        raise ValueError('plan: digit count outside 0..%d in canvas %d' % (MM_MAX_DIGITS, int(np.argmax((n < 0) | (n > MM_MAX_DIGITS)))))
    rec = plan[:, 1:].reshape(-1, MM_MAX_DIGITS, 4)
    used = np.arange(MM_MAX_DIGITS)[None, :] < n[:, None]
    ix, w, top, left = (rec[:, :, k] for k in range(4))
    for bad, what in (((ix < 0) | (ix >= int(n_bank)), 'bank index outside 0..%d' % (int(n_bank) - 1)),
                      ((w < MM_WMIN) | (w > MM_WMAX), 'width outside %d..%d' % (MM_WMIN, MM_WMAX)),
                      ((top < 0) | (top + w > MM_CANVAS), 'rows top..top+w outside the %d-pixel canvas' % MM_CANVAS),
                      ((left < 0) | (left + w > MM_CANVAS), 'columns left..left+w outside the %d-pixel canvas' % MM_CANVAS)):
        bad = bad & used
        if bad.any():
            m, d = np.argwhere(bad)[0]
            raise ValueError('plan: %s (canvas %d, digit %d: index %d, w %d, top %d, left %d)'
                             % (what, m, d, ix[m, d], w[m, d], top[m, d], left[m, d]))
    return plan.astype(np.int32)


def _multimnist_tables(device):
    """The fixed-point BILINEAR tables of 28 -> w for every supported width, zero-padded to one shape."""
    import numpy as np
    key = (device.type, device.index)
    if key not in _MM_TABLES:
        from .preprocess import _axis_tables
        kk = np.zeros((MM_WMAX - MM_WMIN + 1, MM_CANVAS, MM_KSIZE), dtype=np.int32)
        bounds = np.zeros((MM_WMAX - MM_WMIN + 1, MM_CANVAS, 2), dtype=np.int32)
        for w in range(MM_WMIN, MM_WMAX + 1):
            k, b, ks = _axis_tables(MM_DIGIT, w)
            if ks > MM_KSIZE or int((b[:, 0] + b[:, 1]).max()) > MM_DIGIT or int(b[:, 1].max()) > ks:
                raise RuntimeError('resample table of 28 -> %d does not fit the compose kernel' % w)
            kk[w - MM_WMIN, :w, :ks] = k
            bounds[w - MM_WMIN, :w] = b
        _MM_TABLES[key] = (torch.from_numpy(kk).to(device), torch.from_numpy(bounds).to(device))
    return _MM_TABLES[key]


def multimnist_compose(bank, plan):
    """Compose ``M`` MultiMNIST canvases in one launch (mvae_multimnist_compose).  ``bank``: uint8 [n_bank, 28, 28] on
    the GPU; ``plan``: host integer array [M, 17] (see ``multimnist_validate_plan`` -- validated here, on the host,
    before anything else).  Returns (canvas uint8 [M, 50, 50], flags int32 [M]) on the GPU: flags is 1 where a pixel
    sum exceeded 255, and the canvas holds min(sum, 255)."""
    if bank.dim() != 3 or tuple(bank.shape[1:]) != (MM_DIGIT, MM_DIGIT) or bank.dtype != torch.uint8:
        raise ValueError('bank must be uint8 [n_bank, 28, 28], got %s %s' % (bank.dtype, tuple(bank.shape)))
    plan = multimnist_validate_plan(plan, bank.shape[0])
    _need_gpu(bank)
    bank = bank.contiguous()
    M = plan.shape[0]
    canvas = torch.empty(M, MM_CANVAS, MM_CANVAS, dtype=torch.uint8, device=bank.device)
    flags = torch.empty(M, dtype=torch.int32, device=bank.device)
    kk, bounds = _multimnist_tables(bank.device)
    plan_dev = torch.from_numpy(plan).to(bank.device)
    check(_lib.lib().mvae_multimnist_compose(_ptr(bank), int(bank.shape[0]), _ptr(plan_dev), M, _ptr(kk), _ptr(bounds),
                                             _ptr(canvas), _ptr(flags), _stream()), 'mvae_multimnist_compose')
    return canvas, flags


# ---------------------------------------------------------------------------- label prediction (K28)
PREDICT_MODES = {'categorical': _lib.PREDICT_CATEGORICAL, 'bernoulli': _lib.PREDICT_BERNOULLI}


def _predict_mode(mode, who):
    if mode not in PREDICT_MODES:
        raise RuntimeError("%s: mode must be 'categorical' or 'bernoulli', got %r" % (who, mode))
    return PREDICT_MODES[mode]


def fresh_predict_state(B, C, mode, device):
    """An empty state for ``predict_fold``: (maximum, sum) = (-inf, 0) per (datum, class) -- [B, C, 2] categorical,
    [B, C, 2, 2] Bernoulli (class 1 first)."""
    _predict_mode(mode, 'fresh_predict_state')
    shape = (int(B), int(C), 2) if mode == 'categorical' else (int(B), int(C), 2, 2)
    state = torch.zeros(shape, dtype=torch.float32, device=device)
    state[..., 0] = float('-inf')
    return state


def predict_fold(logits, B, mode, state, out=None, finish_k=0):
    """Fold the chunk ``logits`` [Kc * B, C] (sample-major rows, row r belongs to datum r % B; any two strides under which
    no two elements alias, so the transpose of a [G, R] block qualifies) into ``state`` (``fresh_predict_state``) --
    mvae_predict_fold.  ``finish_k`` = the total number of samples folded so far, this chunk included, also writes
    ``out`` ([B, C] categorical, [B, C, 2] Bernoulli: log p(1), log p(0)) = logsumexp over the samples - log(finish_k)."""
    code = _predict_mode(mode, 'predict_fold')
    _need_gpu(logits, state, out); _f32c(state, out)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise RuntimeError('predict_fold: logits must be float32 [Kc * B, C], got %s %s' % (logits.dtype, tuple(logits.shape)))
    R, C = logits.shape
    B = int(B)
    tail = (2,) if mode == 'categorical' else (2, 2)
    if B < 1 or R < 1 or R % B != 0 or not 1 <= C <= _lib.PREDICT_MAX_C:
        raise RuntimeError('predict_fold: %d rows of %d logits for %d data (rows a positive multiple of the data, at most '
                           '%d classes)' % (R, C, B, _lib.PREDICT_MAX_C))
    if tuple(state.shape) != (B, C) + tail:
        raise RuntimeError('predict_fold: state must be %s, got %s' % ((B, C) + tail, tuple(state.shape)))
    rs = logits.stride(0) if R > 1 else 1           # an axis of extent 1: torch's stride for it means nothing
    cs = logits.stride(1) if C > 1 else 1
    if rs < 1 or cs < 1 or (rs <= (C - 1) * cs and cs <= (R - 1) * rs):
        raise RuntimeError('predict_fold: the strides %s of logits %s make elements alias' % (logits.stride(), (R, C)))
    if finish_k and (out is None or tuple(out.shape) != (B, C) + tail[1:]):
        raise RuntimeError('predict_fold: finish needs out %s' % ((B, C) + tail[1:],))
    check(_lib.lib().mvae_predict_fold(_ptr(logits), int(rs), int(cs), R, B, C, code, _ptr(state), _ptr(out), int(finish_k),
                                       _stream()), 'mvae_predict_fold')


def predict_score(logp, mode, pred, targets=None, nll=None, correct=None, confusion=None):
    """Predictions from ``predict_fold``'s ``out`` and, with ``targets``, their score (mvae_predict_score): ``pred`` int64,
    ``nll`` float32 and ``correct`` uint8, each [B] categorical / [B, C] Bernoulli; ``targets`` int64 [B] / float {0, 1}
    [B, C] with unit column stride; the counts are ADDED into ``confusion`` (int64 [C, C] (truth, prediction) /
    [C, 2, 2]; zero it once).  A target out of range is counted nowhere (nll = +inf, correct = 0)."""
    code = _predict_mode(mode, 'predict_score')
    _need_gpu(logp, pred, targets, nll, correct, confusion); _f32c(logp, nll)
    cat = mode == 'categorical'
    if logp.dim() != (2 if cat else 3) or (not cat and logp.shape[2] != 2):
        raise RuntimeError('predict_score: logp must be %s, got %s' % ('[B, C]' if cat else '[B, C, 2]', tuple(logp.shape)))
    B, C = logp.shape[:2]
    if B < 1 or not 1 <= C <= _lib.PREDICT_MAX_C:
        raise RuntimeError('predict_score: %d data of %d classes (at most %d)' % (B, C, _lib.PREDICT_MAX_C))
    shape = (B,) if cat else (B, C)
    for t, name, dtype in ((pred, 'pred', torch.int64), (nll, 'nll', torch.float32), (correct, 'correct', torch.uint8)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
            raise RuntimeError('predict_score: %s must be a contiguous %s %s' % (name, dtype, shape))
    if pred is None:
        raise RuntimeError('predict_score: pred is required')
    ldt = 0
    if targets is None:
        if nll is not None or correct is not None or confusion is not None:
            raise RuntimeError('predict_score: nll, correct and confusion need targets')
    else:
        if nll is None or correct is None:
            raise RuntimeError('predict_score: targets need nll and correct')
        if cat:
            if targets.dtype != torch.int64 or tuple(targets.shape) != (B,) or not targets.is_contiguous():
                raise RuntimeError('predict_score: categorical targets must be a contiguous int64 [%d]' % B)
        else:
            if targets.dtype != torch.float32 or tuple(targets.shape) != (B, C) or (C > 1 and targets.stride(1) != 1) \
                    or (B > 1 and targets.stride(0) < C):
                raise RuntimeError('predict_score: Bernoulli targets must be float32 [%d, %d] with unit column stride' % (B, C))
            ldt = targets.stride(0) if B > 1 else max(C, targets.stride(0))
        want = (C, C) if cat else (C, 2, 2)
        if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != want
                                      or not confusion.is_contiguous()):
            raise RuntimeError('predict_score: confusion must be a contiguous int64 %s' % (want,))
    check(_lib.lib().mvae_predict_score(_ptr(logp), code, _ptr(targets), int(ldt), B, C, _ptr(pred), _ptr(nll),
                                        _ptr(correct), _ptr(confusion), _stream()), 'mvae_predict_score')
