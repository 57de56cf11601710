"""CPU: the vision experiment's surface (vision/model.py, vision/train.py) against the facts recorded from the
reference in tests/golden/vision_b4.npz, the plain-torch restatement against the recorded seven-term step, and the
host-side refusals of the segmented BCE entry points (no launch happens: there is no GPU here)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib
from mvae_amd.vision import model as VM, train as VT
from oracle import models as OM
import vision_ref as R
from util import load_golden

ELBO_NAMES = ['recon_image', 'image', 'recon_gray', 'gray', 'recon_edge', 'edge', 'recon_mask', 'mask',
              'recon_obscured', 'obscured', 'recon_watermark', 'watermark', 'mu', 'logvar', 'annealing_factor']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return load_golden(golden_dir, 'vision_b4')


def test_restatement_reproduces_the_golden_step(golden):
    fx, meta = golden
    model = OM.fill_parameters(R.MVAE(meta['n_latents']), meta['model_seed']).train()
    batch6 = R.synthetic_batch(meta['batch'], meta['batch_seed'])
    noise = R.draw_step_noise(meta['batch'], meta['n_latents'], torch.Generator().manual_seed(meta['noise_seed']))
    total, terms, _ = R.seven_term_step(model, batch6, noise, meta['annealing_factor'])
    total.backward()
    assert abs(total.item() - float(fx['total'])) <= 1e-5 * abs(float(fx['total']))
    assert np.allclose([t.item() for t in terms], fx['terms'], rtol=1e-5, atol=0)
    for name, p in model.named_parameters():
        ref = float(fx['gnorm/' + name])
        assert abs(p.grad.double().norm().item() - ref) <= 1e-4 * max(ref, 1e-30), name
    for name, b in model.named_buffers():
        if name.endswith('num_batches_tracked'):
            assert int(b) == int(fx['nbt/' + name]) == (2 if '_encoder.' in name else 7), name
        else:
            assert np.allclose(b.numpy(), fx['buf/' + name], rtol=1e-5, atol=1e-7), name


def test_state_dict_keys_shapes_and_count_equal_the_reference(golden):
    fx, _ = golden
    assert int(fx['n_params_250']) == 39119160
    model = VM.MVAE()
    assert model.n_latents == 250
    mine = ['%s %s' % (k, 'x'.join(str(d) for d in v.shape)) for k, v in model.state_dict().items()]
    assert mine == list(fx['state_keys'])
    assert sum(p.numel() for p in model.parameters()) == int(fx['n_params_250'])
    # the twelve stacks and their channel counts, as vision/model.py:16-28 assigns them
    pairs = [s.split() for s in fx['attr_pairs']]
    assert [p[0] for p in pairs] == [n for n, _ in model.named_children() if n != 'experts']
    for name, kind, c in pairs:
        stack = getattr(model, name)
        assert type(stack).__name__ == 'Image' + kind
        first_or_last = stack.features[0].in_channels if kind == 'Encoder' else stack.hallucinate[-1].out_channels
        assert first_or_last == int(c) == VM.N_CHANNELS[name.split('_')[0]], name
    # the restatement carries the same keys (it is what the GPU tests load into the HIP modules)
    assert list(R.MVAE(250).state_dict().keys()) == list(model.state_dict().keys())


def test_parser_defaults_equal_the_reference(golden):
    fx, _ = golden
    args = VT.parser().parse_args([])
    recorded = dict(s.split(' ', 1) for s in fx['parser_defaults'])
    assert sorted(recorded) == ['--annealing-epochs', '--batch-size', '--cuda', '--epochs', '--log-interval', '--lr',
                                '--n-latents']
    for flag, default in recorded.items():
        assert repr(getattr(args, flag[2:].replace('-', '_'))) == default, flag
    assert args.step in ('eager', 'fused') and args.step == VT.DEFAULT_STEP


def test_reference_surface_names_and_signatures():
    assert list(inspect.signature(VT.elbo_loss).parameters) == ELBO_NAMES
    assert inspect.signature(VT.elbo_loss).parameters['annealing_factor'].default == 1.
    assert list(inspect.signature(VM.MVAE.forward).parameters)[1:] == [
        'image', 'gray', 'edge', 'mask', 'obscured', 'watermark', 'eps', 'dropout_masks']
    assert list(inspect.signature(VM.MVAE.get_params).parameters)[1:] == ['image', 'gray', 'edge', 'mask', 'obscured',
                                                                          'watermark']
    assert list(inspect.signature(VM.MVAE.__init__).parameters)[1:] == ['n_latents', 'use_cuda']
    assert list(inspect.signature(VM.ImageEncoder.__init__).parameters)[1:] == ['n_latents', 'n_channels']
    assert inspect.signature(VM.ImageDecoder.__init__).parameters['n_channels'].default == 3
    for name in ('MVAE', 'ImageEncoder', 'ImageDecoder', 'ProductOfExperts', 'Swish', 'prior_expert', 'get_batch_size'):
        assert hasattr(VM, name), name
    assert VM.ProductOfExperts.VARIANT == 'A' and VM.MVAE.infer is VM.MVAE.get_params
    assert VM.get_batch_size(None, torch.zeros(3, 2)) == 3
    for name in ('train_step', 'fused_step', 'load_checkpoint', 'save_checkpoint', 'AverageMeter',
                 'binary_cross_entropy_with_logits'):
        assert hasattr(VT, name), name
    m = VM.MVAE(8)
    with pytest.raises(RuntimeError, match='GPU'):
        m(gray=torch.zeros(2, 1, 64, 64))
    with pytest.raises(RuntimeError, match='GPU'):
        VT.elbo_loss(*([None] * 12), torch.zeros(2, 8), torch.zeros(2, 8))


def test_train_cli_exits_without_data_or_gpu():
    with pytest.raises(SystemExit, match='out of scope'):
        VT.main([])
    with pytest.raises(SystemExit, match='pass --cuda'):
        VT.main(['--synthetic'])


def _segs(n, P=8, logits=True, target=True):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (_lib.BceSeg * max(n, 1))()
    for s in range(n):
        arr[s] = _lib.BceSeg(p if logits else None, p if target else None, p, P, 1.0)
    return arr, p, buf


def test_bce_multi_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    arr, p, _keep = _segs(2)
    big = ctypes.c_size_t(1 << 20)

    def fwd(a=arr, n=2, rowsum=p, drow=p, R=4, rpg=2, trows=2, ws=p, ws_bytes=big):
        return lib.mvae_bce_multi_fwd(a, n, rowsum, drow, R, rpg, trows, ws, ws_bytes, None)

    def bwd(a=arr, n=2, drow=p, R=4, rpg=2, trows=2):
        return lib.mvae_bce_multi_bwd(a, n, drow, R, rpg, trows, None)

    for call in (fwd, bwd):
        assert call(a=None) == -1                                     # null table
        assert call(n=0) == -1 and call(n=9) == -1                    # n_segs outside 1..8
        assert call(a=_segs(2, logits=False)[0]) == -1                # null logits
        assert call(a=_segs(2, target=False)[0]) == -1                # null target
        assert call(a=_segs(2, P=0)[0]) == -1 and call(a=_segs(2, P=-4)[0]) == -1
        assert call(R=0) == -1 and call(R=-1) == -1
        assert call(R=4, rpg=3) == -1 and call(rpg=0) == -1           # R % rows_per_group != 0
        assert call(trows=0) == -1
    assert bwd(drow=None) == -1                                       # a gradient needs d loss / d rowsum
    assert fwd(rowsum=None, drow=None) == -1                          # nothing to write
    need = lib.mvae_bce_multi_ws_bytes(arr, 2, 4)
    assert fwd(ws_bytes=ctypes.c_size_t(need - 1)) == -3 and fwd(ws_bytes=ctypes.c_size_t(0)) == -3   # scratch too small
    assert fwd(ws=None) == -1                                         # enough bytes promised, no buffer
    assert _lib.BCE_MULTI_MAX == 8


def test_bce_multi_ws_bytes_is_a_pure_host_call():
    lib = _lib.lib()
    arr, _, _keep = _segs(2, P=8)
    assert lib.mvae_bce_multi_ws_bytes(arr, 2, 4) == 4 * 2 * 4                 # one chunk per short segment
    vis, _, _keep2 = _segs(6)
    for s, P in enumerate((12288, 4096, 4096, 4096, 12288, 12288)):
        vis[s].P = P
    per_row = lib.mvae_bce_multi_ws_bytes(vis, 6, 1)
    assert per_row % 4 == 0 and per_row // 4 >= 6                              # at least one partial per segment ...
    assert per_row // 4 > 6, 'a 49,152-element row must be split across more blocks than it has segments'
    assert lib.mvae_bce_multi_ws_bytes(vis, 6, 350) == 350 * per_row           # ... and linear in R
    vis[3].P = 4097
    assert lib.mvae_bce_multi_ws_bytes(vis, 6, 1) > per_row                    # a ragged tail is a chunk of its own
    assert lib.mvae_bce_multi_ws_bytes(None, 1, 4) == 0 and lib.mvae_bce_multi_ws_bytes(arr, 0, 4) == 0
    assert lib.mvae_bce_multi_ws_bytes(arr, 2, 0) == 0
