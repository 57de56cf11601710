"""No GPU: the host side of the MultiMNIST MVAE -- the general stride-2 conv family's ABI and predicate, plan
compilation of the 50 x 50 image stacks, the reference's state_dict keys / parser defaults / function signatures (from
the golden captured from the unmodified reference, tests/golden/make_multimnist_mvae_golden.py)."""
import ctypes
import inspect

import pytest
import torch

import mvae_amd
from mvae_amd import _lib, kernels as K, layers as L
from mvae_amd.multimnist import model as MM, train as MT
from util import load_golden

GEN_SYMBOLS = ['mvae_conv2d_gen_fwd', 'mvae_conv2d_gen_dgrad', 'mvae_conv2d_gen_wgrad', 'mvae_convT2d_gen_fwd',
               'mvae_convT2d_gen_dgrad', 'mvae_convT2d_gen_wgrad', 'mvae_conv_gen_ws_bytes', 'mvae_conv_gen_supported']

# the four geometries of multimnist/model.py the 4x4 family refuses: (transposed, Cin, H, Cout, ks, pad)
MM_GEOMETRIES = [(False, 32, 25, 64, 4, 1), (False, 128, 6, 256, 4, 0), (True, 256, 2, 128, 4, 0), (True, 64, 12, 32, 5, 1)]


def test_library_exports_the_gen_symbols():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in GEN_SYMBOLS:
        assert name in _lib._SIGNATURES and hasattr(handle, name), name
    assert _lib.lib().mvae_abi_version() == 6


def test_conv_gen_supported_answers_on_the_host():
    for transposed, Cin, H, Cout, ks, pad in MM_GEOMETRIES:
        for B in (1, 100, 512):
            assert K.conv_gen_supported(transposed, B, Cin, H, H, Cout, ks, 2, pad), (transposed, Cin, H, Cout, ks, pad)
    assert K.conv_gen_supported(False, 2, 3, 9, 11, 5, 4, 2, 1) and K.conv_gen_supported(True, 2, 6, 1, 1, 4, 4, 2, 0)
    for transposed in (False, True):
        assert not K.conv_gen_supported(transposed, 2, 3, 8, 8, 4, 3, 2, 1)      # ks = 3
        assert not K.conv_gen_supported(transposed, 2, 3, 8, 8, 4, 4, 1, 1)      # stride 1
        assert not K.conv_gen_supported(transposed, 2, 3, 8, 8, 4, 4, 2, 2)      # pad 2
        assert not K.conv_gen_supported(transposed, 0, 3, 8, 8, 4, 4, 2, 1)      # empty batch
    assert not K.conv_gen_supported(False, 2, 3, 2, 8, 4, 4, 2, 0)               # H + 2 pad < ks
    assert not K.conv_gen_supported(False, 2, 3, 8, 3, 4, 5, 2, 0)               # W + 2 pad < ks
    assert not K.conv_gen_supported(False, 1 << 12, 64, 64, 64, 64, 4, 2, 1)     # 2^30 input elements: 32-bit byte offsets
    lib = _lib.lib()
    # refused on the host before any launch; scratch: the weight gradients' partial slabs, the parity-form launches' weight copy
    assert lib.mvae_conv2d_gen_fwd(None, None, None, None, 1, 32, 25, 25, 64, 4, 2, 1, None) == -1
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mvae_conv2d_gen_fwd(p, p, p, None, 1, 1, 8, 8, 1, 3, 2, 1, None) == -1
    assert lib.mvae_convT2d_gen_wgrad(p, p, p, 1, 1, 8, 8, 1, 4, 1, 1, 0, None, 0, None) == -1
    assert lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['conv_fwd'], 100, 32, 25, 25, 64, 4, 2, 1) == 0
    assert lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['convT_dgrad'], 100, 64, 12, 12, 32, 5, 2, 1) == 0
    assert lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['conv_dgrad'], 100, 32, 25, 25, 64, 4, 2, 1) == 64 * 32 * 16 * 4
    assert lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['convT_fwd'], 100, 64, 12, 12, 32, 5, 2, 1) == 64 * 32 * 25 * 4
    assert lib.mvae_convT2d_gen_fwd(p, p, p, None, 1, 2, 3, 3, 2, 5, 2, 1, None, 0, None) == -3      # MVAE_ERR_WS: no room for the copy
    n = lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['conv_wgrad'], 100, 32, 25, 25, 64, 4, 2, 1)
    assert n > 0 and n % (64 * 32 * 16 * 4) == 0                                  # whole partial slabs of dw
    assert lib.mvae_conv_gen_ws_bytes(_lib.CONV_OPS['conv_wgrad'], 100, 32, 25, 25, 64, 3, 2, 1) == 0


def test_plans_compile_for_both_image_stacks_and_still_refuse_the_rest():
    enc, dec = MM.ImageEncoder(64), MM.ImageDecoder(64)
    assert [(op.kind, op.act, op.drop) for op in enc.plan()] == [
        ('conv', True, 0.0), ('conv', False, 0.0), ('bn', True, 0.0), ('conv', False, 0.0), ('bn', True, 0.0),
        ('conv', False, 0.0), ('bn', True, 0.0), ('view', False, 0.0), ('lin', True, 0.1), ('lin', False, 0.0)]
    assert [(op.kind, op.act) for op in dec.plan()] == [
        ('lin', True), ('view', False), ('convT', False), ('bn', True), ('convT', False), ('bn', True),
        ('convT', False), ('bn', True), ('convT', False)]
    with pytest.raises(RuntimeError, match='general stride-2'):
        L.compile_plan([L.Conv2d(3, 8, 3, 1, 1, bias=False)])
    with pytest.raises(RuntimeError, match='general stride-2'):
        L.compile_plan([L.Conv2d(3, 8, 5, 1, 0, bias=False)])
    with pytest.raises(RuntimeError, match='4x4'):
        L.compile_plan([L.ConvTranspose2d(3, 8, 5, 2, 1, bias=True)])
    # per launch: what the 4x4 family admits stays there; odd maps, pad 0 and 5x5 go to the general family
    k4 = [L._k4_launch(op, h, h) for op, h in zip([o for o in enc.plan() if o.kind == 'conv'], (50, 25, 12, 6))]
    assert k4 == [True, False, True, False]
    k4 = [L._k4_launch(op, h, h) for op, h in zip([o for o in dec.plan() if o.kind == 'convT'], (2, 6, 12, 25))]
    assert k4 == [False, True, False, True]
    for m in (mvae_amd.celeba.model.MVAE(8), mvae_amd.fashionmnist.model.MVAE(8)):
        for stack in (m.image_encoder, m.image_decoder):
            assert all(L._k4_module(op.mod) for op in stack.plan() if op.kind in ('conv', 'convT'))


def test_state_dict_keys_and_shapes_equal_the_reference(golden_dir):
    fx, meta = load_golden(golden_dir, 'multimnist_mvae_b6')
    model = MM.MVAE(meta['n_latents'])
    mine = ['%s %s' % (k, 'x'.join(str(d) for d in v.shape)) for k, v in model.state_dict().items()]
    assert sorted(mine) == sorted(str(s) for s in fx['state_keys'])
    assert sum(p.numel() for p in model.parameters()) == 3103988      # SURVEY: 3.10 M
    for name in ('image_encoder', 'image_decoder', 'text_encoder', 'text_decoder', 'experts', 'n_latents'):
        assert hasattr(model, name)
    assert isinstance(model.experts, MM.ProductOfExperts) and model.n_latents == meta['n_latents']
    with pytest.raises(RuntimeError, match='GPU'):
        model(torch.zeros(2, 1, 50, 50), torch.zeros(2, 4, dtype=torch.long))


def test_train_parser_defaults_equal_the_reference(golden_dir):
    fx, _ = load_golden(golden_dir, 'multimnist_mvae_b6')
    args = MT.parser().parse_args([])
    want = [str(s).split(' ', 1) for s in fx['parser_defaults']]
    assert [f for f, _ in want] == ['--n-latents', '--batch-size', '--epochs', '--annealing-epochs', '--lr',
                                    '--log-interval', '--lambda-image', '--lambda-text', '--cuda']
    for flag, default in want:
        got = getattr(args, flag[2:].replace('-', '_'))
        assert repr(got) == default and type(got).__name__ == type(eval(default)).__name__, (flag, got, default)
    for extra in ('synthetic', 'steps_per_epoch', 'synthetic_last_batch', 'out_dir'):
        assert hasattr(args, extra)
    with pytest.raises(SystemExit, match='dataset builder'):      # without --synthetic: a clear message, before anything else
        MT.main([])


def test_module_level_names_have_the_references_signatures():
    sig = inspect.signature(MT.elbo_loss)
    assert list(sig.parameters) == ['recon_image', 'image', 'recon_text', 'text', 'mu', 'logvar', 'lambda_image',
                                    'lambda_text', 'annealing_factor']
    assert [sig.parameters[k].default for k in ('lambda_image', 'lambda_text', 'annealing_factor')] == [1.0, 1.0, 1]
    assert list(inspect.signature(MT.binary_cross_entropy_with_logits).parameters) == ['input', 'target']
    ce = inspect.signature(MT.cross_entropy)
    assert list(ce.parameters) == ['input', 'target', 'eps'] and ce.parameters['eps'].default == 1e-6
    assert list(inspect.signature(MT.save_checkpoint).parameters) == ['state', 'is_best', 'folder', 'filename']
    lc = inspect.signature(MT.load_checkpoint)
    assert list(lc.parameters) == ['file_path', 'use_cuda'] and lc.parameters['use_cuda'].default is False
    m = MT.AverageMeter(); m.update(2.0, 3); m.update(4.0, 1)
    assert (m.val, m.sum, m.count, m.avg) == (4.0, 10.0, 4, 2.5)
    with pytest.raises(RuntimeError, match='GPU'):
        MT.elbo_loss(None, None, None, None, torch.zeros(2, 8), torch.zeros(2, 8))
