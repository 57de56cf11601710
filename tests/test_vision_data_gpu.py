"""GPU: the vision input pipeline -- ``preprocess.VisionCompose`` (csrc/vision_data.hip, one launch for the six
modalities) against the Pillow golden, and ``CelebVisionLoader`` (host decode, one upload per source, one launch per
batch) against the per-item Pillow path of ``CelebVision``.  Integer work and one IEEE division, ``1.0f - q`` for the
mask: equality, no tolerance."""
import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import preprocess as PP
from mvae_amd.vision import datasets as VD, model as VM
import vision_data_ref as R
from test_vision_data_cpu import make_vision_tree
from util import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return load_golden(golden_dir, 'vision_data')[0]


@pytest.mark.parametrize('name,with_gray', R.golden_runs())
def test_vision_compose_equals_the_pillow_golden(golden, name, with_gray):
    x = R.case_inputs(name)
    H, W, S, B, _ = R.CASES[name]
    dev = {k: torch.from_numpy(x[k]).to(DEV) for k in ('rgb', 'edge', 'mask', 'gray', 'mark')}
    out = PP.VisionCompose(S)(dev['rgb'], dev['edge'], dev['mask'], dev['mark'], gray=dev['gray'] if with_gray else None)
    want = R.to_float([golden[R.golden_key(name, m, with_gray)] for m in R.MODALITIES])
    assert len(out) == 6
    for m, modality in enumerate(VM.MODALITIES):
        got = out[m].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (B, VM.N_CHANNELS[modality], S, S)
        assert np.array_equal(got, want[m]), '%s %s: %d of %d values differ' % (name, modality, (got != want[m]).sum(),
                                                                                  got.size)


def test_vision_compose_takes_misaligned_bases_and_a_cached_plan(golden):
    """Views one byte into a larger buffer: every source base is odd.  The second call reuses the cached plan."""
    name = 'tall'
    x = R.case_inputs(name)
    S = R.CASES[name][2]

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
        buf[1:] = torch.from_numpy(a.ravel()).to(DEV)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 2 == 1 and v.is_contiguous()
        return v
    op = PP.VisionCompose(S)
    want = R.to_float([golden[R.golden_key(name, m, True)] for m in R.MODALITIES])
    for _ in range(2):
        out = op(*[shifted(x[k]) for k in ('rgb', 'edge', 'mask', 'mark')], gray=shifted(x['gray']))
        for m in range(6):
            assert np.array_equal(out[m].cpu().numpy(), want[m]), VM.MODALITIES[m]
    assert len(op._resize._tables) == 1


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('vision_tree'))
    names, mark_path = make_vision_tree(root, counts=(5, 0, 0), hw=(23, 17), seed=6)
    return root, names, mark_path


@pytest.mark.parametrize('gray', ['folder', 'rgb'])
def test_loader_batches_equal_the_per_item_dataset(tree, gray):
    root, names, mark_path = tree
    ds = VD.CelebVision('train', root, watermark_path=mark_path, gray=gray, size=8)
    loader = VD.CelebVisionLoader('train', root, 2, False, torch.device(DEV), watermark_path=mark_path, gray=gray, size=8)
    assert len(loader) == 3 and len(loader.dataset) == 5
    seen, sizes = 0, []
    for batch6 in loader:
        assert len(batch6) == 6
        sizes.append(batch6[0].shape[0])
        for m, modality in enumerate(VM.MODALITIES):
            assert batch6[m].is_cuda and batch6[m].dtype == torch.float32
            assert tuple(batch6[m].shape[1:]) == (VM.N_CHANNELS[modality], 8, 8)
        host = [t.cpu() for t in batch6]
        for i in range(sizes[-1]):
            item = ds[seen + i]
            for m, modality in enumerate(VM.MODALITIES):
                assert torch.equal(host[m][i], item[m]), 'item %d %s' % (seen + i, modality)
        seen += sizes[-1]
    assert sizes == [2, 2, 1] and seen == 5
    assert len(loader._marks) == 1                                   # the watermark was resized and uploaded once


def test_shuffled_loader_is_a_permutation_of_the_items(tree):
    root, names, mark_path = tree
    dev = torch.device(DEV)
    plain = torch.cat([b[0] for b in VD.CelebVisionLoader('train', root, 2, False, dev, watermark_path=mark_path, size=8)])
    a = VD.CelebVisionLoader('train', root, 2, True, dev, seed=3, watermark_path=mark_path, size=8)
    b = VD.CelebVisionLoader('train', root, 2, True, dev, seed=3, watermark_path=mark_path, size=8)
    first, again = torch.cat([x[0] for x in a]), torch.cat([x[0] for x in b])
    assert torch.equal(first, again) and first.shape == plain.shape
    order = [next(i for i in range(5) if torch.equal(first[k], plain[i])) for k in range(5)]
    assert sorted(order) == list(range(5))
    epochs = [order, [next(i for i in range(5) if torch.equal(img, plain[i])) for img in torch.cat([x[0] for x in a])]]
    assert sorted(epochs[1]) == list(range(5))
    assert any(o != list(range(5)) for o in epochs)                  # two seeded permutations of five, not both the identity


def test_loader_refuses_images_of_different_sizes(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    names, mark_path = make_vision_tree(root, counts=(2, 0, 0), hw=(23, 17), seed=8)
    Image.fromarray(np.zeros((17, 23), dtype=np.uint8)).save(str(tmp_path / VD.EDGE_DIR / names[0][1]))
    loader = VD.CelebVisionLoader('train', root, 2, False, torch.device(DEV), watermark_path=mark_path, size=8)
    with pytest.raises(ValueError, match='differ in size'):
        next(iter(loader))
