"""No GPU: the host side of the vision data path -- the numpy restatement of the six-modality pipeline against the Pillow
golden (and Pillow live), ``vision/datasets.py``'s host functions and ``CelebVision`` on a tree of lossless PNGs, the
refusals of ``mvae_vision_compose`` and ``preprocess.VisionCompose`` before any launch, and ``train.py`` up to the point
where it needs the data or a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib, preprocess as PP
from mvae_amd.vision import datasets as VD, model as VM, train as VT
import vision_data_ref as R
from util import load_golden

Image = pytest.importorskip('PIL.Image')
FOLDERS = (VD.IMAGE_DIR, VD.GRAY_DIR, VD.EDGE_DIR, VD.MASK_DIR)


def make_vision_tree(root, counts=(5, 0, 0), hw=(23, 17), seed=0, mark_hw=(6, 10)):
    """A data dir as the reference's vision/setup.py leaves it, of lossless PNGs so that the decoded bytes are known:
    ``counts`` files per partition (train, val, test), the four image folders (the gray files are NOT the luma of the
    colour files) and an RGBA ``watermark.png``.  Returns (names by partition, the watermark's path)."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'Eval'))
    for d in FOLDERS:
        os.makedirs(os.path.join(root, d))
    names, lines = {0: [], 1: [], 2: []}, []
    for part, n in enumerate(counts):
        for i in range(n):
            name = '%06d.png' % (len(lines) + 1)
            names[part].append(name)
            lines.append('%s %d' % (name, part))
            for d in FOLDERS:
                shape = hw + (3,) if d == VD.IMAGE_DIR else hw
                Image.fromarray(rng.randint(0, 256, shape).astype(np.uint8)).save(os.path.join(root, d, name))
    with open(os.path.join(root, VD.PARTITION_FILE), 'w') as fp:
        fp.write('\n'.join(lines) + '\n')
    mark = rng.randint(0, 256, mark_hw + (4,)).astype(np.uint8)
    mark_path = os.path.join(root, 'watermark.png')
    Image.fromarray(mark, 'RGBA').save(mark_path)
    return names, mark_path


def restated_item(root, name, mark_path, from_folder, size):
    """The six float32 [C, size, size] arrays of one file of the tree by the restatement (the mark resized by Pillow)."""
    def read(d, mode):
        return np.asarray(Image.open(os.path.join(root, d, name)).convert(mode), dtype=np.uint8)
    rgb, edge, mask = read(VD.IMAGE_DIR, 'RGB'), read(VD.EDGE_DIR, 'L'), read(VD.MASK_DIR, 'L')
    gray = read(VD.GRAY_DIR, 'L') if from_folder else None
    mark = np.asarray(Image.open(mark_path).resize((rgb.shape[1], rgb.shape[0]), Image.BICUBIC), dtype=np.uint8)
    six = R.compose(rgb[None], edge[None], mask[None], mark, None if gray is None else gray[None], size)
    return [v[0] for v in six]


# ----------------------------------------------------------------------------- restatement
def test_restatement_reproduces_the_pillow_golden(golden_dir):
    fx, meta = load_golden(golden_dir, 'vision_data')
    assert meta['cases'] == R.CASES and meta['gray_twice'] == R.GRAY_TWICE
    assert len(fx) == 6 * len(R.golden_runs())
    for name, with_gray in R.golden_runs():
        x = R.case_inputs(name)
        H, W, S, B, _ = R.CASES[name]
        got = R.compose_u8(x['rgb'], x['edge'], x['mask'], x['mark'], x['gray'] if with_gray else None, S)
        for m, modality in enumerate(R.MODALITIES):
            want = fx[R.golden_key(name, modality, with_gray)]
            assert want.dtype == np.uint8 and want.shape == (B, VM.N_CHANNELS[modality], S, S)
            assert np.array_equal(got[m], want), (name, modality, with_gray)
    assert tuple(R.MODALITIES) == tuple(VM.MODALITIES)


def test_golden_cases_hold_what_they_are_named_for():
    from mvae_amd.preprocess import center_crop_origin, resized_size
    tops = {}
    for name, (H, W, S, B, _) in R.CASES.items():
        tops[name] = center_crop_origin(*resized_size(H, W, S), S)
        x = R.case_inputs(name)
        assert not np.array_equal(x['gray'], R.luma(x['rgb']))
        if B > 1:
            assert not np.array_equal(x['rgb'][0], x['rgb'][1])
    assert tops['tall'] == (1, 0) and tops['wide'][0] == 0 and tops['wide'][1] > 0
    assert tops['unit'] == (0, 0) and tops['one_row'][1] == 0
    H, W, S, B, _ = R.CASES['tall']
    assert (H * W) % 2 == 1 and (H * W) % 4 != 0 and (2 * H * W) % 4 != 0 and B == 3      # images 1, 2 start misaligned
    x = R.case_inputs('tall')
    alpha = set(x['mark'][..., 3].ravel().tolist())
    assert {0, 255, 128} <= alpha
    for r in range(6):          # every (dst, src) in {0, 255}^2 under each alpha row
        pairs = {(int(d), int(s)) for d, s in zip(x['rgb'][0, r, :, 0], x['mark'][r, :, 0])}
        assert pairs == {(0, 0), (0, 255), (255, 0), (255, 255)}, r


def test_restatement_matches_pillow_live():
    rng = np.random.RandomState(9)
    rgb = rng.randint(0, 256, (31, 47, 3)).astype(np.uint8)
    mark = rng.randint(0, 256, (31, 47, 4)).astype(np.uint8)
    mark[:4, :, 3] = 0; mark[4:8, :, 3] = 255
    image = Image.fromarray(rgb, 'RGB')
    assert np.array_equal(np.asarray(image.convert('L')), R.luma(rgb))
    m = Image.fromarray(mark, 'RGBA')
    pasted = image.copy()
    pasted.paste(m, (0, 0), m)
    assert np.array_equal(np.asarray(pasted), R.paste(rgb, mark))
    assert np.array_equal(np.asarray(VD.obscure_image(image)), R.obscure(rgb))


# ----------------------------------------------------------------------------- vision/datasets.py on the host
def test_module_surface():
    assert VD.N_MODALITIES == 6 == len(VM.MODALITIES) and VD.VALID_PARTITIONS == {'train': 0, 'val': 1, 'test': 2}
    from mvae_amd.celeba import datasets as CD
    assert VD.load_eval_partition is CD.load_eval_partition
    for text in ('grayscale_image', 'in place', 'JPEG round trip'):
        assert text.lower() in VD.__doc__.lower(), text


def test_obscure_image_and_add_watermark_equal_pillow_and_leave_their_argument(tmp_path):
    rng = np.random.RandomState(4)
    rgb = rng.randint(0, 256, (9, 7, 3)).astype(np.uint8)
    mark = rng.randint(0, 256, (4, 5, 4)).astype(np.uint8)
    mark_path = str(tmp_path / 'mark.png')
    Image.fromarray(mark, 'RGBA').save(mark_path)
    image = Image.fromarray(rgb, 'RGB')
    out = VD.obscure_image(image)
    want = rgb.copy()
    want[:, 7 // 2 + 1:, :] = 0                                   # columns 4, 5, 6
    assert isinstance(out, Image.Image) and out.mode == 'RGB' and np.array_equal(np.asarray(out), want)
    assert want[:, 3].any() and np.array_equal(np.asarray(image), rgb)
    out = VD.add_watermark(image, watermark_path=mark_path)
    ref = Image.fromarray(rgb, 'RGB')
    m = Image.open(mark_path).resize((7, 9), Image.BICUBIC)
    ref.paste(m, (0, 0), m)
    assert isinstance(out, Image.Image) and out.size == (7, 9) and np.array_equal(np.asarray(out), np.asarray(ref))
    assert not np.array_equal(np.asarray(out), rgb) and np.array_equal(np.asarray(image), rgb)
    assert np.array_equal(R.paste(rgb, VD.watermark_rgba(mark_path, 7, 9)), np.asarray(ref))
    Image.fromarray(rgb, 'RGB').save(str(tmp_path / 'opaque.png'))
    with pytest.raises(ValueError, match='alpha'):
        VD.watermark_rgba(str(tmp_path / 'opaque.png'), 7, 9)


@pytest.mark.parametrize('gray', ['folder', 'rgb', 'auto'])
def test_celeb_vision_items_equal_the_restatement(tmp_path, gray):
    root = str(tmp_path)
    names, mark_path = make_vision_tree(root, counts=(5, 1, 0), seed=1)
    ds = VD.CelebVision('train', root, watermark_path=mark_path, gray=gray, size=8)
    assert len(ds) == 5 and ds.image_paths == names[0] and len(VD.CelebVision('val', root, mark_path)) == 1
    for i in range(5):
        item = ds[i]
        want = restated_item(root, names[0][i], mark_path, gray != 'rgb', 8)
        assert len(item) == 6
        for m, (got, ref) in enumerate(zip(item, want)):
            assert got.dtype == torch.float32 and tuple(got.shape) == (VM.N_CHANNELS[VM.MODALITIES[m]], 8, 8)
            assert np.array_equal(got.numpy(), ref), (i, VM.MODALITIES[m])
    # the repaired defect: the obscured modality carries no watermark, the watermark modality is not half black
    item = ds[0]
    assert not torch.equal(item[4], item[5]) and not torch.equal(item[0], item[5])
    with pytest.raises(AssertionError):
        VD.CelebVision('nope', root)
    with pytest.raises(ValueError, match='gray'):
        VD.CelebVision('train', root, gray='jpeg')


def test_gray_auto_without_the_folder_takes_the_luma(tmp_path):
    root = str(tmp_path)
    names, mark_path = make_vision_tree(root, counts=(2, 0, 0), seed=2)
    for name in names[0]:
        os.remove(os.path.join(root, VD.GRAY_DIR, name))
    os.rmdir(os.path.join(root, VD.GRAY_DIR))
    assert VD.missing_data(root) == []
    ds = VD.CelebVision('train', root, watermark_path=mark_path, size=8)
    assert not ds.gray_from_folder
    want = restated_item(root, names[0][1], mark_path, False, 8)
    assert np.array_equal(ds[1][1].numpy(), want[1])
    with pytest.raises(ValueError, match='img_align_celeba_grayscale'):
        VD.CelebVision('train', root, watermark_path=mark_path, gray='folder')


# ----------------------------------------------------------------------------- refusals before any launch
def test_compose_entry_is_exported_bound_and_refuses_bad_arguments_without_a_gpu():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, 'mvae_vision_compose') and len(_lib._SIGNATURES['mvae_vision_compose'][1]) == 28
    lib = _lib.lib()
    assert lib.mvae_abi_version() == 6
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(rgb=p, edge=p, mask=p, gray=p, mark=p, o0=p, o1=p, o2=p, o3=p, o4=p, o5=p, B=2, H=218, W=178, out_h=78,
                out_w=64, S=64, top=7, left=0, kx=p, bx=p, ksx=7, ky=p, by=p, ksy=7, y0=16, y1=201)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mvae_vision_compose(*([a[k] for k in order] + [None]))

    for name in ('rgb', 'edge', 'mask', 'mark', 'o0', 'o1', 'o2', 'o3', 'o4', 'o5', 'kx', 'bx', 'ky', 'by'):
        assert call(**{name: None}) == -1, name                       # a null required pointer (gray may be null)
    for name in ('B', 'H', 'W', 'S', 'ksx', 'ksy'):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(top=-1) == -1 and call(left=-1) == -1
    assert call(top=15) == -1 and call(left=1) == -1                  # the crop leaves the resized image
    assert call(out_h=63) == -1 and call(out_w=63) == -1
    assert call(y0=-1) == -1 and call(y1=219) == -1                   # rows outside the image
    assert call(y0=100, y1=100) == -1 and call(y0=101, y1=100) == -1  # no rows at all
    # LDS: 800 rows x 64 columns x 3 planes = 153,600 bytes of intermediate fill the 150 KiB cap alone, no room for a source row
    assert call(H=1000, out_h=1000, y0=0, y1=800) == -1 and call(H=1000, out_h=1000, y0=0, y1=1000) == -1
    assert call(W=30000, out_w=30000) == -1                           # one staged row of the watermark group: 210 KB


def test_vision_compose_checks_its_arguments_then_asks_for_a_gpu():
    op = PP.VisionCompose(8)
    rgb = torch.zeros(2, 23, 17, 3, dtype=torch.uint8)
    plane = torch.zeros(2, 23, 17, dtype=torch.uint8)
    mark = torch.zeros(23, 17, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU'):
        op(rgb, plane, plane, mark)
    with pytest.raises(RuntimeError, match='GPU'):
        op(rgb, plane, plane, mark, gray=plane)
    with pytest.raises(TypeError, match='rgb'):
        op(rgb.float(), plane, plane, mark)
    with pytest.raises(TypeError, match='gray'):
        op(rgb, plane, plane, mark, gray=plane.float())
    with pytest.raises(TypeError, match='mark'):
        op(rgb, plane, plane, mark.numpy())
    with pytest.raises(ValueError, match='rgb'):
        op(rgb[0], plane, plane, mark)                                # rank
    with pytest.raises(ValueError, match='rgb'):
        op(torch.zeros(2, 23, 17, 4, dtype=torch.uint8), plane, plane, mark)
    with pytest.raises(ValueError, match='edge'):
        op(rgb, plane[:1], plane, mark)                               # another batch size
    with pytest.raises(ValueError, match='mask'):
        op(rgb, plane, torch.zeros(2, 17, 23, dtype=torch.uint8), mark)
    with pytest.raises(ValueError, match='mark'):
        op(rgb, plane, plane, torch.zeros(23, 17, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match='gray'):
        op(rgb, plane, plane, mark, gray=plane[:, :22])


# ----------------------------------------------------------------------------- train.py
def test_train_cli_names_what_is_missing(tmp_path):
    empty = str(tmp_path / 'empty')
    os.makedirs(empty)
    with pytest.raises(SystemExit, match='out of scope') as e:
        VT.main(['--data-dir', empty])
    text = str(e.value)
    for rel in VD.REQUIRED:
        assert rel in text, rel
    assert '--synthetic' in text and 'setup.py' in text and empty in text
    root = str(tmp_path / 'data')
    os.makedirs(root)
    _, mark_path = make_vision_tree(root, counts=(2, 1, 0), hw=(64, 64))
    with pytest.raises(SystemExit, match='--watermark-file'):
        VT.main(['--data-dir', root, '--watermark-file', str(tmp_path / 'none.png')])
    with pytest.raises(SystemExit, match='pass --cuda'):              # the data is there: the next stop is the GPU
        VT.main(['--data-dir', root, '--watermark-file', mark_path])
    import shutil
    shutil.rmtree(os.path.join(root, VD.MASK_DIR))
    with pytest.raises(SystemExit, match='out of scope') as e:
        VT.main(['--data-dir', root, '--watermark-file', mark_path])
    assert VD.MASK_DIR in str(e.value) and VD.EDGE_DIR not in str(e.value)
    assert VT.parser().parse_args([]).watermark_file == './watermark.png'
