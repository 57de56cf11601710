"""GPU: the Canny kernels (csrc/vision_setup.hip) behind ``preprocess.Canny`` -- the hysteresis stage byte for byte against
the restatement on class planes built to be hard for a sweep scheme, the float stage against the restatement in fp64 under
the tolerance rule of tests/test_vision_setup_cpu.py (tol = 8 x max|mag_fp32 - mag_fp64| of the restatement, classes
compared at every pixel whose margin is at least tol), and ``vision/setup.py edge`` / ``CelebVisionLoader(edge='canny')``
end to end on a tree of lossless files."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib, preprocess as PP
from mvae_amd.vision import datasets as VD, setup as VS
import vision_data_ref as VR
import vision_setup_ref as R
from test_vision_data_cpu import make_vision_tree

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cached scenes are read-only


# ----------------------------------------------------------------------------- hysteresis, exact
def spiral(h, w):
    """The pixels of a one-pixel-wide spiral from the corner inwards, arms one empty pixel apart, in walking order."""
    p = np.zeros((h, w), bool)
    y, x, dy, dx = 0, 0, 0, 1
    p[0, 0] = True
    path = [(0, 0)]
    while True:
        for _ in range(2):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not p[ny, nx] and not (0 <= ay < h and 0 <= ax < w and p[ay, ax]):
                break
            dy, dx = dx, -dy                   # turn right
        else:
            return path
        y, x = ny, nx
        p[y, x] = True
        path.append((y, x))


def plane_of(path, shape, strong=()):
    cls = np.zeros(shape, np.uint8)
    for y, x in path:
        cls[y, x] = 1
    for k in strong:
        cls[path[k]] = 2
    return cls


def serpentine(h, w, vertical=False):
    """A boustrophedon chain over the whole plane: every other row full, joined at alternating ends (or the transpose)."""
    if vertical:
        return [(y, x) for x, y in serpentine(w, h)]
    path = []
    for y in range(0, h, 2):
        xs = range(w) if (y // 2) % 2 == 0 else range(w - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < h:
            path.append((y + 1, path[-1][1]))
    return path


def hysteresis_planes():
    """name -> [3, H, W] class planes, a different plane per image of a batch."""
    h, w = 33, 29
    rng = np.random.RandomState(5)
    sp = spiral(h, w)
    assert len(sp) > h * w // 3
    diag = np.zeros((h, w), np.uint8)
    for k in range(min(h, w)):                 # two crossing diagonals: every link is a diagonal one; seeded at one end
        diag[k, k] = 1
        diag[h - 1 - k, k] = 1
    zig = np.zeros((h, w), np.uint8)
    for k in range(w):                         # a zigzag: every step is a diagonal one
        zig[10 + (k % 2), k] = 1
    zig[10, 0] = 2
    diag[0, 0] = 2
    two = np.zeros((h, w), np.uint8)           # two components one empty pixel apart: one seeded, one not
    two[5, 2:20] = 1
    two[7, 2:20] = 1
    two[5, 2] = 2
    two[20:30, 10] = 1
    two[20:30, 12] = 1
    two[29, 12] = 2
    border = np.zeros((h, w), np.uint8)        # a weak chain along all four image borders, one strong pixel
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 1
    border[h - 1, w // 2] = 2
    border[10:20, 10] = 1                      # and an unseeded piece inside
    rand = []
    for density in (0.1, 0.4, 0.8):
        c = (rng.rand(h, w) < density).astype(np.uint8)
        c[(rng.rand(h, w) < 0.02) & (c > 0)] = 2
        rand.append(c)
    rand[1][rand[1] == 2] = 255                # anything above weak counts as strong
    big = (218, 178)
    long_chain = np.zeros((70, 70), np.uint8)  # crosses every multiple of 32 in both directions
    long_chain[3, :] = 1
    long_chain[:, 66] = 1
    for k in range(70):
        long_chain[k, max(0, 60 - k)] = 1
    long_chain[69, 66] = 2
    return {
        'spirals': np.stack([plane_of(sp, (h, w), strong=[len(sp) - 1]), plane_of(sp, (h, w)),
                             plane_of(sp, (h, w), strong=[0])]),
        'diagonals': np.stack([diag, zig, two]),
        'border_and_random': np.stack([border, rand[0], rand[1]]),
        'dense': np.stack([rand[2], rand[2][::-1, ::-1].copy(), np.zeros((h, w), np.uint8)]),
        'celeba_sized': np.stack([plane_of(serpentine(*big), big, strong=[0]),
                                  plane_of(serpentine(*big, vertical=True), big, strong=[-1]),
                                  plane_of(spiral(*big), big, strong=[-1])]),
        'tiles': np.stack([long_chain, long_chain.T.copy(), np.where(long_chain == 2, 1, long_chain).astype(np.uint8)]),
    }


@pytest.mark.parametrize('name', ['spirals', 'diagonals', 'border_and_random', 'dense', 'celeba_sized', 'tiles'])
def test_hysteresis_equals_the_restatement(name):
    planes = hysteresis_planes()[name]
    want = np.stack([R.hysteresis(p) for p in planes])
    got = PP.canny_hysteresis(dev(planes)).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == planes.shape
    for b in range(3):
        assert np.array_equal(got[b], want[b]), '%s image %d: %d of %d pixels differ' % (
            name, b, (got[b] != want[b]).sum(), want[b].size)
    if name == 'spirals':
        assert want[0].astype(bool).sum() == (planes[0] > 0).sum() and not want[1].any() and want[2].any()
    if name == 'celeba_sized':
        assert all(want[b].astype(bool).sum() == (planes[b] > 0).sum() > 218 * 178 // 3 for b in range(3))
    if name == 'diagonals':
        assert want[2][5, 10] and not want[2][7, 10] and want[2][25, 12] and not want[2][25, 10]


# ----------------------------------------------------------------------------- the float stage
@pytest.mark.parametrize('h,w,seed', R.SCENES)
def test_float_stage_against_the_restatement_in_fp64(h, w, seed):
    c = R.scene_case(h, w, seed)
    edges, cls, mag = [t.cpu().numpy()[0] for t in PP.Canny().stages(dev(c['img'][None]))]
    assert mag.dtype == np.float32 and cls.dtype == np.uint8 and edges.dtype == np.uint8
    err = np.abs(mag.astype(np.float64) - c['s64']['mag'])
    differ = cls != c['s64']['cls']
    print('%dx%d seed %d: max|mag - mag64| %.3g (tol %.3g), class pixels that differ %d (of them excused %d), '
          'bits equal to the fp32 restatement at %.2f %% of the pixels'
          % (h, w, seed, err.max(), c['tol'], differ.sum(), (differ & c['excused']).sum(),
             100.0 * (mag == c['s32']['mag']).mean()))
    assert err.max() <= c['tol']
    assert not (differ & ~c['excused']).any()
    assert set(np.unique(cls)) <= {0, 1, 2} and set(np.unique(edges)) <= {0, 255}
    assert np.array_equal(edges, R.hysteresis(cls))
    if not differ.any():
        assert np.array_equal(edges, c['edges'])


def rgb_scene(h, w, seeds):
    return np.stack([R.scene(h, w, s) for s in seeds], axis=-1)


def test_rgb_input_equals_the_result_on_pillows_luma():
    from PIL import Image
    rgb = np.stack([rgb_scene(37, 29, (31, 32, 33)), rgb_scene(37, 29, (34, 35, 36))])
    gray = np.stack([np.asarray(Image.fromarray(im, 'RGB').convert('L')) for im in rgb])
    assert np.array_equal(gray, VR.luma(rgb)) and gray.std() > 5
    op = PP.Canny()
    a, b = op.stages(dev(rgb)), op.stages(dev(gray))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].any() and torch.equal(op(dev(rgb)), a[0])


def test_batches_alignment_determinism_and_nullable_outputs():
    imgs = np.stack([R.scene(37, 29, s) for s in (41, 42, 43)])
    op = PP.Canny()
    whole = op.stages(dev(imgs))
    assert whole[0].shape == (3, 37, 29) and whole[0].any()
    for b in range(3):                                                 # a batch of 3 equals three single calls
        single = op.stages(dev(imgs[b:b + 1]))
        for x, y in zip(whole, single):
            assert torch.equal(x[b], y[0]), b
    again = op.stages(dev(imgs))                                       # two runs are bit-identical
    for x, y in zip(whole, again):
        assert torch.equal(x, y)
    assert torch.equal(op(dev(imgs)), whole[0])                        # cls and mag null: the workspace path
    # base pointers 1 and 3 bytes off a 256-byte boundary, for src, edges and cls alike (37 * 29 is odd: images 1 and 2
    # of the aligned batch start misaligned as well)
    lib, n = _lib.lib(), imgs.size
    for off in (1, 3):
        src = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        src[off:off + n] = dev(imgs).reshape(-1)
        edges = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        cls = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        assert src.data_ptr() % 4 == 0 and edges.data_ptr() % 4 == 0
        for cls_ptr, ws_ptr in ((cls.data_ptr() + off, None), (None, cls.data_ptr() + off)):
            edges.zero_()
            rc = lib.mvae_canny(ctypes.c_void_p(src.data_ptr() + off), 1, 3, 37, 29, 2.0, 0.1, 0.2,
                                ctypes.c_void_p(edges.data_ptr() + off), ctypes.c_void_p(cls_ptr) if cls_ptr else None,
                                None, ctypes.c_void_p(ws_ptr) if ws_ptr else None, n,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            torch.cuda.synchronize()
            assert torch.equal(edges[off:off + n].view(3, 37, 29), whole[0]), off
            assert torch.equal(cls[off:off + n].view(3, 37, 29), whole[1]), off
            assert not edges[:off].any() and not edges[off + n:].any()      # nothing written outside


def test_other_sigmas_and_thresholds_follow_the_restatement():
    """Radius 4 (sigma 1) and the largest one, 16 (sigma 4), with thresholds that are not the defaults."""
    img = R.scene(37, 29, 10)
    for sigma, low, high in ((1.0, 0.05, 0.3), (4.0, 0.02, 0.05)):
        s64, s32 = R.stages(img, np.float64, sigma, low, high), R.stages(img, np.float32, sigma, low, high)
        tol = R.TOL_FACTOR * float(np.abs(s32['mag'].astype(np.float64) - s64['mag']).max())
        excused = s64['margin'] < tol
        assert excused.mean() <= R.MAX_EXCUSED_SHARE and (s64['cls'] > 0).any()
        edges, cls, mag = [t.cpu().numpy()[0] for t in PP.Canny(sigma, low, high).stages(dev(img[None]))]
        assert np.abs(mag.astype(np.float64) - s64['mag']).max() <= tol
        assert np.array_equal(cls[~excused], s64['cls'][~excused])
        assert np.array_equal(edges, R.hysteresis(cls))


# ----------------------------------------------------------------------------- end to end
def test_setup_edge_cli_and_the_canny_loader_on_a_tree_of_lossless_files(tmp_path):
    from PIL import Image
    root = str(tmp_path / 'data')
    os.makedirs(root)
    names, mark_path = make_vision_tree(root, counts=(5, 0, 0), hw=(23, 17), seed=16)
    # a second image size in the folder: the CLI groups equal sizes into launches
    odd = np.random.RandomState(3).randint(0, 256, (9, 31, 3)).astype(np.uint8)
    Image.fromarray(odd).save(os.path.join(root, VD.IMAGE_DIR, 'other.png'))
    shutil.rmtree(os.path.join(root, VD.EDGE_DIR))
    VS.main(['edge', os.path.join(root, VD.IMAGE_DIR), os.path.join(root, VD.EDGE_DIR), '--batch-size', '4',
             '--decode-threads', '2'])
    assert sorted(os.listdir(os.path.join(root, VD.EDGE_DIR))) == sorted(names[0] + ['other.png'])
    op = PP.Canny()
    some = False
    for name in names[0] + ['other.png']:
        luma = np.asarray(Image.open(os.path.join(root, VD.IMAGE_DIR, name)).convert('L'))
        got = Image.open(os.path.join(root, VD.EDGE_DIR, name))
        want = op(dev(luma[None]))[0].cpu().numpy()
        assert got.mode == 'L' and np.array_equal(np.asarray(got), want), name
        assert np.array_equal(want, R.hysteresis(op.stages(dev(luma[None]))[1][0].cpu().numpy()))
        some = some or want.any()
    assert some
    os.remove(os.path.join(root, VD.IMAGE_DIR, 'other.png'))
    device = torch.device(DEV)
    folder = VD.CelebVisionLoader('train', root, 2, False, device, watermark_path=mark_path, size=8)
    canny = VD.CelebVisionLoader('train', root, 2, False, device, watermark_path=mark_path, size=8, edge='canny')
    shutil.rmtree(os.path.join(root, VD.EDGE_DIR) + '_moved', ignore_errors=True)
    batches = list(folder)
    os.rename(os.path.join(root, VD.EDGE_DIR), os.path.join(root, VD.EDGE_DIR) + '_moved')      # 'canny' opens no edge file
    ds = VD.CelebVision('train', root, watermark_path=mark_path, size=8, edge='canny')
    seen = 0
    for a, b in zip(batches, canny):
        assert len(a) == len(b) == 6
        for m in range(6):
            assert torch.equal(a[m], b[m]), m
        item = ds[seen]                                                 # the per-item surface, same mode
        for m in range(6):
            assert torch.equal(b[m][0].cpu(), item[m]), m
        seen += a[0].shape[0]
    assert seen == 5 and len(batches) == 3
