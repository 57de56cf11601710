"""CPU restatement (numpy, integer arithmetic) of the vision experiment's six-modality input pipeline, the checker for
``mvae_vision_compose`` (csrc/vision_data.hip) and ``vision/datasets.py``.

TEST INFRASTRUCTURE: imported only by tests/ and tools/vision_data_bench.py.

Written from the description of the step: from one colour image [H, W, 3], an edge, a mask and (optionally) a gray plane
[H, W] and the RGBA watermark [H, W, 4], all uint8,

    gray       the gray plane, or Pillow's convert('L') of the colour image: (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
    obscured   the colour image with the columns x > W // 2 black
    watermark  Pillow's paste(mark, (0, 0), mark): per channel t = dst * (255 - a) + src * a + 128, ((t >> 8) + t) >> 8

then Pillow's two-pass 8-bit BILINEAR resample to Resize(S)'s size and CenterCrop(S) on every plane
(``oracle.preprocess``), ``u8 / 255`` in float32, and ``1 - x`` for the mask.  Pinned against Pillow 12.2 itself by
tests/golden/vision_data.npz (tests/golden/make_vision_data_golden.py) and, where Pillow imports, live in
tests/test_vision_data_cpu.py.
"""
import numpy as np

from oracle import preprocess as OP

MODALITIES = ('image', 'gray', 'edge', 'mask', 'obscured', 'watermark')

# the golden cases: name -> (H, W, S, B, seed); inputs come from ``case_inputs`` (only outputs are stored)
CASES = {
    'celeba': (218, 178, 64, 2, 101),       # the real shape: the LDS budget and the plane split
    'tall': (23, 17, 8, 3, 102),            # odd H * W: images 1 and 2 start misaligned; crop_top = 1
    'wide': (17, 23, 8, 2, 103),            # crop_left > 0
    'unit': (64, 64, 64, 1, 104),           # unit scale: the 3-tap filter
    'one_row': (65, 64, 64, 1, 105),        # the one-row crop
}
GRAY_TWICE = 'tall'                          # this case runs with its gray source and with gray = None


def luma(rgb):
    """Pillow convert('L') of uint8 [..., 3]."""
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def obscure(rgb):
    out = np.array(rgb, copy=True)
    out[..., out.shape[-2] // 2 + 1:, :] = 0
    return out


def paste(rgb, mark):
    """Pillow paste(mark, (0, 0), mark) of an RGBA mark [H, W, 4] on uint8 [..., H, W, 3]."""
    a = mark[..., 3:4].astype(np.int64)
    t = rgb.astype(np.int64) * (255 - a) + mark[..., :3].astype(np.int64) * a + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def resize_crop_u8(u8_hwc, size):
    """Resize(size) + CenterCrop(size) of uint8 [H, W, C] -> uint8 [size, size, C]."""
    h, w, _ = u8_hwc.shape
    nh, nw = OP.resized_size(h, w, size)
    top, left = OP.center_crop_origin(nh, nw, size)
    return OP.resize_bilinear_u8(u8_hwc, nw, nh)[top:top + size, left:left + size]


def derive(rgb, edge, mask, mark, gray=None):
    """The six uint8 images of one item before the resample, in MODALITIES order ([H, W, 3] or [H, W, 1])."""
    g = luma(rgb) if gray is None else gray
    return [rgb, g[:, :, None], edge[:, :, None], mask[:, :, None], obscure(rgb), paste(rgb, mark)]


def compose_u8(rgb, edge, mask, mark, gray=None, size=64, resize_crop=resize_crop_u8):
    """Batched: rgb [B, H, W, 3], edge / mask / gray [B, H, W], mark [H, W, 4] -> six uint8 arrays [B, C, size, size]
    BEFORE the division (the mask NOT yet inverted)."""
    out = [[] for _ in MODALITIES]
    for b in range(rgb.shape[0]):
        planes = derive(rgb[b], edge[b], mask[b], mark, None if gray is None else gray[b])
        for m, p in enumerate(planes):
            out[m].append(resize_crop(np.ascontiguousarray(p), size).transpose(2, 0, 1))
    return [np.stack(v) for v in out]


def to_float(u8_six):
    """ToTensor of the six uint8 arrays and ``1 - x`` for the mask, float32."""
    out = [v.astype(np.float32) / np.float32(255.0) for v in u8_six]
    out[3] = np.float32(1.0) - out[3]
    return out


def compose(rgb, edge, mask, mark, gray=None, size=64):
    return to_float(compose_u8(rgb, edge, mask, mark, gray, size))


def case_inputs(name):
    """The seeded inputs of a golden case: dict(rgb, edge, mask, gray, mark, size).  Every case puts hard 0 / 255 columns
    on both sides of the obscure boundary W // 2 + 1; 'tall' also carries a mark whose alpha holds 0, 255 and mid values
    over colour values 0 and 255 on both sides."""
    H, W, S, B, seed = CASES[name]
    rng = np.random.RandomState(seed)
    rgb = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    edge = rng.randint(0, 256, (B, H, W)).astype(np.uint8)
    mask = rng.randint(0, 256, (B, H, W)).astype(np.uint8)
    gray = rng.randint(0, 256, (B, H, W)).astype(np.uint8)        # NOT the luma of rgb: the source must be what is read
    mark = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
    cut = W // 2 + 1
    rgb[:, : H // 2, cut - 1] = 255; rgb[:, : H // 2, cut] = 255       # bright on both sides of the cut
    rgb[:, H // 2:, cut - 1] = 0; rgb[:, H // 2:, cut] = 255
    edge[0, :, : W // 3] = 255; mask[0, : H // 3] = 0                  # saturated regions stay saturated
    if name == 'tall':
        # rows 0..5: alpha 0 / 255 / mid, each over dst in {0, 255} x src in {0, 255}
        for r, alpha in enumerate((0, 255, 128, 1, 254, 77)):
            mark[r, :, 3] = alpha
            mark[r, 0::2, :3] = 0; mark[r, 1::2, :3] = 255
            rgb[:, r, 0::4] = 0; rgb[:, r, 1::4] = 0; rgb[:, r, 2::4] = 255; rgb[:, r, 3::4] = 255
    return dict(rgb=rgb, edge=edge, mask=mask, gray=gray, mark=mark, size=S)


def golden_key(name, modality, with_gray):
    return '%s/%s/%s' % (name, 'gray' if with_gray else 'luma', modality)


def golden_runs():
    """(case, with_gray) of every stored run: every case with its gray source, GRAY_TWICE also without."""
    return [(name, True) for name in CASES] + [(GRAY_TWICE, False)]
