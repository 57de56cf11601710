"""Drop-in for the reference's ``vision/datasets.py``: ``N_MODALITIES``, ``VALID_PARTITIONS``, ``load_eval_partition``,
``obscure_image``, ``add_watermark`` and the ``CelebVision`` dataset surface (vision/datasets.py:15-129) -- plus
``CelebVisionLoader``, which feeds the train step: per batch the four files of every item are decoded on the host
(Pillow), each source goes to HBM once and ONE HIP launch (``preprocess.VisionCompose``, csrc/vision_data.hip) derives
the two further modalities and runs ``Resize(64) + CenterCrop(64) + ToTensor`` on all six, byte-exact with the per-item
Pillow arithmetic of ``CelebVision``.

Only Pillow is needed here.  The folder ``img_align_celeba_edge`` (Canny) is written once by ``vision/setup.py edge`` of
this package (HIP kernels) or of the reference (scikit-image); ``img_align_celeba_mask`` (dlib landmarks) only by the
reference's ``vision/setup.py``, whose mask builder stays out of scope.  This module reads
``Eval/list_eval_partition.txt``, ``img_align_celeba``, ``img_align_celeba_edge``, ``img_align_celeba_mask`` and,
optionally, ``img_align_celeba_grayscale``.

Two defects of the reference text are repaired:

    :79,90   ``grayscale_image`` is undefined -- the transformed gray tensor is what is returned.
    :74-76   the watermark is pasted onto ``obscured_image`` IN PLACE (``add_watermark`` mutates its argument), so the
             obscured modality would carry the mark too and the watermark modality would be half black.  Here the mark
             goes onto the full colour image and ``obscured`` stays unmarked -- the reading ``vision/sample.py`` takes
             for ``--condition-type watermark``; ``add_watermark`` works on a copy.

``gray``: ``'folder'`` reads ``img_align_celeba_grayscale`` as the reference does, ``'rgb'`` takes Pillow's
``convert('L')`` of the colour image (on the device: the kernel's integer luma), ``'auto'`` is ``'folder'`` when the
folder exists.  The grayscale folder holds JPEGs, so its pixels went through one more JPEG round trip than the luma of
the colour file: ``'rgb'`` does not reproduce that round trip.

``edge``: ``'folder'`` (the default, the reference's data) reads ``img_align_celeba_edge``; ``'canny'`` does not open that
folder: the edge modality is ``preprocess.Canny`` (sigma 2, thresholds 0.1 / 0.2: what ``setup.py edge`` writes) of the
colour image's luma, computed on the device -- by ``CelebVisionLoader`` on the uploaded colour batch, one more op in
front of the compose launch, and by ``CelebVision.__getitem__`` on its one image (so the per-item surface needs a GPU
in this mode and raises the usual "GPU" ``RuntimeError`` without one).  The same caveat as for ``gray='rgb'``: an edge
folder of ``.jpg`` names went through a JPEG round trip after Canny, ``'canny'`` does not reproduce that round trip.  On
a folder of lossless files the two modes give equal batches."""
import os

import numpy as np
import torch

from ..celeba.datasets import VALID_PARTITIONS, load_eval_partition  # noqa: F401
from ..preprocess import center_crop_origin, resized_size

N_MODALITIES = 6
PARTITION_FILE = 'Eval/list_eval_partition.txt'
IMAGE_DIR, GRAY_DIR, EDGE_DIR, MASK_DIR = ('img_align_celeba', 'img_align_celeba_grayscale', 'img_align_celeba_edge',
                                           'img_align_celeba_mask')
REQUIRED = (PARTITION_FILE, IMAGE_DIR, EDGE_DIR, MASK_DIR)
GRAY_MODES = ('auto', 'folder', 'rgb')
EDGE_MODES = ('folder', 'canny')


def check_edge_mode(edge):
    if edge not in EDGE_MODES:
        raise ValueError("edge must be one of %s, got %r" % (', '.join(EDGE_MODES), edge))
    return edge


def missing_data(data_dir, edge='folder'):
    """The entries of ``REQUIRED`` that are not under ``data_dir``; with ``edge='canny'`` the edge folder is not needed."""
    check_edge_mode(edge)
    wanted = [rel for rel in REQUIRED if not (edge == 'canny' and rel == EDGE_DIR)]
    return [rel for rel in wanted
            if not (os.path.isfile if rel == PARTITION_FILE else os.path.isdir)(os.path.join(data_dir, rel))]


def gray_from_folder(gray, data_dir):
    """Resolve ``gray`` ('auto' | 'folder' | 'rgb') to whether the grayscale folder is read."""
    if gray not in GRAY_MODES:
        raise ValueError("gray must be one of %s, got %r" % (', '.join(GRAY_MODES), gray))
    have = os.path.isdir(os.path.join(data_dir, GRAY_DIR))
    if gray == 'folder' and not have:
        raise ValueError('gray=%r but %s is missing' % (gray, os.path.join(data_dir, GRAY_DIR)))
    return gray == 'folder' or (gray == 'auto' and have)


def obscure_image(image):
    """Block image vertically in half with black pixels (vision/datasets.py:97-111): PIL colour image in, a new PIL
    image out with the columns ``> width // 2`` black."""
    from PIL import Image
    image_npy = np.array(image, copy=True)
    center_h = image_npy.shape[1] // 2
    image_npy[:, center_h + 1:, :] = 0
    return Image.fromarray(image_npy)


def open_watermark(watermark_path, width, height):
    """The watermark file resized to the image as the reference does it (:125-127, BICUBIC in the file's own mode)."""
    from PIL import Image
    return Image.open(watermark_path).resize((width, height), Image.BICUBIC)


def add_watermark(image, watermark_path='./watermark.png'):
    """Overlay the watermark file on a colour image (vision/datasets.py:114-129).  PIL in, PIL out; the argument is
    left as it was (the reference pastes in place)."""
    watermark = open_watermark(watermark_path, image.size[0], image.size[1])
    image = image.copy()
    image.paste(watermark, (0, 0), watermark)
    return image


def watermark_rgba(watermark_path, width, height):
    """uint8 [H, W, 4]: the resized watermark as the RGBA array ``paste(mark, (0, 0), mark)`` blends with."""
    watermark = open_watermark(watermark_path, width, height)
    if watermark.mode != 'RGBA':
        raise ValueError('the watermark %s has mode %s: an RGBA image is needed, its alpha is the mask of paste()'
                         % (watermark_path, watermark.mode))
    return np.array(watermark, dtype=np.uint8)


def image_transform(image, size=64):
    """``Compose([Resize(size), CenterCrop(size), ToTensor()])`` of one PIL image on the host (:43-45)."""
    from PIL import Image
    w, h = image.size
    nh, nw = resized_size(h, w, size)
    if nh < size or nw < size:
        raise ValueError('image %dx%d is smaller than the crop after Resize(%d)' % (h, w, size))
    top, left = center_crop_origin(nh, nw, size)
    arr = np.asarray(image.resize((nw, nh), Image.BILINEAR), dtype=np.uint8)[top:top + size, left:left + size]
    arr = arr[:, :, None] if arr.ndim == 2 else arr
    return torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0))


class CelebVision(object):
    """The reference's Dataset surface (vision/datasets.py:19-94): ``dataset[i]`` is the 6-tuple (image, gray, edge,
    mask, obscured, watermark) of float tensors [C, size, size], computed on the host with Pillow.  The per-item yardstick:
    the train step does not go through it -- see ``CelebVisionLoader``."""

    def __init__(self, partition='train', data_dir='./data', watermark_path='./watermark.png', gray='auto', size=64,
                 edge='folder'):
        if partition not in VALID_PARTITIONS:
            raise AssertionError(partition)
        self.partition, self.data_dir, self.watermark_path = partition, data_dir, watermark_path
        self.edge = check_edge_mode(edge)
        self._canny = None
        self.gray_from_folder = gray_from_folder(gray, data_dir)
        self.image_paths = load_eval_partition(partition, data_dir=data_dir)
        self.size = int(len(self.image_paths))
        self.out_size = int(size)

    def load_sources(self, index):
        """The decoded files of one item as PIL images: (rgb, edge, mask, gray or None); edge is None with
        ``edge='canny'``."""
        from PIL import Image
        name = self.image_paths[index]
        rgb = Image.open(os.path.join(self.data_dir, IMAGE_DIR, name)).convert('RGB')
        edge = None
        if self.edge == 'folder':
            edge = Image.open(os.path.join(self.data_dir, EDGE_DIR, name)).convert('L')
        mask = Image.open(os.path.join(self.data_dir, MASK_DIR, name)).convert('L')
        gray = None
        if self.gray_from_folder:
            gray = Image.open(os.path.join(self.data_dir, GRAY_DIR, name)).convert('L')
        return rgb, edge, mask, gray

    def canny_edges(self, image):
        """``edge='canny'``: the edge map of one PIL colour image as a PIL 'L' image, by the device op on its luma."""
        from PIL import Image
        from ..preprocess import Canny
        if self._canny is None:
            self._canny = Canny()
        u8 = torch.from_numpy(np.array(image.convert('L'), dtype=np.uint8))[None]
        if torch.cuda.is_available():
            u8 = u8.cuda()
        return Image.fromarray(self._canny(u8)[0].cpu().numpy())

    def __getitem__(self, index):
        image, edge_image, mask_image, gray_image = self.load_sources(index)
        if gray_image is None:
            gray_image = image.convert('L')
        if edge_image is None:
            edge_image = self.canny_edges(image)
        obscured_image = obscure_image(image)
        watermark_image = add_watermark(image, watermark_path=self.watermark_path)
        image, gray_image, edge_image, mask_image, obscured_image, watermark_image = [
            image_transform(x, self.out_size)
            for x in (image, gray_image, edge_image, mask_image, obscured_image, watermark_image)]
        # masks are white with black lines; like edges, make the background black and the lines white (:84-87)
        mask_image = 1 - mask_image
        return image, gray_image, edge_image, mask_image, obscured_image, watermark_image

    def __len__(self):
        return self.size


class CelebVisionLoader(object):
    """The 6-tuple batches ``train_step`` / ``fused_step`` / ``test()`` take: the DataLoader over ``CelebVision`` of
    vision/train.py:138-144 with everything after the file decode on the GPU.  Per batch: Pillow decodes the three or
    four files of every item (host threads), ONE pinned uint8 copy to HBM per source, ONE ``VisionCompose`` launch; with
    ``edge='canny'`` the edge file is not opened and ``Canny`` runs on the uploaded colour batch before it.  The
    watermark is opened and resized once per image size and kept on the device.  All images of a batch must share a
    size (aligned CelebA: 218 x 178)."""

    def __init__(self, partition, data_dir, batch_size, shuffle, device, seed=0, watermark_path='./watermark.png',
                 gray='auto', decode_threads=8, size=64, edge='folder'):
        from ..preprocess import Canny, VisionCompose
        self.data = CelebVision(partition, data_dir, watermark_path=watermark_path, gray=gray, size=size, edge=edge)
        self._canny = Canny() if edge == 'canny' else None
        if not os.path.isfile(watermark_path):
            raise ValueError('the watermark file %s is missing' % watermark_path)
        self.batch_size, self.shuffle, self.device = int(batch_size), bool(shuffle), device
        self.dataset = range(len(self.data))
        self._gen = torch.Generator().manual_seed(seed)
        self._compose = VisionCompose(size)
        self._threads = max(1, int(decode_threads))
        self._marks = {}

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _decode(self, index):
        return [None if im is None else np.asarray(im, dtype=np.uint8) for im in self.data.load_sources(index)]

    def _mark(self, h, w):
        if (h, w) not in self._marks:
            rgba = watermark_rgba(self.data.watermark_path, w, h)
            self._marks[(h, w)] = torch.from_numpy(rgba).to(self.device)
        return self._marks[(h, w)]

    def _upload(self, frames):
        u8 = torch.from_numpy(np.stack(frames))
        if torch.cuda.is_available():
            u8 = u8.pin_memory()
        return u8.to(self.device, non_blocking=True)

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        n_total = len(self.data)
        order = (torch.randperm(n_total, generator=self._gen) if self.shuffle else torch.arange(n_total)).tolist()
        with ThreadPoolExecutor(self._threads) as pool:
            for i in range(0, len(order), self.batch_size):
                items = list(pool.map(self._decode, order[i:i + self.batch_size]))
                shapes = {f.shape[:2] for item in items for f in item if f is not None}
                if len(shapes) != 1:
                    raise ValueError('images of one batch differ in size: %s' % sorted(shapes))
                h, w = shapes.pop()
                rgb, edge, mask, gray = [None if item0 is None else self._upload([item[s] for item in items])
                                         for s, item0 in enumerate(items[0])]
                if self._canny is not None:
                    edge = self._canny(rgb)
                yield self._compose(rgb, edge, mask, self._mark(h, w), gray=gray)
