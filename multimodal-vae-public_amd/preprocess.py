"""On-device input pipeline: the per-image transforms of the reference's loaders as batch launches.

    ToTensor                      (mnist/train.py:160,164)        -> ``to_tensor(u8)``
    Compose([Resize(64), CenterCrop(64), ToTensor()])
                                  (celeba/train.py:146-148)       -> ``ResizeCenterCropToTensor(64)(u8_nhwc)``
    the six modalities of one item  (vision/datasets.py:54-91)    -> ``VisionCompose(64)(rgb, edge, mask, mark, gray)``
    feature.canny(image / 255., sigma=2)  (vision/setup.py:70-73) -> ``Canny(2.0)(u8)``

Input: raw ``uint8`` images already in HBM (``[B, H, W]`` / ``[B, H, W, 3]``, the decoded JPEG / IDX
bytes); output: the ``float32`` NCHW batch the MVAE step consumes.  Resize is byte-exact with Pillow's
BILINEAR (what torchvision calls); the coefficient tables depend only on the image size and are built
once per size on the host by the library (``mvae_resample_coeffs``) and cached on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .kernels import _need_gpu, _ptr, _stream, check


def to_tensor(u8):
    """uint8 [B, H, W] or [B, C, H, W] (cuda) -> float32 / 255; a missing channel axis is added."""
    _need_gpu(u8)
    if u8.dtype != torch.uint8:
        raise TypeError('to_tensor expects uint8, got %s' % u8.dtype)
    u8 = u8.contiguous()
    out = torch.empty(u8.shape, dtype=torch.float32, device=u8.device)
    check(_lib.lib().mvae_u8_to_f32(_ptr(u8), _ptr(out), u8.numel(), _stream()), 'mvae_u8_to_f32')
    return out.unsqueeze(1) if out.dim() == 3 else out


def resized_size(h, w, size):
    """torchvision Resize(int): shorter side -> size, longer -> int(size * long / short)."""
    return (int(size * h / w), size) if w <= h else (size, int(size * w / h))


def center_crop_origin(h, w, size):
    return int(round((h - size) / 2.0)), int(round((w - size) / 2.0))


def _axis_tables(in_size, out_size):
    lib = _lib.lib()
    ks = lib.mvae_resample_ksize(in_size, out_size)
    check(min(ks, 0), 'mvae_resample_ksize')
    kk = np.zeros((out_size, ks), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    rc = lib.mvae_resample_coeffs(in_size, out_size, kk.ctypes.data_as(ctypes.c_void_p),
                                  bounds.ctypes.data_as(ctypes.c_void_p))
    check(min(rc, 0), 'mvae_resample_coeffs')
    return kk, bounds, ks


class ResizeCenterCropToTensor(object):
    """``transforms.Compose([Resize(size), CenterCrop(size), ToTensor()])`` for a uint8 NHWC batch."""

    def __init__(self, size=64):
        self.size = int(size)
        self._tables = {}

    def _plan(self, h, w, device):
        key = (h, w, device)
        if key not in self._tables:
            S = self.size
            nh, nw = resized_size(h, w, S)
            if nh < S or nw < S:
                raise ValueError('image %dx%d is smaller than the crop after Resize(%d)' % (h, w, S))
            top, left = center_crop_origin(nh, nw, S)
            kx, bx, ksx = _axis_tables(w, nw)
            ky, by, ksy = _axis_tables(h, nh)
            rows = by[top:top + S]
            y0, y1 = int(rows[:, 0].min()), int((rows[:, 0] + rows[:, 1]).max())
            dev = [torch.from_numpy(t).to(device) for t in (kx, bx, ky, by)]
            self._tables[key] = (nh, nw, top, left, ksx, ksy, y0, y1, dev)
        return self._tables[key]

    def __call__(self, u8_nhwc):
        _need_gpu(u8_nhwc)
        if u8_nhwc.dtype != torch.uint8 or u8_nhwc.dim() != 4 or u8_nhwc.shape[3] != 3:
            raise TypeError('expected a uint8 [B, H, W, 3] batch')
        x = u8_nhwc.contiguous()
        B, H, W, _ = x.shape
        nh, nw, top, left, ksx, ksy, y0, y1, (kx, bx, ky, by) = self._plan(H, W, x.device)
        S = self.size
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=x.device)
        check(_lib.lib().mvae_resize_crop_u8_to_f32(_ptr(x), _ptr(out), B, H, W, nh, nw, S, top, left, _ptr(kx),
                                                    _ptr(bx), ksx, _ptr(ky), _ptr(by), ksy, y0, y1, _stream()),
              'mvae_resize_crop_u8_to_f32')
        return out


class Canny(object):
    """Canny edges of a uint8 batch on the device (csrc/vision_setup.hip): what the reference's ``vision/setup.py edge``
    computes per file with ``skimage.feature.canny(image / 255., sigma=2)``.  ``__call__(u8)`` takes [B, H, W] (gray) or
    [B, H, W, 3] (RGB: Pillow's ``convert('L')`` first) and returns the edge map [B, H, W] uint8, 0 or 255.

    What is computed is scikit-image's DOCUMENTED algorithm (Gaussian blur normalised by the blur of ones, Sobel, bilinear
    non-maximum suppression, thresholds ``low`` / ``high`` on the gradient magnitude, 8-connected hysteresis; spelled out
    under K26 in include/mvae_hip.h and restated in tests/vision_setup_ref.py), not a particular release of that library:
    newer releases differ in details such as ``>`` against ``>=`` at the thresholds.

    The blur taps are built by the library per call (33 numbers at most, passed by value) and the normalisation is
    rebuilt per tile on the device, so there is no table to cache: per (H, W) the op keeps the library's verdict on the
    shape, per device one workspace (the class plane between the two launches) that grows to the largest batch seen."""

    def __init__(self, sigma=2.0, low=0.1, high=0.2):
        self.sigma, self.low, self.high = float(sigma), float(low), float(high)
        if not (0.0 <= self.low <= self.high < float('inf')):
            raise ValueError('Canny: need 0 <= low <= high, got low=%r high=%r' % (low, high))
        self._shapes = {}
        self._ws = {}

    def _check(self, u8):
        if not torch.is_tensor(u8) or u8.dtype != torch.uint8:
            raise TypeError('Canny expects a uint8 tensor, got %s' % getattr(u8, 'dtype', type(u8)))
        if u8.dim() not in (3, 4) or (u8.dim() == 4 and u8.shape[3] != 3) or u8.shape[0] <= 0:
            raise ValueError('Canny expects a non-empty [B, H, W] or [B, H, W, 3] batch, got %s' % (tuple(u8.shape),))
        B, H, W = (int(s) for s in u8.shape[:3])
        if (H, W) not in self._shapes:
            self._shapes[(H, W)] = bool(_lib.lib().mvae_canny_supported(H, W, self.sigma))
        if not self._shapes[(H, W)]:
            raise ValueError('Canny: images of %d x %d at sigma %g are not supported (needs H, W >= 3, a blur radius '
                             'int(4 sigma + 0.5) <= 16 and a class plane that fits one block\'s LDS)' % (H, W, self.sigma))
        _need_gpu(u8)
        return B, H, W

    def _run(self, u8, want_stages):
        B, H, W = self._check(u8)
        x = u8.contiguous()
        edges = torch.empty(B, H, W, dtype=torch.uint8, device=x.device)
        cls = mag = ws = None
        need = 0
        if want_stages:
            cls = torch.empty(B, H, W, dtype=torch.uint8, device=x.device)
            mag = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
        else:
            need = _lib.lib().mvae_canny_ws_bytes(B, H, W)
            ws = self._ws.get(x.device)
            if ws is None or ws.numel() < need:
                ws = self._ws[x.device] = torch.empty(need, dtype=torch.uint8, device=x.device)
        check(_lib.lib().mvae_canny(_ptr(x), 3 if x.dim() == 4 else 1, B, H, W, self.sigma, self.low, self.high,
                                    _ptr(edges), _ptr(cls), _ptr(mag), _ptr(ws), need, _stream()), 'mvae_canny')
        return edges, cls, mag

    def __call__(self, u8):
        return self._run(u8, False)[0]

    def stages(self, u8):
        """(edges, cls, mag): the edge map, the class plane (0 none, 1 weak, 2 strong) and the gradient magnitude."""
        return self._run(u8, True)


def canny_hysteresis(cls):
    """Step 6 of ``Canny`` alone: uint8 class planes [B, H, W] (0 none, 1 weak, >= 2 strong) -> edge maps, 0 or 255."""
    if not torch.is_tensor(cls) or cls.dtype != torch.uint8 or cls.dim() != 3:
        raise TypeError('canny_hysteresis expects a uint8 [B, H, W] tensor')
    _need_gpu(cls)
    x = cls.contiguous()
    out = torch.empty_like(x)
    check(_lib.lib().mvae_canny_hysteresis(_ptr(x), _ptr(out), x.shape[0], x.shape[1], x.shape[2], _stream()),
          'mvae_canny_hysteresis')
    return out


class VisionCompose(object):
    """The six modalities of the vision step (``vision.model.MODALITIES`` order: image, gray, edge, mask, obscured,
    watermark) from one batch of raw uint8 sources, in ONE launch: the right half blacked out, the watermark pasted, and
    ``Compose([Resize(size), CenterCrop(size), ToTensor()])`` on all six, ``1 - x`` for the mask (vision/datasets.py:
    43-45, 64-87, 97-129).  ``rgb`` [B, H, W, 3], ``edge`` / ``mask`` / ``gray`` [B, H, W], ``mark`` [H, W, 4]: the RGBA
    watermark already resized to the images' size.  Without ``gray`` the kernel takes the luma of ``rgb`` (Pillow's
    ``convert('L')``)."""

    def __init__(self, size=64):
        self.size = int(size)
        self._resize = ResizeCenterCropToTensor(self.size)      # its per-(H, W, device) plan cache, unchanged

    def __call__(self, rgb, edge, mask, mark, gray=None):
        named = [('rgb', rgb, 4), ('edge', edge, 3), ('mask', mask, 3), ('mark', mark, 3)]
        if gray is not None:
            named.append(('gray', gray, 3))
        for name, t, rank in named:
            if not torch.is_tensor(t) or t.dtype != torch.uint8:
                raise TypeError('%s: expected a uint8 tensor, got %s' % (name, getattr(t, 'dtype', type(t))))
            if t.dim() != rank:
                raise ValueError('%s: expected %d dimensions, got shape %s' % (name, rank, tuple(t.shape)))
        if rgb.shape[3] != 3:
            raise ValueError('rgb: expected [B, H, W, 3], got %s' % (tuple(rgb.shape),))
        B, H, W, _ = rgb.shape
        if B <= 0:
            raise ValueError('rgb: an empty batch')
        for name, t, _ in named[1:]:
            want = (H, W, 4) if name == 'mark' else (B, H, W)
            if tuple(t.shape) != want:
                raise ValueError('%s: expected %s to go with rgb %s, got %s' % (name, want, tuple(rgb.shape),
                                                                                tuple(t.shape)))
        tensors = [t for _, t, _ in named]
        _need_gpu(*tensors)
        if any(t.device != rgb.device for t in tensors):
            raise ValueError('the sources are on different devices')
        rgb, edge, mask, mark = [t.contiguous() for t in (rgb, edge, mask, mark)]
        gray = gray.contiguous() if gray is not None else None
        nh, nw, top, left, ksx, ksy, y0, y1, (kx, bx, ky, by) = self._resize._plan(H, W, rgb.device)
        S = self.size
        out = [torch.empty(B, c, S, S, dtype=torch.float32, device=rgb.device) for c in (3, 1, 1, 1, 3, 3)]
        check(_lib.lib().mvae_vision_compose(_ptr(rgb), _ptr(edge), _ptr(mask), _ptr(gray), _ptr(mark),
                                             *([_ptr(o) for o in out] +
                                               [B, H, W, nh, nw, S, top, left, _ptr(kx), _ptr(bx), ksx, _ptr(ky),
                                                _ptr(by), ksy, y0, y1, _stream()])),
              'mvae_vision_compose')
        return tuple(out)
