"""CPU restatement (numpy + scipy.ndimage) of the Canny edge detector of ``mvae_canny`` (csrc/vision_setup.hip), the
checker for the kernel, for ``preprocess.Canny`` and for ``vision/setup.py edge``.

TEST INFRASTRUCTURE: imported only by tests/ and tools/vision_setup_bench.py.

Written from the description of the algorithm (include/mvae_hip.h, K26) -- scikit-image's documented ``feature.canny`` on
a float image in [0, 1] with its default thresholds and no mask.  scikit-image itself is not a dependency of this
repository: the description is the yardstick, not a release of that library (newer ones differ in details such as ``>``
against ``>=`` at the thresholds).

    g      = u8 / 255
    blur   = taps w[k] = exp(-k^2 / 2 sigma^2), |k| <= r = int(4 sigma + 0.5), sum 1; correlate1d(mode='constant') down
             the columns, then along the rows; divided by by[y] * bx[x], the same two blurs of ones
    sobel  = scipy.ndimage.sobel along axis 0 (isobel) and axis 1 (jsobel), mode 'reflect' (the border sample duplicated)
    mag    = sqrt(isobel^2 + jsobel^2)
    maxima = the four interpolation cases of the header, applied in order on the candidates (not on the image border,
             mag > 0); classes 2 / 1 / 0 from ``high`` / ``low``
    edges  = scipy.ndimage.label with a 3 x 3 structure: the components that hold a strong pixel

``stages(img, dtype)`` runs all of it in ``dtype`` (scipy's filters accumulate in double and round to the array's type
once per pass) and also returns, per pixel, the MARGIN of its class: how far the magnitude comparisons that decide the
class are from flipping it.  Every comparison is of ``mag`` against another number -- the two interpolated neighbour
values v+ and v- (local maximum: v+ <= mag and v- <= mag), ``low`` and ``high``:

    class 2   min(|mag - v+|, |mag - v-|, mag - high)                     any one of them flipping changes the class
    class 1   min(|mag - v+|, |mag - v-|, mag - low, high - mag)
    class 0   max over the comparisons that FAIL (v+ > mag, v- > mag, mag < low) of their distance: the class changes
              only when all of them flip
    not a candidate (image border, mag == 0)    infinity

A pixel whose margin is below the tolerance of a test is "excused" from the class comparison there.
"""
import numpy as np
from scipy import ndimage as ndi

SIGMA, LOW, HIGH = 2.0, 0.1, 0.2

# the scenes of the GPU test: (H, W, seed).  5 x 40 and 40 x 5: the blur radius (8) exceeds the image; 37 x 29 and 17 x 9
# are no multiple of the float stage's 32 x 32 tile; 64 x 64 is exactly four tiles; 218 x 178 is the CelebA shape.
SCENES = ((24, 20, 12), (37, 29, 10), (5, 40, 10), (40, 5, 4), (17, 9, 11), (3, 3, 6), (64, 64, 7), (218, 178, 8),
          (218, 178, 9))
TOL_FACTOR = 8.0            # tol = 8 x max|mag_fp32 - mag_fp64| of THIS restatement: summation order, FMA contraction
MAX_EXCUSED_SHARE = 0.01


def scene(h, w, seed):
    """uint8 [h, w]: a mid-gray ground, a few disks and rectangles of random gray level, Gaussian noise of 0.02."""
    rng = np.random.RandomState(seed)
    img = np.full((h, w), 0.5)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(3 + rng.randint(3)):
        level = 0.5 + rng.choice([-1.0, 1.0]) * rng.uniform(0.04, 0.3)
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        if rng.rand() < 0.5:
            rad = rng.uniform(0.15, 0.45) * max(min(h, w), 6)
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = level
        else:
            hh, hw = rng.uniform(0.1, 0.4) * max(h, 6), rng.uniform(0.1, 0.4) * max(w, 6)
            img[(abs(yy - cy) <= hh) & (abs(xx - cx) <= hw)] = level
    img = img + rng.normal(0.0, 0.02, (h, w))
    return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)


def radius(sigma):
    return int(4.0 * float(np.float32(sigma)) + 0.5)


def taps(sigma, dtype):
    s = float(np.float32(sigma))        # the C ABI takes sigma as a float
    k = np.arange(-radius(sigma), radius(sigma) + 1, dtype=np.float64)
    w = np.exp(-0.5 * k * k / (s * s))
    return (w / w.sum()).astype(dtype)


def smooth(img, dtype, sigma=SIGMA):
    g = img.astype(dtype) / dtype(255)
    w = taps(sigma, dtype)
    blur = ndi.correlate1d(ndi.correlate1d(g, w, axis=0, mode='constant'), w, axis=1, mode='constant')
    by = ndi.correlate1d(np.ones(img.shape[0], dtype), w, mode='constant')
    bx = ndi.correlate1d(np.ones(img.shape[1], dtype), w, mode='constant')
    return blur / (by[:, None] * bx[None, :])


def _at(a, off):
    """a[y + dy, x + dx] at [y, x]; only read at interior pixels, where the wrap of roll does not reach."""
    return np.roll(a, (-off[0], -off[1]), axis=(0, 1))


def stages(img, dtype, sigma=SIGMA, low=LOW, high=HIGH):
    """uint8 [H, W] -> dict(mag, isobel, jsobel [H, W] dtype; cls [H, W] uint8; margin [H, W] float64)."""
    dtype = np.dtype(dtype).type
    sm = smooth(img, dtype, sigma)
    isobel, jsobel = ndi.sobel(sm, axis=0), ndi.sobel(sm, axis=1)
    mag = np.sqrt(isobel * isobel + jsobel * jsobel)
    assert mag.dtype == dtype
    low, high = dtype(np.float32(low)), dtype(np.float32(high))
    ai, aj = np.abs(isobel), np.abs(jsobel)
    cand = np.zeros(img.shape, bool)
    cand[1:-1, 1:-1] = True
    cand &= mag > 0
    same = ((isobel >= 0) & (jsobel >= 0)) | ((isobel <= 0) & (jsobel <= 0))
    opposite = ((isobel <= 0) & (jsobel >= 0)) | ((isobel >= 0) & (jsobel <= 0))
    one = dtype(1)
    ok_p, ok_m = np.zeros(img.shape, bool), np.zeros(img.shape, bool)
    d_p, d_m = np.full(img.shape, np.inf), np.full(img.shape, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        w_i, w_j = aj / ai, ai / aj
    for cond, c1, c2, w in ((same & (ai >= aj), (1, 0), (1, 1), w_i), (same & (ai <= aj), (0, 1), (1, 1), w_j),
                            (opposite & (ai <= aj), (0, 1), (-1, 1), w_j), (opposite & (ai >= aj), (-1, 0), (-1, 1), w_i)):
        sel = cand & cond
        with np.errstate(invalid='ignore'):
            vp = _at(mag, c2) * w + _at(mag, c1) * (one - w)
            vm = _at(mag, (-c2[0], -c2[1])) * w + _at(mag, (-c1[0], -c1[1])) * (one - w)
        ok_p[sel], ok_m[sel] = (vp <= mag)[sel], (vm <= mag)[sel]
        d_p[sel] = np.abs(mag.astype(np.float64) - vp)[sel]
        d_m[sel] = np.abs(mag.astype(np.float64) - vm)[sel]
    lm = cand & ok_p & ok_m
    cls = np.zeros(img.shape, np.uint8)
    cls[lm & (mag >= low)] = 1
    cls[lm & (mag >= high)] = 2
    m64 = mag.astype(np.float64)
    keep = np.minimum(d_p, d_m)
    margin = np.full(img.shape, np.inf)
    s2, s1, s0 = cls == 2, cls == 1, cand & (cls == 0)
    margin[s2] = np.minimum(keep, m64 - float(high))[s2]
    margin[s1] = np.minimum(keep, np.minimum(m64 - float(low), float(high) - m64))[s1]
    fail = np.maximum(np.where(ok_p, 0.0, d_p), np.where(ok_m, 0.0, d_m))
    fail = np.maximum(fail, np.where(mag < low, float(low) - m64, 0.0))
    margin[s0] = fail[s0]
    return dict(mag=mag, isobel=isobel, jsobel=jsobel, cls=cls, margin=margin)


def hysteresis(cls):
    """uint8 class plane [H, W] (0 none, 1 weak, >= 2 strong) -> uint8 0 / 255: the 8-connected components of non-zero
    classes that hold a strong pixel."""
    lab, _ = ndi.label(cls > 0, structure=np.ones((3, 3), bool))
    strong = np.unique(lab[cls >= 2])
    return (np.isin(lab, strong[strong > 0]) & (lab > 0)).astype(np.uint8) * 255


def canny(img, sigma=SIGMA, low=LOW, high=HIGH, dtype=np.float64):
    return hysteresis(stages(img, dtype, sigma, low, high)['cls'])


_CACHE = {}


def scene_case(h, w, seed):
    """Everything the tests need of one scene, computed once per process and never modified: the image, the fp64 and fp32
    stages, tol = TOL_FACTOR x max|mag32 - mag64| and the excused mask (margin of the fp64 run < tol)."""
    key = (h, w, seed)
    if key not in _CACHE:
        img = scene(h, w, seed)
        s64, s32 = stages(img, np.float64), stages(img, np.float32)
        tol = TOL_FACTOR * float(np.abs(s32['mag'].astype(np.float64) - s64['mag']).max())
        case = dict(img=img, s64=s64, s32=s32, tol=tol, excused=s64['margin'] < tol, edges=hysteresis(s64['cls']))
        for v in (img, case['excused'], case['edges']) + tuple(s64.values()) + tuple(s32.values()):
            v.setflags(write=False)
        _CACHE[key] = case
    return _CACHE[key]
