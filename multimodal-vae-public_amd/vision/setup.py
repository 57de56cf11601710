"""Drop-in for the reference's ``vision/setup.py``: the folders ``vision/datasets.py`` reads besides the CelebA download
are computed once, before training -- same positional CLI, same function names.

    python multimodal-vae-public_amd/vision/setup.py grayscale ./data/img_align_celeba ./data/img_align_celeba_grayscale
    python multimodal-vae-public_amd/vision/setup.py edge      ./data/img_align_celeba ./data/img_align_celeba_edge
    python multimodal-vae-public_amd/vision/setup.py mask      ./data/img_align_celeba ./data/img_align_celeba_mask

``grayscale``  host only, as the reference (:37-52): ``convert('RGB').convert('L')``, saved under the same name.
``edge``       the reference (:55-75) calls ``skimage.feature.canny(image / 255., sigma)`` per file and saves
               ``Image.fromarray(edges * 255)`` under the same name (so ``.jpg`` names become JPEGs).  Here host threads
               decode (``convert('L')``) and encode, images of equal size are grouped into launches of ``--batch-size``
               and ``preprocess.Canny`` (csrc/vision_setup.hip) computes the edge maps on the GPU.  What is computed is
               scikit-image's DOCUMENTED algorithm -- Gaussian blur normalised by the blur of ones, Sobel, bilinear
               non-maximum suppression, thresholds 0.1 / 0.2, 8-connected hysteresis (include/mvae_hip.h, K26) -- not a
               particular release of that library, which is not a dependency here: newer releases differ in details such
               as ``>`` against ``>=`` at the thresholds.  ``--sigma`` defaults to 2, what the reference's ``__main__``
               passes; ``build_edge_dataset`` keeps the reference's default of 3.  ``out_dir`` is created when missing.
``mask``       NOT BUILT: the reference draws dlib's 68 facial landmarks (HOG face detector + the landmark model file
               ``shape_predictor_68_face_landmarks.dat``) with OpenCV.  Neither library nor the model file is a dependency
               of this repository; the script says so and exits.  The mask folder is the one thing a user must bring from
               the reference's ``setup.py``: with ``--edge canny`` the loaders derive the edge modality on the fly.
"""
import os
import sys

if __package__ in (None, ''):      # executed as a script, like the reference (`python setup.py edge in out`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.vision'

import numpy as np  # noqa: E402

MASK_MESSAGE = ("the mask builder is not built here: it needs dlib's face detector, OpenCV and the landmark model file "
                "shape_predictor_68_face_landmarks.dat, none of which this repository depends on.  Run the reference's "
                "vision/setup.py mask for the mask folder")


def build_grayscale_dataset(in_dir, out_dir):
    """Generate a dataset of grayscale images (vision/setup.py:37-52).  Host only."""
    from PIL import Image
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
    image_paths = sorted(os.listdir(in_dir))
    n_images = len(image_paths)
    for i, image_path in enumerate(image_paths):
        print('Building grayscale dataset: [%d/%d] images.' % (i + 1, n_images))
        image = Image.open(os.path.join(in_dir, image_path)).convert('RGB').convert('L')
        image.save(os.path.join(out_dir, image_path))


def build_edge_dataset(in_dir, out_dir, sigma=3, batch_size=64, decode_threads=8):
    """Generate a dataset of (canny) edge-detected images (vision/setup.py:55-75) on the GPU.

    @param sigma: float (default: 3, the reference's; its ``__main__`` and this one pass 2)
    @param batch_size: images decoded per round; those of equal size share one launch
    @param decode_threads: host threads that decode and encode
    """
    import torch
    from PIL import Image
    from concurrent.futures import ThreadPoolExecutor
    from ..preprocess import Canny
    if not torch.cuda.is_available():
        raise SystemExit('setup.py edge computes the Canny edges with HIP kernels and needs a ROCm GPU (the box the '
                         'other scripts want --cuda on); grayscale runs on the host')
    device = torch.device('cuda', 0)
    op = Canny(sigma=sigma)
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
    image_paths = sorted(os.listdir(in_dir))
    n_images = len(image_paths)

    def decode(name):
        return np.asarray(Image.open(os.path.join(in_dir, name)).convert('L'), dtype=np.uint8)

    def encode(job):
        name, edges = job
        Image.fromarray(edges).save(os.path.join(out_dir, name))

    batch_size = max(1, int(batch_size))
    with ThreadPoolExecutor(max(1, int(decode_threads))) as pool:
        for i in range(0, n_images, batch_size):
            names = image_paths[i:i + batch_size]
            frames = list(pool.map(decode, names))
            by_shape = {}
            for k, f in enumerate(frames):
                by_shape.setdefault(f.shape, []).append(k)
            out = [None] * len(names)
            for shape, ks in by_shape.items():
                u8 = torch.from_numpy(np.stack([frames[k] for k in ks])).pin_memory().to(device, non_blocking=True)
                try:
                    edges = op(u8).cpu().numpy()
                except ValueError as e:
                    raise SystemExit('%s (first such file: %s)' % (e, os.path.join(in_dir, names[ks[0]])))
                for j, k in enumerate(ks):
                    out[k] = edges[j]
            list(pool.map(encode, zip(names, out)))
            print('Building edge-detected dataset: [%d/%d] images.' % (i + len(names), n_images))


def build_mask_dataset(in_dir, out_dir, model_path):
    """Generate a dataset of segmentation masks from images (vision/setup.py:78-116): not built, see the module text."""
    raise SystemExit(MASK_MESSAGE)


def parser():
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument('type', type=str, help='grayscale|edge|mask')
    p.add_argument('in_dir', type=str, help='where images are located')
    p.add_argument('out_dir', type=str, help='where images are to be saved')
    p.add_argument('--batch-size', type=int, default=64, help='edge: images per launch [default: 64]')
    p.add_argument('--decode-threads', type=int, default=8, help='edge: host threads that decode and encode [default: 8]')
    p.add_argument('--sigma', type=float, default=2.0, help='edge: smoothness for edge detection [default: 2]')
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.type == 'grayscale':
        build_grayscale_dataset(args.in_dir, args.out_dir)
    elif args.type == 'edge':
        build_edge_dataset(args.in_dir, args.out_dir, sigma=args.sigma, batch_size=args.batch_size,
                           decode_threads=args.decode_threads)
    elif args.type == 'mask':
        build_mask_dataset(args.in_dir, args.out_dir, './data/shape_predictor_68_face_landmarks.dat')
    else:
        raise SystemExit('type must be grayscale, edge or mask, got %r' % args.type)


if __name__ == '__main__':
    main()
