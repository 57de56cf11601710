"""Drop-in for the reference's ``multimnist/datasets.py``: the ``MultiMNIST`` dataset surface (:29-101), the builder
that makes the data set out of MNIST (:107-290) and its command line (:293-342) -- plus ``MultiMNISTLoader``, which
feeds the train loop from HBM.

    python multimodal-vae-public_amd/multimnist/datasets.py --data-dir ./data

The data set does not exist until it is built: 0-4 MNIST digits, each resized by a random factor (Pillow's 8-bit
BILINEAR, which is what ``scipy.misc.imresize`` called), pasted at a random place on a 50 x 50 canvas; a canvas whose
pixel sums exceed 255 ("crude check for overlapping digits", :141-144) is thrown away and drawn again.  The reference
does this one canvas at a time in numpy.  Here the compose step is one HIP launch per chunk of canvases
(``kernels.multimnist_compose``, csrc/multimnist_data.hip) over a digit bank resident in HBM, and the rejection loop
runs in ROUNDS:

  1. the host draws a plan for a chunk of at most ``CHUNK`` = 8192 canvases from ``np.random.RandomState(seed)``
     (default seed 681307, the reference's) with the reference's formulas -- ``num_digits = randint(min, max + 1)``,
     ``i = randint(n_bank)``, ``w = int(28 * (1 / scale))`` with ``scale = 0.1 * randn() + 1.3``, ``randint(0, 50 - w)``
     twice; without resize ``w = 28``; without translate both offsets are ``(50 - w) // 2``; in fixed mode ``w = 21``
     and the offsets are (4, 4), (4, 23), (23, 4), (23, 23); ``no_repeat``, ``reverse`` and ``scramble`` act on the
     labels, on the host;
  2. the device composes the chunk and flags the canvases with a sum above 255;
  3. the host redraws only the flagged canvases -- each keeps its digit count, as the reference's recursion does;
  4. until none is flagged.

This samples the reference's DISTRIBUTION but not its random stream: the reference's retry consumes a data-dependent
number of draws from the same stream before the next canvas is begun, so a batched builder cannot reproduce that
stream (and the reference's builder cannot run on a current stack to compare: ``scipy.misc.imresize`` is gone).
A chunk that needs more than ``MAX_ROUNDS`` = 1000 rounds raises ``RuntimeError``.  The kernel takes widths 7..50;
at the defaults a width outside that range does not occur (``w < 7`` needs a scale ten standard deviations out); such
a draw, and ``w = 50`` with translation (``randint(0, 0)`` is an error in numpy), is redrawn on the host.
``max_digits > 4`` is refused: the text modality holds ``max_length`` = 4 characters.
"""
import os
import sys

if __package__ in (None, ''):      # executed as a script, like the reference (`python datasets.py`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import mvae_amd  # noqa: F401
    __package__ = 'multimodal-vae-public_amd.multimnist'

import numpy as np  # noqa: E402
import torch  # noqa: E402

from .. import kernels as K  # noqa: E402
from ..train_common import _find_idx, read_idx, shard_len, shard_order  # noqa: E402
from .utils import charlist_tensor, max_length  # noqa: E402

CANVAS = K.MM_CANVAS
CHUNK = 8192
MAX_ROUNDS = 1000
DEFAULT_SEED = 681307                                   # multimnist/datasets.py:187
FIXED_W = int(28 * (1. / 1.3))                          # sample_one_fixed's scale=1.3 -> 21
FIXED_PADS = [(4, 4), (4, 23), (23, 4), (23, 23)]       # multimnist/datasets.py:224


class MultiMNIST(object):
    """Images with 0 to 4 digits of non-overlapping MNIST numbers: the reference's Dataset surface
    (multimnist/datasets.py:29-101).  ``dataset[i] -> (PIL 'L' image, list of digit labels)`` with the optional
    transforms applied.  The files hold ``(ByteTensor [N, 50, 50], list of per-image label lists)``; labels stored
    as 0-d tensors (what the reference writes) are accepted and come back as ints."""
    processed_folder = 'multimnist'
    training_file = 'training.pt'
    test_file = 'test.pt'

    def __init__(self, root, train=True, transform=None, target_transform=None, download=False):
        self.root = os.path.expanduser(root)
        self.transform = transform
        self.target_transform = target_transform
        self.train = train
        if download:
            self.download()
        if not self._check_exists():
            raise RuntimeError('Dataset not found. You can use download=True to build it from the MNIST IDX files')
        data, labels = torch.load(os.path.join(self.root, self.processed_folder,
                                               self.training_file if self.train else self.test_file))
        data = torch.as_tensor(data)
        labels = [[int(d) for d in row] for row in labels]
        if data.dtype != torch.uint8 or data.dim() != 3 or len(labels) != data.shape[0]:
            raise ValueError('unexpected MultiMNIST file: %s %s, %d label lists' % (data.dtype, tuple(data.shape), len(labels)))
        if self.train:
            self.train_data, self.train_labels = data, labels
        else:
            self.test_data, self.test_labels = data, labels

    def _split(self):
        return (self.train_data, self.train_labels) if self.train else (self.test_data, self.test_labels)

    def __getitem__(self, index):
        from PIL import Image
        data, labels = self._split()
        img, target = Image.fromarray(data[index].numpy()), labels[index]      # uint8 [50, 50] -> mode 'L'
        if self.transform is not None:
            img = self.transform(img)
        if self.target_transform is not None:
            target = self.target_transform(target)
        return img, target

    def __len__(self):
        return len(self._split()[0])

    def _check_exists(self):
        folder = os.path.join(self.root, self.processed_folder)
        return os.path.exists(os.path.join(folder, self.training_file)) and os.path.exists(os.path.join(folder, self.test_file))

    def download(self):
        if self._check_exists():
            return
        make_dataset(self.root, self.processed_folder, self.training_file, self.test_file)


# ----------------------------------------------------------------------------- plans
def _check_digit_range(min_digits, max_digits):
    if max_digits > max_length:
        raise ValueError('max_digits = %d: the text modality holds at most %d characters' % (max_digits, max_length))
    if min_digits < 0 or min_digits > max_digits:
        raise ValueError('need 0 <= min_digits <= max_digits, got %d..%d' % (min_digits, max_digits))


def draw_canvas(rng, num_digits, mnist, resize=True, translate=True):
    """One canvas of the classic data set (sample_multi / sample_one, multimnist/datasets.py:107-146): ``num_digits``
    records (bank index, w, top, left) and their labels."""
    n_bank = mnist['digits'].shape[0]
    records, labels = [], []
    for _ in range(num_digits):
        i = rng.randint(n_bank)
        w = K.MM_DIGIT
        if resize:
            while True:
                scale = 0.1 * rng.randn() + 1.3
                w = int(K.MM_DIGIT * (1. / scale)) if scale > 0 else -1
                if K.MM_WMIN <= w <= K.MM_WMAX and (w < CANVAS or not translate):
                    break
        padding = CANVAS - w
        if translate:
            top, left = rng.randint(0, padding), rng.randint(0, padding)
        else:
            top = left = padding // 2
        records.append((i, w, top, left))
        labels.append(int(mnist['labels'][i]))
    return records, labels


def draw_canvas_fixed(rng, num_digits, mnist, reverse=False, scramble=False, no_repeat=False):
    """One canvas of the fixed-position data set (sample_multi_fixed, multimnist/datasets.py:220-251)."""
    n_bank = mnist['digits'].shape[0]
    records, labels = [], []
    for d in range(num_digits):
        while True:
            i = rng.randint(n_bank)
            label = int(mnist['labels'][i])
            if not no_repeat or label not in labels:
                break
        records.append((i, FIXED_W, FIXED_PADS[d][0], FIXED_PADS[d][1]))
        labels.append(label)
    if reverse and rng.rand() > 0.5:
        labels = labels[::-1]
    if scramble:
        rng.shuffle(labels)
    return records, labels


def _plan_row(records):
    row = np.zeros(K.MM_PLAN_STRIDE, dtype=np.int32)
    row[0] = len(records)
    for d, rec in enumerate(records):
        row[1 + 4 * d:5 + 4 * d] = rec
    return row


def device_composer(digits, device=None):
    """``plan -> (canvas uint8 [m, 50, 50], flags int32 [m])`` (numpy) on the HIP kernel, over ``digits`` uploaded
    to HBM once."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    bank = torch.from_numpy(np.array(digits, dtype=np.uint8)).to(device)       # a copy: IDX arrays are read-only views

    def compose(plan):
        canvas, flags = K.multimnist_compose(bank, plan)
        return canvas.cpu().numpy(), flags.cpu().numpy()
    return compose


def build_split(n, mnist, num_digits, draw, composer, chunk=CHUNK, max_rounds=MAX_ROUNDS):
    """The round driver.  ``num_digits``: int array [n], the digit count of every canvas (never redrawn);
    ``draw(k)``: records and labels of a fresh canvas of k digits; ``composer(plan)``: (canvas, flags) of a plan.
    Returns (canvases uint8 [n, 50, 50], label lists, final plans int32 [n, 17], stats): ``stats['rounds']`` holds
    the rounds every chunk took and ``stats['redrawn']`` the canvases redrawn in each round, summed over chunks."""
    n_bank = mnist['digits'].shape[0]
    x = np.zeros((n, CANVAS, CANVAS), dtype=np.uint8)
    y = [None] * n
    plans = np.zeros((n, K.MM_PLAN_STRIDE), dtype=np.int32)
    stats = {'rounds': [], 'redrawn': []}
    for c0 in range(0, n, chunk):
        todo = np.arange(c0, min(n, c0 + chunk))
        rounds = 0
        while todo.size:
            if rounds == max_rounds:
                raise RuntimeError('%d canvases still overlap after %d rounds' % (todo.size, max_rounds))
            if rounds:
                if len(stats['redrawn']) < rounds:
                    stats['redrawn'].append(0)
                stats['redrawn'][rounds - 1] += int(todo.size)
            for m in todo:
                records, y[m] = draw(int(num_digits[m]))
                plans[m] = _plan_row(records)
            sub = K.multimnist_validate_plan(plans[todo], n_bank)
            canvas, flags = composer(sub)
            canvas, flags = np.asarray(canvas), np.asarray(flags).reshape(-1)
            if canvas.shape != (todo.size, CANVAS, CANVAS) or flags.shape != (todo.size,) or (flags < 0).any():
                raise RuntimeError('the composer returned %s canvases / %s flags for %d plans'
                                   % (canvas.shape, flags.shape, todo.size))
            keep = flags == 0
            x[todo[keep]] = canvas[keep]
            todo = todo[~keep]
            rounds += 1
        stats['rounds'].append(rounds)
    return x, y, plans, stats


def _rng(rng):
    return np.random.RandomState(DEFAULT_SEED) if rng is None else rng


def _finish(out, return_plans):
    x, y, plans, stats = out
    return (x, y, plans, stats) if return_plans else (x, y)


def mk_dataset(n, mnist, min_digits, max_digits, canvas_size, resize=True, translate=True, composer=None, rng=None,
               return_plans=False):
    """``n`` canvases of the classic data set (multimnist/datasets.py:149-159): (uint8 [n, 50, 50], label lists), and
    with ``return_plans`` also the final plans and the round statistics.  ``composer``: the compose step as a
    callable ``plan -> (canvas, flags)``; the HIP kernel by default."""
    if canvas_size != CANVAS:
        raise ValueError('the compose kernel is built for %d x %d canvases' % (CANVAS, CANVAS))
    _check_digit_range(min_digits, max_digits)
    rng = _rng(rng)
    num_digits = np.array([rng.randint(min_digits, max_digits + 1) for _ in range(n)], dtype=np.int64)
    composer = device_composer(mnist['digits']) if composer is None else composer
    return _finish(build_split(n, mnist, num_digits, lambda k: draw_canvas(rng, k, mnist, resize, translate), composer),
                   return_plans)


def mk_dataset_fixed(n, mnist, min_digits, max_digits, canvas_size, reverse=False, scramble=False, no_repeat=False,
                     composer=None, rng=None, return_plans=False):
    """``n`` canvases of the fixed-position data set (multimnist/datasets.py:254-264)."""
    if canvas_size != CANVAS:
        raise ValueError('the compose kernel is built for %d x %d canvases' % (CANVAS, CANVAS))
    _check_digit_range(min_digits, max_digits)
    if no_repeat and max_digits > len(set(int(v) for v in mnist['labels'])):
        raise ValueError('no_repeat with %d digits needs that many distinct labels' % max_digits)
    rng = _rng(rng)
    num_digits = np.array([rng.randint(min_digits, max_digits + 1) for _ in range(n)], dtype=np.int64)
    composer = device_composer(mnist['digits']) if composer is None else composer
    return _finish(build_split(n, mnist, num_digits,
                               lambda k: draw_canvas_fixed(rng, k, mnist, reverse, scramble, no_repeat), composer),
                   return_plans)


def load_mnist(data_dir='./data'):
    """MNIST's two splits as {'digits': uint8 [N, 28, 28], 'labels': int64 [N]} from the raw IDX files under
    ``data_dir`` (multimnist/datasets.py:162-179 reads them through torchvision, which downloads them; there is no
    network here, so they must already be there)."""
    paths = [_find_idx(data_dir, stem) for stem in ('train-images-idx3-ubyte', 'train-labels-idx1-ubyte',
                                                    't10k-images-idx3-ubyte', 't10k-labels-idx1-ubyte')]
    if any(p is None for p in paths):
        raise SystemExit('no MNIST IDX files under %s (no network to download them): the MultiMNIST dataset builder '
                         'makes its canvases out of them' % data_dir)
    splits = []
    for images, labels in (paths[:2], paths[2:]):
        digits, lab = read_idx(images), read_idx(labels)
        if digits.ndim != 3 or digits.shape[1:] != (28, 28) or lab.shape != (digits.shape[0],):
            raise ValueError('unexpected IDX shapes %s / %s' % (digits.shape, lab.shape))
        splits.append({'digits': digits, 'labels': lab.astype(np.int64)})
    return splits[0], splits[1]


def _make(root, folder, training_file, test_file, build, data_dir, n_train, n_test, seed, composer, return_plans):
    if not os.path.isdir(os.path.join(root, folder)):
        os.makedirs(os.path.join(root, folder))
    rng = np.random.RandomState(seed)
    report = {}
    for name, mnist, n, fname in zip(('train', 'test'), load_mnist(root if data_dir is None else data_dir),
                                     (n_train, n_test), (training_file, test_file)):
        x, y, plans, stats = build(n, mnist, rng, None if composer is None else composer(mnist['digits']))
        with open(os.path.join(root, folder, fname), 'wb') as f:
            torch.save((torch.from_numpy(x), y), f)
        report[name] = {'plans': plans, 'rounds': stats['rounds'], 'redrawn': stats['redrawn']}
    return report if return_plans else None


def make_dataset(root, folder, training_file, test_file, min_digits=0, max_digits=2, resize=True, translate=True,
                 data_dir=None, n_train=60000, n_test=10000, seed=DEFAULT_SEED, composer=None, return_plans=False):
    """Build and save both splits of the classic data set (multimnist/datasets.py:182-204).  ``data_dir``: where the
    MNIST IDX files are (``root`` by default, as in the reference); ``composer``: a factory ``digits -> (plan ->
    (canvas, flags))`` replacing the HIP kernel; ``return_plans=True`` returns, per split, the final plan of every
    canvas and the round statistics."""
    _check_digit_range(min_digits, max_digits)
    return _make(root, folder, training_file, test_file,
                 lambda n, mnist, rng, comp: mk_dataset(n, mnist, min_digits, max_digits, CANVAS, resize=resize,
                                                        translate=translate, composer=comp, rng=rng, return_plans=True),
                 data_dir, n_train, n_test, seed, composer, return_plans)


def make_dataset_fixed(root, folder, training_file, test_file, min_digits=0, max_digits=3, reverse=False,
                       scramble=False, no_repeat=False, data_dir=None, n_train=60000, n_test=10000, seed=DEFAULT_SEED,
                       composer=None, return_plans=False):
    """Build and save both splits of the fixed-position data set (multimnist/datasets.py:267-290)."""
    _check_digit_range(min_digits, max_digits)
    return _make(root, folder, training_file, test_file,
                 lambda n, mnist, rng, comp: mk_dataset_fixed(n, mnist, min_digits, max_digits, CANVAS, reverse=reverse,
                                                              scramble=scramble, no_repeat=no_repeat, composer=comp,
                                                              rng=rng, return_plans=True),
                 data_dir, n_train, n_test, seed, composer, return_plans)


# ----------------------------------------------------------------------------- loader
class MultiMNISTLoader(object):
    """(image float32 [B, 1, 50, 50], text int64 [B, 4]) batches for the MultiMNIST train loop: the DataLoader +
    ``ToTensor`` / ``charlist_tensor`` transforms of multimnist/train.py:163-176 with no host work per batch.  The
    whole split sits in HBM as uint8 (60000 canvases: 150 MB) with its labels as FILL-padded int64 [N, 4]; a batch is
    an index gather + ``preprocess.to_tensor`` on the device, like ``IdxLoader``.  The short last batch is kept; with
    ``shuffle`` every epoch draws a new permutation; ``rank`` / ``world`` shard one shared permutation."""

    def __init__(self, root, train, batch_size, shuffle, device, seed=0, rank=0, world=1):
        from .. import preprocess
        self._to_tensor = preprocess.to_tensor
        data = MultiMNIST(root, train=train)
        images, labels = data._split()
        if tuple(images.shape[1:]) != (CANVAS, CANVAS):
            raise ValueError('MultiMNIST canvases are 50 x 50, got %s' % (tuple(images.shape),))
        self.images = images.contiguous().to(device)
        self.labels = (torch.stack([charlist_tensor(row) for row in labels]) if labels
                       else torch.zeros(0, max_length, dtype=torch.int64)).to(device)
        self.batch_size, self.shuffle, self.device = int(batch_size), bool(shuffle), device
        self.rank, self.world = int(rank), int(world)
        self._n_total = int(images.shape[0])
        self.dataset = range(shard_len(self._n_total, self.world))       # samples per rank, equal on all ranks
        self._gen = torch.Generator().manual_seed(seed)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n_total = self._n_total
        order = torch.randperm(n_total, generator=self._gen) if self.shuffle else torch.arange(n_total)
        order = shard_order(order, self.rank, self.world).to(self.device)
        for i in range(0, order.numel(), self.batch_size):
            idx = order[i:i + self.batch_size]
            yield self._to_tensor(self.images[idx]), self.labels[idx]


# ----------------------------------------------------------------------------- command line
def parser():
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument('--min-digits', type=int, default=0, help='minimum number of digits to add to an image')
    p.add_argument('--max-digits', type=int, default=4, help='maximum number of digits to add to an image')
    p.add_argument('--no-resize', action='store_true', default=False, help='if True, fix the image to be MNIST size')
    p.add_argument('--no-translate', action='store_true', default=False, help='if True, fix the image to be in the center')
    p.add_argument('--fixed', action='store_true', default=False,
                   help='If True, ignore resize/translate options and generate')
    p.add_argument('--scramble', action='store_true', default=False,
                   help='If True, scramble labels and generate. Only does something if fixed is True.')
    p.add_argument('--reverse', action='store_true', default=False,
                   help='If True, reverse flips the labels i.e. 4321 instead of 1234 with 0.5 probability.')
    p.add_argument('--no-repeat', action='store_true', default=False,
                   help='If True, do not generate images with multiple of the same label.')
    p.add_argument('--data-dir', type=str, default='./data',
                   help='where the MNIST IDX files are and where multimnist/{training,test}.pt go [default: ./data]')
    p.add_argument('--n-train', type=int, default=60000, help='training canvases [default: 60000]')
    p.add_argument('--n-test', type=int, default=10000, help='test canvases [default: 10000]')
    p.add_argument('--seed', type=int, default=DEFAULT_SEED, help='seed of the plan draws [default: %d]' % DEFAULT_SEED)
    return p


def parse_args(argv=None):
    """The reference's flags with its four rules (multimnist/datasets.py:316-327): --no-repeat, --scramble and
    --reverse each need --fixed; --scramble overrides --reverse."""
    args = parser().parse_args(argv)
    args.resize = not args.no_resize
    args.translate = not args.no_translate
    for flag in ('no_repeat', 'scramble', 'reverse'):
        if getattr(args, flag) and not args.fixed:
            raise Exception('Must have --fixed if --%s is supplied.' % flag.replace('_', '-'))
    if args.reverse and args.scramble:
        print('Found --reverse and --scramble. Overriding --reverse.')
        args.reverse = False
    _check_digit_range(args.min_digits, args.max_digits)
    return args


def main(argv=None):
    args = parse_args(argv)
    load_mnist(args.data_dir)              # a missing file is reported before anything else
    if not torch.cuda.is_available():
        raise SystemExit('the MultiMNIST dataset builder composes its canvases with a HIP kernel: run it on a ROCm GPU box')
    common = dict(min_digits=args.min_digits, max_digits=args.max_digits, data_dir=args.data_dir,
                  n_train=args.n_train, n_test=args.n_test, seed=args.seed, return_plans=True)
    names = (args.data_dir, MultiMNIST.processed_folder, MultiMNIST.training_file, MultiMNIST.test_file)
    if args.fixed:
        report = make_dataset_fixed(*names, reverse=args.reverse, scramble=args.scramble, no_repeat=args.no_repeat, **common)
    else:
        report = make_dataset(*names, resize=args.resize, translate=args.translate, **common)
    for name in ('train', 'test'):
        print('%s: %d canvases, %d rounds at most per chunk' % (name, len(report[name]['plans']), max(report[name]['rounds'] or [0])))


if __name__ == "__main__":
    main()
