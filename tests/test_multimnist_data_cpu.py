"""No GPU: the host side of the MultiMNIST data path -- the compose entry's ABI and plan validation, the numpy
restatement of the compose step against the Pillow golden (and Pillow live), ``multimnist/utils.py``, the builder's
plan drawing and round driver with the host composer passed in, the ``MultiMNIST`` dataset class, and the
``train.py`` / ``sample.py`` / ``datasets.py`` command lines up to the point where they need a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mvae_amd  # noqa: F401
from mvae_amd import _lib, kernels as K
from mvae_amd.multimnist import datasets as MD, model as MM, sample as MS, train as MT, utils as MU
import multimnist_data_ref as R
from util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- ABI
def test_compose_symbol_is_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert 'mvae_multimnist_compose' in _lib._SIGNATURES and hasattr(handle, 'mvae_multimnist_compose')
    assert len(_lib._SIGNATURES['mvae_multimnist_compose'][1]) == 9
    assert _lib.lib().mvae_abi_version() == 6
    assert (K.MM_DIGIT, K.MM_CANVAS, K.MM_MAX_DIGITS, K.MM_PLAN_STRIDE, K.MM_WMIN, K.MM_WMAX, K.MM_KSIZE) == \
        (28, 50, 4, 17, 7, 50, 9)
    header = open(os.path.join(ROOT, 'include', 'mvae_hip.h')).read()
    for name in ('DIGIT', 'CANVAS', 'MAX_DIGITS', 'PLAN_STRIDE', 'WMIN', 'WMAX', 'KSIZE'):
        assert int(re.search(r'#define\s+MVAE_MM_%s\s+(\d+)' % name, header).group(1)) == getattr(K, 'MM_' + name), name
    # the widest table row: 28 -> 7 takes ceil(4) * 2 + 1 = 9 taps, and upsampling keeps 3
    assert _lib.lib().mvae_resample_ksize(28, 7) == 9 and _lib.lib().mvae_resample_ksize(28, 50) == 3


def test_compose_refuses_null_and_empty_calls_on_the_host():
    lib = _lib.lib()
    buf = (ctypes.c_int * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mvae_multimnist_compose(None, 12, p, 1, p, p, p, p, None) == -1
    for hole in range(6):
        ptrs = [p] * 6
        ptrs[hole] = None
        bank, plan, kk, bounds, canvas, flags = ptrs
        assert lib.mvae_multimnist_compose(bank, 12, plan, 1, kk, bounds, canvas, flags, None) == -1, hole
    assert lib.mvae_multimnist_compose(p, 12, p, 0, p, p, p, p, None) == -1          # M <= 0
    assert lib.mvae_multimnist_compose(p, 12, p, -3, p, p, p, p, None) == -1
    assert lib.mvae_multimnist_compose(p, 0, p, 1, p, p, p, p, None) == -1           # n_bank <= 0
    odd = ctypes.c_void_p(p.value + 1)                                               # whole-dword loads and stores
    assert lib.mvae_multimnist_compose(odd, 12, p, 1, p, p, p, p, None) == -1
    assert lib.mvae_multimnist_compose(p, 12, p, 1, p, p, odd, p, None) == -1


GOOD = [(3, 20, 5, 30), (0, 7, 43, 0), (11, 50, 0, 0), (5, 28, 22, 22)]
DEFECTS = [
    ('digit count', lambda p: p.__setitem__((0, 0), 5)),
    ('digit count', lambda p: p.__setitem__((0, 0), -1)),
    ('bank index', lambda p: p.__setitem__((0, 1), 12)),
    ('bank index', lambda p: p.__setitem__((0, 1), -1)),
    ('width', lambda p: p.__setitem__((0, 2), 6)),
    ('width', lambda p: p.__setitem__((0, 10), 51)),
    ('rows', lambda p: p.__setitem__((0, 3), -1)),
    ('rows', lambda p: p.__setitem__((0, 3), 31)),           # 31 + 20 > 50
    ('columns', lambda p: p.__setitem__((0, 8), -2)),
    ('columns', lambda p: p.__setitem__((0, 8), 44)),        # 44 + 7 > 50
]


@pytest.mark.parametrize('what,spoil', DEFECTS)
def test_compose_validates_the_plan_before_it_looks_for_a_gpu(what, spoil):
    bank = torch.zeros(12, 28, 28, dtype=torch.uint8)          # a host tensor: a valid plan gets as far as the GPU check
    plan = R.make_plan([GOOD])
    with pytest.raises(RuntimeError, match='GPU'):
        K.multimnist_compose(bank, plan)
    spoil(plan)
    with pytest.raises(ValueError, match=what):
        K.multimnist_compose(bank, plan)


def test_plan_validation_ignores_unused_records_and_checks_the_shape():
    plan = R.make_plan([GOOD[:2]])
    plan[0, 9:] = -7                                             # records past n are never read
    assert K.multimnist_validate_plan(plan, 12).dtype == np.int32
    with pytest.raises(ValueError, match='plan must be'):
        K.multimnist_validate_plan(np.zeros((3, 16), dtype=np.int32), 12)
    with pytest.raises(ValueError, match='plan must be'):
        K.multimnist_validate_plan(np.zeros((0, 17), dtype=np.int32), 12)
    with pytest.raises(ValueError, match='bank'):
        K.multimnist_compose(torch.zeros(12, 28, 27, dtype=torch.uint8), plan)


# ----------------------------------------------------------------------------- the reference composer
def test_reference_composer_reproduces_the_pillow_golden(golden_dir):
    fx, meta = load_golden(golden_dir, 'multimnist_data')
    assert np.array_equal(fx['bank'], R.block_bank(seed=7, n=12)) and fx['plan'].shape == (meta['M'], 17)
    assert 0 < meta['flagged'] < meta['M']
    K.multimnist_validate_plan(fx['plan'], meta['n_bank'])
    canvas, flags = R.compose(fx['bank'], fx['plan'])
    assert np.array_equal(flags, fx['flags']) and np.array_equal(canvas, fx['canvas'])
    canvas2, flags2 = R.composer(fx['bank'])(fx['plan'])
    assert np.array_equal(flags2, fx['flags']) and np.array_equal(canvas2, fx['canvas'])


def test_reference_composer_matches_pillow_live():
    Image = pytest.importorskip('PIL.Image')

    def pillow(digit, w):
        return np.asarray(Image.fromarray(digit).resize((w, w), Image.BILINEAR), dtype=np.uint8)
    rng = np.random.RandomState(5)
    noise = rng.randint(0, 256, (2, 28, 28)).astype(np.uint8)
    for w in range(1, 51):                                       # the resample alone, every width
        for digit in noise:
            assert np.array_equal(R.resize_bilinear_u8(digit[:, :, None], w, w)[:, :, 0], pillow(digit, w)), w
    assert np.array_equal(pillow(noise[0], 28), noise[0])        # 28 is the identity
    bank = R.live_bank()
    plans = [R.live_plans()]
    fresh = []
    for m in range(30):
        records = []
        for _ in range(m % 5):
            w = int(rng.randint(7, 51))
            records.append((int(rng.randint(12)), w, int(rng.randint(0, 51 - w)), int(rng.randint(0, 51 - w))))
        fresh.append(records)
    plans.append(R.make_plan(fresh))
    for plan in plans:
        want = R.compose(bank, plan, resize=pillow)
        got = R.compose(bank, plan)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_live_plans_hold_the_cases_they_are_named_for():
    bank, plan = R.live_bank(), R.live_plans()
    assert plan.shape == (45, 17) and bank.shape == (12, 28, 28)
    K.multimnist_validate_plan(plan, 12)
    widths = {int(plan[m, 2 + 4 * d]) for m in range(45) for d in range(plan[m, 0])}
    assert widths == set(range(7, 51))
    recs = [tuple(plan[m, 1 + 4 * d:5 + 4 * d]) for m in range(45) for d in range(plan[m, 0])]
    assert any(w == 50 and (t, l) == (0, 0) for _, w, t, l in recs)
    assert any(t == 0 for _, w, t, l in recs) and any(l == 0 for _, w, t, l in recs)
    assert any(t == 50 - w and w < 50 for _, w, t, l in recs) and any(l == 50 - w and w < 50 for _, w, t, l in recs)
    assert plan[R.EMPTY, 0] == 0 and (plan[:, 0] == 4).sum() == 3
    assert plan[R.SAME_TWICE, 1] == plan[R.SAME_TWICE, 5]
    canvas, flags = R.compose(bank, plan)
    assert not canvas[R.EMPTY].any() and flags[R.EMPTY] == 0
    assert flags[R.ABUT] == 0 and (canvas[R.ABUT][8:20, 8:32] == 255).all() and canvas[R.ABUT].sum() == 255 * 12 * 24
    assert flags[R.OVERLAP_ONE_ROW] == 1
    sums = R.compose_sums(bank, plan[R.OVERLAP_ONE_ROW])
    assert (sums > 255).any(axis=1).sum() == 1                   # exactly one pixel row overlaps
    assert flags[R.SUM_255] == 0 and canvas[R.SUM_255].max() == 255 and R.compose_sums(bank, plan[R.SUM_255]).max() == 255
    assert flags[R.FOUR_OVERLAPPING] == 1
    assert np.array_equal(canvas[R.IDENTITY][11:39, 11:39], bank[11]) and flags[R.IDENTITY] == 0
    assert flags[:38].sum() == 0


# ----------------------------------------------------------------------------- utils
def test_utils_constants_and_conversions():
    for name in ('max_length', 'all_characters', 'n_characters', 'SOS', 'FILL'):
        assert getattr(MU, name) is getattr(MM, name), name
    assert (MU.max_length, MU.all_characters, MU.n_characters, MU.SOS, MU.FILL) == (4, '0123456789', 12, 10, 11)
    t = MU.char_tensor('17')
    assert t.dtype == torch.int64 and t.tolist() == [1, 7, MU.FILL, MU.FILL]
    assert MU.char_tensor('').tolist() == [MU.FILL] * 4 and MU.char_tensor('9081').tolist() == [9, 0, 8, 1]
    assert MU.charlist_tensor([3, 0, 9]).tolist() == [3, 0, 9, MU.FILL]
    assert MU.charlist_tensor([torch.tensor(4), torch.tensor(2)]).tolist() == [4, 2, MU.FILL, MU.FILL]
    assert MU.tensor_to_string(torch.tensor([MU.SOS, 1, MU.FILL, 7])) == '^17'
    assert MU.tensor_to_string(MU.char_tensor('305')) == '305'
    assert [MU.index_to_char(i) for i in (0, 9, MU.SOS, MU.FILL)] == ['0', '9', '^', '']
    with pytest.raises(IndexError):
        MU.char_tensor('12345')


# ----------------------------------------------------------------------------- plan drawing
def _mnist(n=12, seed=7):
    return {'digits': R.block_bank(seed=seed, n=n), 'labels': np.arange(n) % 10}


def _accept_all(plan):
    return np.zeros((len(plan), 50, 50), dtype=np.uint8), np.zeros(len(plan), dtype=np.int32)


def test_plan_drawing_is_deterministic_and_always_valid():
    mnist = _mnist()
    runs = [MD.mk_dataset(200, mnist, 0, 4, 50, composer=_accept_all, rng=np.random.RandomState(3), return_plans=True)
            for _ in range(2)]
    assert np.array_equal(runs[0][2], runs[1][2]) and runs[0][1] == runs[1][1]
    other = MD.mk_dataset(200, mnist, 0, 4, 50, composer=_accept_all, rng=np.random.RandomState(4), return_plans=True)
    assert not np.array_equal(runs[0][2], other[2])
    x, y, plans, stats = runs[0]
    K.multimnist_validate_plan(plans, 12)
    assert x.shape == (200, 50, 50) and x.dtype == np.uint8 and stats['rounds'] == [1] and stats['redrawn'] == []
    assert set(plans[:, 0]) == {0, 1, 2, 3, 4}
    for m in range(200):
        assert len(y[m]) == plans[m, 0]
        assert y[m] == [int(mnist['labels'][plans[m, 1 + 4 * d]]) for d in range(plans[m, 0])]
    widths = np.array([plans[m, 2 + 4 * d] for m in range(200) for d in range(plans[m, 0])])
    assert 14 <= widths.min() and widths.max() <= 34 and len(set(widths)) > 5        # int(28 / N(1.3, 0.1))
    # the default stream is RandomState(681307)
    a = MD.mk_dataset(20, mnist, 0, 2, 50, composer=_accept_all, return_plans=True)[2]
    b = MD.mk_dataset(20, mnist, 0, 2, 50, composer=_accept_all, rng=np.random.RandomState(681307), return_plans=True)[2]
    assert np.array_equal(a, b) and MD.DEFAULT_SEED == 681307 and a[:, 0].max() <= 2


def test_plan_drawing_without_resize_and_without_translate():
    mnist = _mnist()
    plans = MD.mk_dataset(100, mnist, 1, 4, 50, resize=False, composer=_accept_all, rng=np.random.RandomState(1),
                          return_plans=True)[2]
    recs = np.array([plans[m, 1 + 4 * d:5 + 4 * d] for m in range(100) for d in range(plans[m, 0])])
    assert (recs[:, 1] == 28).all() and recs[:, 2].max() <= 21 and len(set(recs[:, 2])) > 5
    plans = MD.mk_dataset(100, mnist, 1, 4, 50, translate=False, composer=_accept_all, rng=np.random.RandomState(1),
                          return_plans=True)[2]
    recs = np.array([plans[m, 1 + 4 * d:5 + 4 * d] for m in range(100) for d in range(plans[m, 0])])
    assert (recs[:, 2] == (50 - recs[:, 1]) // 2).all() and (recs[:, 3] == (50 - recs[:, 1]) // 2).all()
    assert len(set(recs[:, 1])) > 5


def test_fixed_mode_plans_and_label_options():
    mnist = _mnist(n=40)
    x, y, plans, _ = MD.mk_dataset_fixed(120, mnist, 0, 4, 50, composer=_accept_all, rng=np.random.RandomState(2),
                                         return_plans=True)
    assert MD.FIXED_W == 21 and MD.FIXED_PADS == [(4, 4), (4, 23), (23, 4), (23, 23)]
    for m in range(120):
        for d in range(plans[m, 0]):
            assert tuple(plans[m, 2 + 4 * d:5 + 4 * d]) == (21,) + MD.FIXED_PADS[d]
        assert y[m] == [int(mnist['labels'][plans[m, 1 + 4 * d]]) for d in range(plans[m, 0])]
    y = MD.mk_dataset_fixed(120, mnist, 0, 4, 50, no_repeat=True, composer=_accept_all, rng=np.random.RandomState(2))[1]
    assert all(len(set(row)) == len(row) for row in y) and any(len(row) == 4 for row in y)
    for kw in ({'scramble': True}, {'reverse': True}):
        x, y, plans, _ = MD.mk_dataset_fixed(120, mnist, 2, 4, 50, composer=_accept_all, rng=np.random.RandomState(2),
                                             return_plans=True, **kw)
        drawn = [[int(mnist['labels'][plans[m, 1 + 4 * d]]) for d in range(plans[m, 0])] for m in range(120)]
        assert all(sorted(a) == sorted(b) for a, b in zip(y, drawn)) and y != drawn
        if 'reverse' in kw:
            assert all(a == b or a == b[::-1] for a, b in zip(y, drawn))


def test_more_than_four_digits_and_the_command_line_rules(capsys):
    mnist = _mnist()
    with pytest.raises(ValueError, match='max_digits'):
        MD.mk_dataset(4, mnist, 0, 5, 50, composer=_accept_all)
    with pytest.raises(ValueError, match='max_digits'):
        MD.mk_dataset_fixed(4, mnist, 0, 5, 50, composer=_accept_all)
    with pytest.raises(ValueError, match='max_digits'):
        MD.parse_args(['--max-digits', '5'])
    for flag in ('--no-repeat', '--scramble', '--reverse'):
        with pytest.raises(Exception, match='Must have --fixed if %s is supplied' % flag):
            MD.parse_args([flag])
        assert getattr(MD.parse_args([flag, '--fixed']), flag[2:].replace('-', '_')) is True
    args = MD.parse_args(['--fixed', '--reverse', '--scramble'])
    assert args.scramble and not args.reverse and 'Overriding' in capsys.readouterr().out
    args = MD.parse_args([])
    assert (args.min_digits, args.max_digits, args.resize, args.translate, args.fixed) == (0, 4, True, True, False)
    assert (args.data_dir, args.n_train, args.n_test, args.seed) == ('./data', 60000, 10000, 681307)
    args = MD.parse_args(['--no-resize', '--no-translate'])
    assert not args.resize and not args.translate


def test_builder_without_mnist_files_says_so(tmp_path):
    with pytest.raises(SystemExit, match='IDX'):
        MD.load_mnist(str(tmp_path))
    with pytest.raises(SystemExit, match='IDX'):
        MD.main(['--data-dir', str(tmp_path)])


# ----------------------------------------------------------------------------- round driver
def test_round_driver_redraws_only_flagged_canvases_and_terminates():
    mnist = _mnist()
    host = R.composer(mnist['digits'])
    calls = []

    def recording(plan):
        out = host(plan)
        calls.append((np.array(plan), out[1].copy()))
        return out
    x, y, plans, stats = MD.mk_dataset(64, mnist, 0, 4, 50, composer=recording, rng=np.random.RandomState(681307),
                                       return_plans=True)
    # observed: 25 rounds with this bank and seed.  The block bank rejects about 37 % / 75 % / 94 % of the 2- / 3- / 4-digit
    # canvases drawn at the defaults (1500 draws each), so the last 4-digit canvas of ~13 takes a few dozen rounds.
    assert stats['rounds'] == [len(calls)] and 1 < len(calls) < 300, stats
    assert calls[0][0].shape == (64, 17)
    todo = np.arange(64)
    counts = calls[0][0][:, 0].copy()
    accepted = {}
    for plan, flags in calls:
        assert len(plan) == len(todo)                                  # only the flagged canvases come back
        assert np.array_equal(plan[:, 0], counts[todo])                # each keeps its digit count
        for m, row in zip(todo[flags == 0], plan[flags == 0]):
            accepted[int(m)] = row
        todo = todo[flags != 0]
    assert todo.size == 0 and sorted(accepted) == list(range(64))
    assert stats['redrawn'] == [len(p) for p, _ in calls[1:]]
    for m in range(64):
        assert np.array_equal(plans[m], accepted[m])                   # the reported plan is the accepted one
        assert len(y[m]) == plans[m, 0]
    canvas, flags = R.compose(mnist['digits'], plans)
    assert not flags.any() and np.array_equal(canvas, x)               # no canvas above 255, and the stored bytes are its own


def test_round_driver_gives_up_at_the_cap():
    mnist = _mnist()
    n_calls = [0]

    def flag_everything(plan):
        n_calls[0] += 1
        return np.zeros((len(plan), 50, 50), dtype=np.uint8), np.ones(len(plan), dtype=np.int32)
    with pytest.raises(RuntimeError, match='1000 rounds'):
        MD.mk_dataset(3, mnist, 1, 1, 50, composer=flag_everything, rng=np.random.RandomState(0))
    assert n_calls[0] == MD.MAX_ROUNDS == 1000


def test_chunks_are_at_most_8192_canvases():
    sizes = []

    def accept(plan):
        sizes.append(len(plan))
        return _accept_all(plan)
    assert MD.CHUNK == 8192
    x, y = MD.mk_dataset(8200, _mnist(), 0, 0, 50, composer=accept, rng=np.random.RandomState(0))
    assert sizes == [8192, 8] and x.shape == (8200, 50, 50) and y == [[]] * 8200


# ----------------------------------------------------------------------------- dataset class
def _write_split(folder, name, n, rng, as_tensors=False):
    data = torch.from_numpy(rng.randint(0, 256, (n, 50, 50)).astype(np.uint8))
    labels = [[int(v) for v in rng.randint(0, 10, rng.randint(0, 5))] for _ in range(n)]
    stored = [[torch.tensor(v) for v in row] for row in labels] if as_tensors else labels
    torch.save((data, stored), str(folder / name))
    return data, labels


def test_multimnist_dataset_class(tmp_path):
    with pytest.raises(RuntimeError, match='Dataset not found'):
        MD.MultiMNIST(str(tmp_path))
    folder = tmp_path / 'multimnist'
    folder.mkdir()
    rng = np.random.RandomState(0)
    train, train_labels = _write_split(folder, 'training.pt', 7, rng)
    with pytest.raises(RuntimeError, match='Dataset not found'):      # both files are needed
        MD.MultiMNIST(str(tmp_path))
    test, test_labels = _write_split(folder, 'test.pt', 3, rng, as_tensors=True)
    assert (MD.MultiMNIST.processed_folder, MD.MultiMNIST.training_file, MD.MultiMNIST.test_file) == \
        ('multimnist', 'training.pt', 'test.pt')
    ds = MD.MultiMNIST(str(tmp_path), train=True, download=True)        # the files exist: nothing is built
    assert len(ds) == 7 and torch.equal(ds.train_data, train) and ds.train_labels == train_labels
    dt = MD.MultiMNIST(str(tmp_path), train=False, target_transform=MU.charlist_tensor)
    assert len(dt) == 3 and torch.equal(dt.test_data, test) and dt.test_labels == test_labels
    assert all(isinstance(v, int) for row in dt.test_labels for v in row)
    pytest.importorskip('PIL.Image')
    img, target = ds[2]
    assert img.mode == 'L' and img.size == (50, 50) and np.array_equal(np.asarray(img), train[2].numpy())
    assert target == train_labels[2]
    img, target = dt[1]
    assert target.tolist() == MU.charlist_tensor(test_labels[1]).tolist()
    seen = []
    MD.MultiMNIST(str(tmp_path), transform=lambda im: seen.append(im.size) or 5)[0]
    assert seen == [(50, 50)]


def test_make_dataset_with_the_host_composer(tmp_path):
    """The builder end to end without a GPU: tiny IDX files, the host composer passed in as the factory."""
    from test_loader_cpu import write_idx
    bank = R.block_bank(seed=3, n=40)
    write_idx(str(tmp_path / 'train-images-idx3-ubyte'), bank[:28])
    write_idx(str(tmp_path / 'train-labels-idx1-ubyte'), np.arange(28) % 10)
    write_idx(str(tmp_path / 't10k-images-idx3-ubyte'), bank[28:])
    write_idx(str(tmp_path / 't10k-labels-idx1-ubyte'), np.arange(12) % 10)
    out = tmp_path / 'out'
    report = MD.make_dataset(str(out), 'multimnist', 'training.pt', 'test.pt', max_digits=3, data_dir=str(tmp_path),
                             n_train=20, n_test=6, seed=1, composer=R.composer, return_plans=True)
    assert MD.make_dataset(str(out), 'multimnist', 'training.pt', 'test.pt', max_digits=1, data_dir=str(tmp_path),
                           n_train=2, n_test=2, seed=1, composer=R.composer) is None
    report = MD.make_dataset(str(out), 'multimnist', 'training.pt', 'test.pt', max_digits=3, data_dir=str(tmp_path),
                             n_train=20, n_test=6, seed=1, composer=R.composer, return_plans=True)
    for train, digits, n in ((True, bank[:28], 20), (False, bank[28:], 6)):
        ds = MD.MultiMNIST(str(out), train=train)
        rep = report['train' if train else 'test']
        data, labels = ds._split()
        assert len(ds) == n and rep['plans'].shape == (n, 17) and max(rep['rounds']) < 300
        canvas, flags = R.compose(digits, rep['plans'])
        assert not flags.any() and np.array_equal(canvas, data.numpy())
        assert [len(row) for row in labels] == rep['plans'][:, 0].tolist()


# ----------------------------------------------------------------------------- train.py / sample.py
def test_train_without_the_files_names_the_dataset_builder(tmp_path):
    with pytest.raises(SystemExit, match='dataset builder') as e:
        MT.main(['--data-dir', str(tmp_path)])
    assert 'datasets.py' in str(e.value) and str(tmp_path) in str(e.value)


def test_sample_parser_and_need_cuda(tmp_path):
    args = MS.parser().parse_args(['m.pth.tar'])
    assert (args.model_path, args.n_samples, args.condition_on_image, args.condition_on_text, args.cuda) == \
        ('m.pth.tar', 64, None, None, False)
    assert (args.image_file, args.synthetic, args.out_dir, args.data_dir) == (None, False, '.', './data')
    args = MS.parser().parse_args(['m', '--condition-on-text', '1773', '--condition-on-image', '07', '--n-samples', '8'])
    assert (args.condition_on_text, args.condition_on_image, args.n_samples) == ('1773', '07', 8)
    for bad in ('12345', '1a'):
        with pytest.raises(SystemExit):
            MS.parser().parse_args(['m', '--condition-on-text', bad])
    with pytest.raises(SystemExit, match='pass --cuda'):
        MS.main([str(tmp_path / 'missing.pth.tar')])
    assert MS.fetch_multimnist_text('17').tolist() == [[1, 7, MU.FILL, MU.FILL]]
    words = torch.zeros(2, 4, 12)
    words[0, 0, 3] = words[0, 1, 10] = words[0, 2, 11] = words[0, 3, 0] = 5.0
    words[1, 0, 7] = words[1, 1:, 11] = 5.0
    assert MS.tokens_to_strings(words) == ['3^0', '7']
    words = torch.randn(6, 4, 12)                                  # the dim=1 quirk: soft-max over the positions
    shifted = words - torch.logsumexp(words, dim=1, keepdim=True)
    assert MS.tokens_to_strings(words) == [''.join(MU.index_to_char(i) for i in row) for row in shifted.argmax(2).tolist()]
