"""CPU restatement (numpy, integer arithmetic) of the MultiMNIST compose step, the checker for
``mvae_multimnist_compose`` (csrc/multimnist_data.hip).

TEST INFRASTRUCTURE: imported only by tests/ and tools/multimnist_data_bench.py.

Written from the description of the step, not copied from the reference: every digit of a canvas is resized
28 x 28 -> w x w with Pillow's 8-bit BILINEAR (``oracle.preprocess.resize_bilinear_u8`` -- for 28 x 28 uint8 inputs
that function equals Pillow 12.2 ``Image.resize((w, w), BILINEAR)`` for every w in 1..50, checked on the CPU in
tests/test_multimnist_data_cpu.py where Pillow imports and pinned by tests/golden/multimnist_data.npz), pasted at
rows top..top+w, columns left..left+w of an integer 50 x 50 canvas, and summed.  flag = max(sum) > 255; the stored
byte is min(sum, 255).  A plan row is int32 [17]: n, then four records (bank index, w, top, left).
"""
import numpy as np

from oracle.preprocess import resize_bilinear_u8

CANVAS, PLAN_STRIDE = 50, 17


def make_plan(canvases):
    """[[(index, w, top, left), ...], ...] -> int32 [M, 17]."""
    plan = np.zeros((len(canvases), PLAN_STRIDE), dtype=np.int32)
    for m, records in enumerate(canvases):
        assert len(records) <= 4
        plan[m, 0] = len(records)
        for d, rec in enumerate(records):
            plan[m, 1 + 4 * d:5 + 4 * d] = rec
    return plan


def compose_sums(bank, row, resize=None, cache=None):
    """The integer canvas of one plan row.  ``resize(digit uint8 [28, 28], w) -> uint8 [w, w]`` replaces the
    restated resample (the golden generator passes Pillow itself); ``cache`` (a dict) keeps resized digits by
    (bank index, w)."""
    if resize is None:
        def resize(digit, w):
            return resize_bilinear_u8(digit[:, :, None], w, w)[:, :, 0]
    sums = np.zeros((CANVAS, CANVAS), dtype=np.int64)
    for d in range(int(row[0])):
        ix, w, top, left = (int(v) for v in row[1 + 4 * d:5 + 4 * d])
        small = None if cache is None else cache.get((ix, w))
        if small is None:
            small = resize(np.asarray(bank[ix], dtype=np.uint8), w)
            assert small.shape == (w, w) and small.dtype == np.uint8
            if cache is not None:
                cache[(ix, w)] = small
        sums[top:top + w, left:left + w] += small
    return sums


def compose(bank, plan, resize=None, cache=None):
    """(canvas uint8 [M, 50, 50], flags int32 [M]) of a plan int [M, 17]."""
    plan = np.asarray(plan)
    canvas = np.zeros((plan.shape[0], CANVAS, CANVAS), dtype=np.uint8)
    flags = np.zeros(plan.shape[0], dtype=np.int32)
    for m in range(plan.shape[0]):
        sums = compose_sums(bank, plan[m], resize, cache)
        flags[m] = 1 if sums.max() > 255 else 0
        canvas[m] = np.minimum(sums, 255).astype(np.uint8)
    return canvas, flags


def composer(digits):
    """The builder's composer hook on the host: ``digits -> (plan -> (canvas, flags))``, resized digits cached."""
    cache = {}
    return lambda plan: compose(digits, plan, cache=cache)


def block_bank(seed=7, n=12):
    """The synthetic bank of the golden and of the tests: ``n`` "digits" with a zero background and a centred 12 x 12
    block of random 130..255; the last two are full-frame noise 0..255."""
    rng = np.random.RandomState(seed)
    bank = np.zeros((n, 28, 28), dtype=np.uint8)
    for i in range(n - 2):
        bank[i, 8:20, 8:20] = rng.randint(130, 256, (12, 12))
    bank[n - 2:] = rng.randint(0, 256, (2, 28, 28))
    return bank


def live_bank():
    """12 digits for the kernel's edge cases: the block bank with entry 0 a saturated block (255), entry 1 a block of
    100 and entry 2 a block of 155 (their sum is exactly 255); entries 10 and 11 are full-frame noise."""
    bank = block_bank(seed=11, n=12)
    for ix, value in ((0, 255), (1, 100), (2, 155)):
        bank[ix, 8:20, 8:20] = value
    return bank


# named rows of live_plans()
EMPTY, SAME_TWICE, ABUT, OVERLAP_ONE_ROW, SUM_255, FOUR_OVERLAPPING, IDENTITY = 38, 39, 40, 41, 42, 43, 44


def live_plans():
    """45 canvases over ``live_bank()``: every width 7..50 at least once, offsets 0 and 50 - w on both axes, w = 50 at
    (0, 0), four digits on one canvas, and the named rows above."""
    def corners(w):
        return [(0, 0), (0, 50 - w), (50 - w, 0), (50 - w, 50 - w)]
    canvases = []
    for w0 in (7, 11):                                   # four small noise digits in the four corners: no overlap
        canvases.append([(10 + (w % 2), w, ) + corners(w)[w - w0] for w in range(w0, w0 + 4)])
    for w in range(15, 51):                              # one digit per canvas, corner by corner; 28 is the identity
        canvases.append([((10, 11, 3, 5)[w % 4], w) + corners(w)[w % 4]])
    assert len(canvases) == 38
    canvases.append([])                                                         # EMPTY
    canvases.append([(4, 20, 0, 0), (4, 20, 30, 30)])                           # SAME_TWICE
    canvases.append([(0, 28, 0, 0), (0, 28, 0, 12)])                            # ABUT: blocks at columns 8..19 and 20..31
    canvases.append([(0, 28, 0, 0), (3, 28, 11, 0)])                            # OVERLAP_ONE_ROW: rows 8..19 and 19..30
    canvases.append([(1, 28, 5, 7), (2, 28, 5, 7)])                             # SUM_255: 100 + 155
    canvases.append([(10, 30, 0, 0), (11, 31, 10, 10), (10, 29, 19, 21), (11, 28, 22, 0)])   # FOUR_OVERLAPPING
    canvases.append([(11, 28, 11, 11)])                                         # IDENTITY
    return make_plan(canvases)
