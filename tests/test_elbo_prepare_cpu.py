"""CPU: mvae_elbo_reduce_prepare (the ELBO bookkeeping launch that also carries Adam's counter launch) refuses bad
arguments on the host, before anything is launched."""
import ctypes

from mvae_amd import _lib


def _parts(n, groups=2, rows_per_group=4, first_term=0, rows=True):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (_lib.ElboPart * max(n, 1))()
    for q in range(n):
        arr[q] = _lib.ElboPart(p if rows else None, None, None, first_term, groups, rows_per_group)
    return arr, p, buf


def test_bad_arguments_return_the_error_code_without_a_gpu():
    lib = _lib.lib()
    arr, p, _keep = _parts(3)
    tail = (1, 1e-3, 0.9, 0.999)
    # the optimizer half: counter and factor destination are both required
    assert lib.mvae_elbo_reduce_prepare(arr, 3, p, 3, None, 0, None, 0, None, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, 3, p, 3, None, 0, None, 0, p, *tail, None, None) == -1
    # the ELBO half: what mvae_elbo_reduce refuses
    assert lib.mvae_elbo_reduce_prepare(None, 3, p, 3, None, 0, None, 0, p, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, 0, p, 3, None, 0, None, 0, p, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, _lib.ELBO_MAX_PARTS + 1, p, 3, None, 0, None, 0, p, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, 3, None, 3, None, 0, None, 0, p, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, 3, p, 0, None, 0, None, 0, p, *tail, p, None) == -1
    assert lib.mvae_elbo_reduce_prepare(arr, 3, p, 1, None, 0, None, 0, p, *tail, p, None) == -1     # terms 0..1 do not fit T = 1
    no_rows, _, _keep2 = _parts(1, rows=False)
    assert lib.mvae_elbo_reduce_prepare(no_rows, 1, p, 3, None, 0, None, 0, p, *tail, p, None) == -1
    # and mvae_elbo_reduce refuses the same lists
    assert lib.mvae_elbo_reduce(arr, 3, p, 1, None, 0, None, 0, None) == -1
    assert lib.mvae_elbo_reduce(no_rows, 1, p, 3, None, 0, None, 0, None) == -1
