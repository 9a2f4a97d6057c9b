"""Argument rejection of the eight pose-loss entry points (csrc/image.hip: one check, pose_loss_args, serves them all).
The checks are host code and return before anything is launched, so this runs on a machine WITHOUT a device -- and only
there: the pointers below are dummy host addresses that must never reach a GPU."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason='host-side checks only: the dummy addresses must never reach a device')

LF_EINVAL, LF_ENOSPC = -1, -3
N, h, w, H, W = DIMS = 6, 8, 8, 12, 16
# entry point -> number of leading pointer arguments other than the scratch pointer, which follows them
ENTRIES = {'lf_pose_loss_fwd': 8, 'lf_pose_loss_bwd': 7, 'lf_pose_loss_fwd_masked': 7, 'lf_pose_loss_fwd_depth': 8,
           'lf_pose_loss_bwd_depth': 7, 'lf_pose_loss_fwd_mt': 8, 'lf_pose_loss_fwd_masked_mt': 7, 'lf_pose_loss_bwd_mt': 7}
MT = [name for name in ENTRIES if name.endswith('_mt')]


@pytest.fixture(scope='module')
def L():
    from latentfusion_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def addr():
    buf = ctypes.create_string_buffer(64)                          # (a real host address; nothing reads it)
    yield ctypes.addressof(buf)
    del buf


def _call(L, addr, name, null=None, short=0, N=N, tn=(2, 3), h=h, w=w):
    """Calls `name` with valid arguments except: pointer `null` (position; the scratch pointer is the last) is NULL, the
    scratch is `short` bytes short, and N / (T, n) / h / w as given."""
    nptr = ENTRIES[name] + 1
    ptrs = [None if i == null else addr for i in range(nptr)]
    nbytes = L.lf_pose_loss_scratch_bytes(*DIMS) - short
    dims = (N,) + (tuple(tn) if name.endswith('_mt') else ()) + (h, w, H, W)
    return getattr(L, name)(*ptrs, nbytes, *dims, None)


@pytest.mark.parametrize('name', list(ENTRIES))
def test_null_pointer_in_every_position_is_einval(L, addr, name):
    for pos in range(ENTRIES[name] + 1):
        assert _call(L, addr, name, null=pos) == LF_EINVAL, (name, pos)


@pytest.mark.parametrize('name', MT)
@pytest.mark.parametrize('tn', [(0, 3), (2, 0), (2, -3), (-2, -3), (2, 2), (3, 3)])
def test_rows_that_are_not_T_times_n_are_einval(L, addr, name, tn):
    assert _call(L, addr, name, tn=tn) == LF_EINVAL


@pytest.mark.parametrize('name', list(ENTRIES))
def test_degenerate_sizes_are_einval(L, addr, name):
    assert _call(L, addr, name, h=1) == LF_EINVAL
    assert _call(L, addr, name, w=1) == LF_EINVAL
    assert _call(L, addr, name, N=0, tn=(0, 0)) == LF_EINVAL


@pytest.mark.parametrize('name', list(ENTRIES))
def test_short_scratch_is_enospc(L, addr, name):
    assert _call(L, addr, name, short=4) == LF_ENOSPC
