"""Row limits of the plane paths, host only: the row-paired planes (option rh1_planes) accept exactly the x_mpad
values the one-launch R-forward (rfwd01) accepts, so the default-on path cannot throw where the fallback runs."""
import ctypes

import pytest


def _ok(x_mpad):
    from trpo_amd import _lib
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib.trpo_plane_rows_ok(x_mpad, ctypes.byref(a), ctypes.byref(b)), "trpo_plane_rows_ok")
    return a.value, b.value


@pytest.mark.parametrize("x_mpad", [256, 512, 3072, 1 << 20, (1 << 23) - 512, (1 << 23) - 256, 1 << 23,
                                    (1 << 23) + 256, 1 << 24])
def test_pair_planes_take_the_rows_rfwd01_takes(x_mpad):
    rf, pp = _ok(x_mpad)
    assert rf == pp
    assert rf == (1 if x_mpad < (1 << 23) else 0)   # 4 k-blocks of x_mpad 64-B rows under 2^31 bytes


def test_boundary_batch_sizes():
    """n in (2^23 - 256, 2^23] rounds up to x_mpad = 2^23: outside both; n = 2^23 - 256 is the last one inside."""
    pad = lambda n: (n + 255) // 256 * 256
    assert _ok(pad((1 << 23) - 256)) == (1, 1)
    assert _ok(pad((1 << 23) - 255)) == (0, 0)
    assert _ok(pad(1 << 23)) == (0, 0)
