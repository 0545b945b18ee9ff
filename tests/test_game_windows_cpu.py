"""The window arithmetic of k_game_fast's baseline roles (csrc/game_windows.h), checked exhaustively against `/` and `%`.

A baseline role takes `w / nslots` and `w % nslots` of every window of the minibatch, and the number of windows of its slot,
from a reciprocal of the run-time nslots instead of dividing.  mmg_game_window_split / mmg_game_window_counts run the very inline
functions the kernel calls (no GPU).  Range: the host gives a launch at most ceil(T B / 16) <= 60 slots and the role keeps 64
windows per slot, so nslots = 1..64 with w < 64 nslots, and nw <= 64 nslots for every slot < nslots."""
import ctypes as C

import numpy as np
import pytest

from multimodalgame_amd import _lib

NSLOTS = range(1, 65)


def test_quotient_and_remainder_of_every_window():
    for nslots in NSLOTS:
        w = np.arange(64 * nslots)
        kw, slot = _lib.game_window_split(nslots, len(w))
        np.testing.assert_array_equal(kw, w // nslots, err_msg="nslots %d" % nslots)
        np.testing.assert_array_equal(slot, w % nslots, err_msg="nslots %d" % nslots)


def test_window_count_of_every_slot():
    for nslots in NSLOTS:
        nw = np.arange(64 * nslots + 1)                                  # nw <= 64 nslots
        for slot in range(nslots):
            want = np.where(nw > slot, (nw - slot + nslots - 1) // nslots, 0)       # kernels_game.h before the reciprocal
            np.testing.assert_array_equal(_lib.game_window_counts(nslots, slot, len(nw)), want, err_msg="nslots %d slot %d" % (nslots, slot))
            # ... which is the number of w < nw with w % nslots == slot
            assert want[-1] == 64 and want[nslots] == 1 and want[slot] == 0


def test_arguments_out_of_range_are_refused():
    lib = _lib.load()
    buf = (C.c_int32 * 8)()
    for nslots in (0, -1, 65):
        assert lib.mmg_game_window_split(nslots, 4, buf, buf) < 0 and b"nslots" in lib.mmg_last_error()
        assert lib.mmg_game_window_counts(nslots, 0, 4, buf) < 0
    assert lib.mmg_game_window_split(2, 2 * 64 + 2, buf, buf) < 0               # n beyond 64 nslots + 1
    assert lib.mmg_game_window_split(2, 4, None, buf) < 0
    assert lib.mmg_game_window_counts(2, 2, 4, buf) < 0 and lib.mmg_game_window_counts(2, -1, 4, buf) < 0
    with pytest.raises(_lib.MmgError, match="nslots"):
        _lib.game_window_split(65, 1)
    assert lib.mmg_version() == 3                                             # additive: the ABI version stays
