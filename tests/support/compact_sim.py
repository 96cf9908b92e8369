"""The pairing rule of cnl_outer_compact_dev (include/cannoles_hip.h) in numpy: which rows change places when the active problems of a
lockstep batch move to the front.

With Bc the working batch and A the number of rows b < Bc with status[b] == 0: fewer than `min_finished` finished rows below Bc and
nothing moves, counts = (A, Bc); otherwise the k-th finished row below A (ascending) and the k-th active row at or above A (ascending)
change places for every k, counts = (A, A).  Rows at or above Bc never move."""
import numpy as np


def compact(status, Bc, min_finished):
    """(perm, counts): row b of an array holds, afterwards, what row perm[b] held — new = old[perm] — for all len(status) rows."""
    status = np.asarray(status)
    B = len(status)
    if not (1 <= Bc <= B and min_finished >= 1):
        raise ValueError("1 <= Bc <= len(status) and min_finished >= 1")
    perm = np.arange(B)
    active = status[:Bc] == 0
    A = int(active.sum())
    if Bc - A < min_finished:
        return perm, (A, Bc)
    finished_below = np.flatnonzero(~active[:A])
    active_above = A + np.flatnonzero(active[A:])
    assert len(finished_below) == len(active_above)
    perm[finished_below], perm[active_above] = active_above, finished_below
    return perm, (A, A)


def apply(perm, array):
    return np.asarray(array)[perm]
