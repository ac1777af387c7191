"""Window layout of backward tracking (``MVTracker.forward(..., backward_tracking=True)``).

Pure host logic (numpy only).  Backward tracking fills the frames BEFORE each query's frame from a second pass that runs the
reference's window loop (mvtracker.py:489-540) in reversed time: frame t of the clip is frame T-1-t of the reversed pass, a query
at frame qt enters at reversed time T-1-qt.  Everything below is that loop restated on the reversed query times:

  * the queries are sorted stably by reversed time (descending query frame),
  * the first reversed window starts at wr = min(T-1-qt), the stride is S/2, no window runs once wr >= T - S/2,
  * at window wr the active tracks are the sorted prefix with T-1-qt < wr + S,
  * slot s of window wr is clip frame max(T-1-wr - s, 0): the kernels read the frame store with frame0 = T-1-wr, frame_step = -1.

The merge rule: a reversed window writes clip frame t of a track only where t < qt -- frames from the query frame on are the
forward pass's.  A track no reversed window reaches (T-1-qt >= the last window's end, i.e. the first S/2 frames or so of the clip:
the forward pass's end-of-clip quirk mirrored) keeps the forward result on its early frames.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def window_prefixes(sorted_t: np.ndarray, S: int, T: int) -> List[Tuple[int, int]]:
    """The reference's window loop on ascending start frames ``sorted_t``: [(window start, active prefix length), ...]."""
    out = []
    if len(sorted_t) == 0:
        return out
    w = int(sorted_t[0])
    while w < T - S // 2:
        out.append((w, int(np.searchsorted(sorted_t, w + S, side="left"))))
        w += S // 2
    return out


def reversed_layout(qt, S: int, T: int) -> dict:
    """qt: integer query frames in the caller's order, all within [0, T-1].

    Returns a dict:
      order      (N,) caller row of every row of the reversed pass (stable sort by T-1-qt)
      sorted_qt  (N,) query frame of every row of the reversed pass (descending)
      windows    [(wr, p1), ...] in execution order: window start in reversed time, active prefix
      frame0     [T-1-wr, ...] the clip frame of slot 0 of every window
      active     number of rows that ever enter a reversed window (a sorted prefix)
    """
    qt = np.asarray(qt, dtype=np.int64).reshape(-1)
    if qt.size and (qt.min() < 0 or qt.max() > T - 1):
        raise ValueError(f"backward tracking needs every query frame within the clip [0, {T - 1}], got [{qt.min()}, {qt.max()}]")
    qr = T - 1 - qt
    order = np.argsort(qr, kind="stable")
    windows = window_prefixes(qr[order], S, T)
    return dict(order=order, sorted_qt=qt[order], windows=windows, frame0=[T - 1 - w for w, _ in windows],
                active=windows[-1][1] if windows else 0)
