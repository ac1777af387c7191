"""Row layout of a grouped forward (``MVTracker.forward_grouped``): G independent query sets through one launch sequence.

Pure host logic (numpy only).  Every group follows the reference's window semantics on its own (mvtracker.py:489-540,
598-711): its queries sorted stably by query frame, its first window at w_g = int(min qt_g), window stride S/2, at window w the
active tracks are the sorted prefix with t < w + S, no window at all once w >= T - S/2.  Groups with equal w_g share their
windows; a window's rows are the concatenation of every member group's active prefix, group by group.

Three index spaces:
  * caller rows   -- the groups' query lists concatenated in the caller's order: group g owns [base[g], base[g] + N_g)
  * sorted rows   -- the same ranges, each group sorted by query frame (``sorted_src[r]`` = caller row of sorted row r)
  * window rows   -- the rows of one window: group g's active prefix at [off[k], off[k + 1]) for the k-th member group
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np


def grouped_layout(qts: Sequence[Sequence[int]], S: int, T: int) -> dict:
    """qts: the integer query frames of every group, in the caller's order (no group may be empty).

    Returns a dict:
      base        (G + 1,) caller / sorted row offsets of the groups
      orders      per group: the stable argsort of its query frames
      sorted_src  (N,) caller row of every sorted row
      sorted_qt   (N,) query frame of every sorted row
      first       (G,) w_g of every group
      active      (G,) sorted rows [base[g], base[g] + active[g]) ever enter a window (the rest keep zero outputs)
      windows     in execution order: dict(w, groups (member group ids), p0 / p1 (per member: carried / active prefix),
                  off (row offsets of the members, len + 1), rows (sorted row of every window row), carry (row of the previous
                  window of the same members this row continues from, -1 for a track that enters here: window_prepare's
                  carry_src), out (caller row of
                  every window row: the un-sort map of window_store), new_tracks (bool: the window follows no earlier one))
    """
    G = len(qts)
    if G == 0:
        raise ValueError("forward_grouped needs at least one group")
    qts = [np.asarray(q, dtype=np.int64).reshape(-1) for q in qts]
    for g, q in enumerate(qts):
        if q.size == 0:
            raise ValueError(f"group {g} has no queries")
    base = np.zeros(G + 1, dtype=np.int64)
    base[1:] = np.cumsum([q.size for q in qts])
    orders = [np.argsort(q, kind="stable") for q in qts]
    sorted_src = np.concatenate([base[g] + orders[g] for g in range(G)])
    sorted_qt = np.concatenate([qts[g][orders[g]] for g in range(G)])
    first = np.array([int(q.min()) for q in qts], dtype=np.int64)
    active = np.zeros(G, dtype=np.int64)
    windows: List[dict] = []
    half = S // 2
    for w0 in sorted(set(first.tolist())):
        members = [g for g in range(G) if first[g] == w0]
        w = w0
        p0 = np.zeros(len(members), dtype=np.int64)
        prev_off = None
        while w < T - half:
            p1 = np.array([int(np.searchsorted(sorted_qt[base[g]:base[g + 1]], w + S, side="left")) for g in members], dtype=np.int64)
            off = np.zeros(len(members) + 1, dtype=np.int64)
            off[1:] = np.cumsum(p1)
            rows = np.concatenate([base[g] + np.arange(p1[k]) for k, g in enumerate(members)])
            carry = np.concatenate([np.where(np.arange(p1[k]) < p0[k], (prev_off[k] if prev_off is not None else 0) + np.arange(p1[k]), -1)
                                    for k in range(len(members))])
            windows.append(dict(w=w, groups=list(members), p0=p0.copy(), p1=p1, off=off, rows=rows, carry=carry,
                                out=sorted_src[rows], new_tracks=prev_off is None))
            for k, g in enumerate(members):
                active[g] = p1[k]
            prev_off, p0 = off, p1
            w += half
    return dict(base=base, orders=orders, sorted_src=sorted_src, sorted_qt=sorted_qt, first=first, active=active, windows=windows)
