"""Host-side layout of the grouped forward (mvtracker_amd.grouped.grouped_layout) against a brute-force per-group restatement of
the reference's window loop (mvtracker.py:489-540, 598-711)."""
import numpy as np
import pytest

from mvtracker_amd.grouped import grouped_layout


def _windows_alone(qt, S, T):
    """One group on its own, as forward runs it: [(w, p0, p1)], sorted order."""
    order = np.argsort(qt, kind="stable")
    qs = np.asarray(qt)[order]
    out, w, p0 = [], int(qs.min()), 0
    while w < T - S // 2:
        p1 = int((qs < w + S).sum())
        out.append((w, p0, p1))
        p0 = p1
        w += S // 2
    return out, order


def _check(qts, S, T):
    lay = grouped_layout(qts, S, T)
    base = lay["base"]
    assert base[-1] == sum(len(q) for q in qts)
    per_group = {g: [] for g in range(len(qts))}
    prev_rows = {}
    for wd in lay["windows"]:
        off, rows, carry, out = wd["off"], wd["rows"], wd["carry"], wd["out"]
        assert len(rows) == len(carry) == len(out) == off[-1]
        firsts = {int(lay["first"][g]) for g in wd["groups"]}
        assert len(firsts) == 1  # only groups with the same first window share windows
        key = tuple(wd["groups"])
        for k, g in enumerate(wd["groups"]):
            p0, p1 = int(wd["p0"][k]), int(wd["p1"][k])
            assert off[k + 1] - off[k] == p1
            per_group[g].append((wd["w"], p0, p1))
            sl = slice(off[k], off[k + 1])
            np.testing.assert_array_equal(rows[sl], base[g] + np.arange(p1))
            np.testing.assert_array_equal(out[sl], base[g] + lay["orders"][g][:p1])
            c = carry[sl]
            assert (c[p0:] == -1).all()
            if p0:
                # the carried track i continues from the row of the same track in the previous window of these groups
                pr = prev_rows[key]
                np.testing.assert_array_equal(pr[c[:p0]], base[g] + np.arange(p0))
        assert wd["new_tracks"] == (key not in prev_rows)
        prev_rows[key] = rows
    for g, qt in enumerate(qts):
        ref, order = _windows_alone(qt, S, T)
        assert per_group[g] == ref, (g, per_group[g], ref)
        np.testing.assert_array_equal(lay["orders"][g], order)
        np.testing.assert_array_equal(lay["sorted_src"][base[g]:base[g + 1]], base[g] + order)
        np.testing.assert_array_equal(lay["sorted_qt"][base[g]:base[g + 1]], np.asarray(qt)[order])
        assert lay["active"][g] == (ref[-1][2] if ref else 0)


@pytest.mark.parametrize("S", [8, 12, 16])
@pytest.mark.parametrize("seed", range(6))
def test_grouped_layout_random(S, seed):
    rng = np.random.default_rng(seed * 31 + S)
    T = int(rng.integers(S, 3 * S + 5))
    qts = []
    for g in range(int(rng.integers(1, 7))):
        n = int(rng.integers(1, 40))
        kind = g % 3
        if kind == 0:  # frame 0 present (single_point-like)
            q = np.concatenate([[0], rng.integers(0, T, n - 1)])
        elif kind == 1:  # late-only group (may start past the last window)
            q = rng.integers(T // 2, T, n)
        else:
            q = rng.integers(0, T, n)
        qts.append(q)
    _check(qts, S, T)


def test_grouped_layout_edge_cases():
    S, T = 12, 20
    _check([[0]], S, T)  # one-query group
    _check([[0, 5, 3], [7], [2, 2, 9, 13], [15, 16]], S, T)  # different first windows, one with none at all
    lay = grouped_layout([[15, 16]], S, T)
    assert lay["windows"] == [] and lay["active"].tolist() == [0]
    _check([[3] * 5, [3, 4], [0, 19]], 8, 40)


def test_grouped_layout_rejects_empty():
    with pytest.raises(ValueError):
        grouped_layout([], 12, 20)
    with pytest.raises(ValueError):
        grouped_layout([[0, 1], []], 12, 20)
