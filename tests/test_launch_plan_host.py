"""The launch plans of the updater's block and attention kernels (mvtracker_amd/csrc/launch_plan.h), checked on the CPU.

The header is the one statement of every launch rule: the entries of block_fused.hip and attention_mfma.hip launch what it returns and
updater.hip asks it which forms its sequence takes.  It is HIP-free, so the host compiler alone builds tests/launch_plan_probe.cpp
around it; the probe runs ONCE over every case below and the tests compare its answers with

  * the dispatch restatements that the exact GPU suites select their cases by -- block_forms / ln_proj_form
    (test_gpu_matmul_exact.py), forms (test_gpu_updater_wiring_exact.py), form_of (test_gpu_attention_forms.py): a threshold edited
    in the header and not in a restatement (or the other way round) fails here, not as a green suite that no longer runs the new
    side of the threshold;
  * the launch table written out below (template triple and grid of every form): the record of what the entries launched before
    the rules moved into the header.  A wrong grid on these kernels is an out-of-bounds access, not a failed assertion, so this
    test comes before any GPU run.
"""
import itertools

import pytest

import test_gpu_attention_forms as AF
import test_gpu_matmul_exact as MM
import test_gpu_updater_wiring_exact as UW
from plan_probe import run_probe

H = 1024  # the MLP width of the updater's blocks


def cdiv(a, b):
    return (a + b - 1) // b


def sw(nmb="rule", nosplit=0, time_small=1, frame_small=1):
    """The probe's five switch fields: nmb_forced nmb_force no_split time_small frame_small."""
    return f"{int(nmb != 'rule')} {0 if nmb == 'rule' else nmb} {int(nosplit)} {int(time_small)} {int(frame_small)}"


# ------------------------------------------------------------------ the sweeps

BLOCK_M = (1, 31, 32, 33, 64, 2016, 2048, 2049, 2080, 4095, 4096, 12288)
BLOCK_CASES = [(M, ws, nmb, nosplit, slices) for M in BLOCK_M for ws in (0, 1) for nmb in ("rule", 1, 2) for nosplit in (0, 1) for slices in (1, 4)]
LN_CASES = [(M, slices) for M in BLOCK_M for slices in (1, 3)]
NEXTS = [(), (288,), (864,), (576, 288, 288), (1, 256), (257,), (1024, 32, 33)]

UPD_S, UPD_G, UPD_N = (7, 8, 12, 16, 32), (1, 2, 4), range(1, 801)
UPD_CASES = list(itertools.product(UPD_S, UPD_G, range(64), (0, 1), (0, 1)))  # (S, G, mask, time_small, frame_small), every n each

ATTN_CASES = list(itertools.product((1, 7, 12, 32, 43), (1, 64, 65, 740), (1, 64, 511, 512, 513, 640, 1024), (0, 1)))

# (n tracks, S, G) -> the time block over all rows; on both sides of 256 small tiles at every S, with and without the switch
TIME_CASES = [((n + 64 * G) * S, S, ws, ts) for S in UPD_S + (1, 33, 64) for n in (1, 21, 342, 448, 449, 512, 740, 2000) for G in (1, 2)
              for ws in (0, 1) for ts in (0, 1)]
TIME_CASES += [(M, S, 0, 1) for S in (7, 12, 32) for M in (256 * (32 // S) * S, 256 * (32 // S) * S + 1)]
PART_CASES = [(64 * S, S, nk, ns, ws, defer, slices) for S in (1, 7, 12, 32, 33) for nk in (63, 64) for ns in (0, 1, 4, 5) for ws in (0, 1)
              for defer in (0, 1) for slices in (1, 4)] + [(64 * 12 + 12, 12, 64, 4, 1, 0, 4), (32 * 12, 12, 64, 4, 1, 0, 4)]
FRAME_NTOK = (1, 32, 33, 64, 96, 160, 192, 341, 342, 448, 512, 513, 672, 673, 704, 740, 2000)
FRAME_CASES = [(nt * S, S, ws, defer, slices, fs) for S in (7, 8, 12, 32) for nt in FRAME_NTOK for ws in (0, 1) for defer in (0, 1)
               for slices in (1, 4) for fs in (0, 1)]
CTX_CASES = [(nt * S, S, nk, ws, defer, ch, nn) for S in (8, 12, 32) for nt in (64, 127, 128, 341, 342, 512, 673, 704, 740) for nk in (63, 64)
             for ws in (0, 1) for defer in (0, 1) for ch in (0, 1, 4, 5) for nn in (0, 288, 864)]
INPUT_M = BLOCK_M + (65, 4097)
PARTFLOATS = [(G, S, 6) for G in (1, 2, 4) for S in (7, 12, 32)]


def probe_input():
    """[(tag, line)] in the order the probe answers."""
    out = [("block", f"block {M} {H} {ws} {sl} {sw(nmb, ns)}") for M, ws, nmb, ns, sl in BLOCK_CASES]
    out += [("lnproj", f"lnproj {M} {sl}") for M, sl in LN_CASES]
    out += [("slices", "slices {} {} {} {}".format(len(ns), *(ns + (0, 0, 0))[:3])) for ns in NEXTS]
    out += [("time", f"time {M} {S} {ws} {sw(time_small=ts)}") for M, S, ws, ts in TIME_CASES]
    out += [("partials", f"partials {M} {S} {H} {nk} {ns} {ws} {df} {sl}") for M, S, nk, ns, ws, df, sl in PART_CASES]
    out += [("frame", f"frame {M} {S} {H} {ws} {df} {sl} {sw(frame_small=fs)}") for M, S, ws, df, sl, fs in FRAME_CASES]
    out += [("ctx", f"ctx {M} {S} {nk} {ws} {df} {ch} {nn}") for M, S, nk, ws, df, ch, nn in CTX_CASES]
    out += [("input", f"input {M}") for M in INPUT_M]
    out += [("attn", f"attn {g} {AF.H} {nq} {nk} {ws}") for g, nq, nk, ws in ATTN_CASES]
    out += [("partfloats", f"partfloats {G} {S} {h}") for G, S, h in PARTFLOATS]
    out += [("upd", f"upd {UPD_N[0]} {UPD_N[-1]} {S} {G} {mask} {sw(time_small=ts, frame_small=fs)}") for S, G, mask, ts, fs in UPD_CASES]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{tag: [answer lines]} of ONE run of the probe over every case of this module."""
    cases = probe_input()
    lines = run_probe(tmp_path_factory, "launch_plan_probe.cpp", [line for _, line in cases])
    out, at = {}, 0
    for tag, _ in cases:
        k = len(UPD_N) if tag == "upd" else 1
        out.setdefault(tag, []).extend(lines[at:at + k])
        at += k
    assert at == len(lines)
    return out


def parse_plan(line):
    """`ws=0 bmv=24 <1,0,1>(29,1,1)` -> (uses_ws, bmv, [((NMB, MODE, ATT), (gx, gy, gz)), ...]); `refused` -> None."""
    if line == "refused":
        return None
    f = line.split()
    launches = []
    for tok in f[2:]:
        t, g = tok[1:-1].split(">(")
        launches.append((tuple(map(int, t.split(","))), tuple(map(int, g.split(",")))))
    return int(f[0][3:]), int(f[1][4:]), launches


def plan(launches, ws=0, bmv=0):
    return ws, bmv, launches


# ------------------------------------------------------------------ the launch table, written out


def table_block(M, ws, nmb, nosplit, slices):
    if (nmb if nmb != "rule" else (2 if M >= 4096 else 1)) == 2:
        return plan([((2, 0, 0), (cdiv(M, 64), 1, 1))])
    if ws and not nosplit and M <= 2048 and M % 32 == 0:
        return plan([((1, 1, 0), (cdiv(M, 32), H // 256, 1)), ((1, 2, 0), (cdiv(M, 32), slices, 1))], ws=1)
    return plan([((1, 0, 0), (cdiv(M, 32), 1, 1))])


def table_ln_proj(M, slices):
    return plan([((2, 3, 0), (cdiv(M, 64), 1, 1))] if M >= 4096 else [((1, 2, 0), (cdiv(M, 32), slices, 1))])


def table_time(M, S, ws, time_small):
    if S > 32 or ws:
        return None
    if time_small and cdiv(M, (32 // S) * S) <= 256:
        bmv = (32 // S) * S
        return plan([((1, 0, 1), (cdiv(M, bmv), 1, 1))], bmv=bmv)
    bmv = (64 // S) * S
    return plan([((2, 0, 1), (cdiv(M, bmv), 1, 1))], bmv=bmv)


def table_partials(M, S, nk, nsplits, ws, defer, slices):
    if not (1 <= nsplits <= 4 and nk == 64 and M == 64 * S and ws and M <= 2048):
        return None
    return plan([((1, 1, 3), (2, H // 256, S))] + ([] if defer else [((1, 2, 5), (2, slices, S))]), ws=1)


def table_frame(M, S, ws, defer, slices, frame_small):
    ntok = M // S
    if frame_small and ntok * S >= 4096 and cdiv(ntok, 32) * S <= 256:
        return None if ws else plan([((1, 0, 2), (cdiv(ntok, 32), 1, S))])
    if ntok * S >= 4096:
        return None if ws else plan([((2, 0, 2), (cdiv(ntok, 64), 1, S))])
    if not (ws and M <= 2048 and ntok % 32 == 0):
        return None
    return plan([((1, 1, 2), (ntok // 32, H // 256, S))] + ([] if defer else [((1, 2, 5), (ntok // 32, slices, S))]), ws=1)


def table_ctx(M, S, nk, ws, defer, chunks, next_n):
    ntok = M // S
    tiles = cdiv(ntok, 64)
    if not (nk == 64 and ntok * S >= 4096 and not ws and not defer and 1 <= chunks <= 4):
        return None
    if next_n and cdiv(next_n, 32) > 8 * tiles:
        return None
    return plan([((2, 0, 6), (tiles, 1, S))])


# ------------------------------------------------------------------ the tests


def test_block_plans(answers):
    assert len(answers["block"]) == len(BLOCK_CASES)
    seen = set()
    for (M, ws, nmb, nosplit, slices), line in zip(BLOCK_CASES, answers["block"]):
        got = parse_plan(line)
        assert got == table_block(M, ws, nmb, nosplit, slices), (M, ws, nmb, nosplit, slices, line)
        assert [("block", t[0], t[1]) for t, _ in got[2]] == MM.block_forms(M, ws, nmb=nmb, nosplit=bool(nosplit)), (M, ws, nmb, nosplit)
        assert all(t[2] == 0 for t, _ in got[2])
        seen |= {t for t, _ in got[2]}
    assert seen == {(2, 0, 0), (1, 1, 0), (1, 2, 0), (1, 0, 0)}


def test_ln_proj_plans(answers):
    for (M, slices), line in zip(LN_CASES, answers["lnproj"]):
        got = parse_plan(line)
        assert got == table_ln_proj(M, slices), (M, slices, line)
        assert ("ln_proj",) + got[2][0][0][:2] == MM.ln_proj_form(M) and len(got[2]) == 1
    for M, line in zip(INPUT_M, answers["input"]):
        assert parse_plan(line) == plan([((2, 3, 4), (cdiv(M, 64), 1, 1))]), (M, line)


def test_pass2_slices(answers):
    for ns, line in zip(NEXTS, answers["slices"]):
        assert int(line) == (cdiv(max(cdiv(n, 32) for n in ns), 8) if ns else 1), (ns, line)


def test_attention_block_plans(answers):
    """The time, partials, per-frame and context forms against the table, refusals included; every form and every refusal is met."""
    seen, refused = set(), set()
    for name, cases, table in (("time", TIME_CASES, table_time), ("partials", PART_CASES, table_partials), ("frame", FRAME_CASES, table_frame),
                               ("ctx", CTX_CASES, table_ctx)):
        assert len(answers[name]) == len(cases)
        for c, line in zip(cases, answers[name]):
            got = parse_plan(line)
            assert got == table(*c), (name, c, line)
            if got is None:
                refused.add(name)
            else:
                seen |= {(t, len(got[2])) for t, _ in got[2]}
    assert refused == {"time", "partials", "frame", "ctx"}
    assert {t for t, _ in seen} == {(1, 0, 1), (2, 0, 1), (1, 1, 3), (1, 2, 5), (1, 0, 2), (2, 0, 2), (1, 1, 2), (2, 0, 6)}
    assert ((1, 1, 3), 1) in seen and ((1, 1, 3), 2) in seen and ((1, 1, 2), 1) in seen and ((1, 1, 2), 2) in seen  # deferred pass 2 and not


def test_attention_forms(answers):
    names = {"keysplit": "split", "ks4": "ks4", "ks1": "ks1"}
    seen = set()
    for (g, nq, nk, ws), line in zip(ATTN_CASES, answers["attn"]):
        kernel, blocks = line.split()
        assert names[kernel] == AF.form_of(g, nq, nk, ws), (g, nq, nk, ws, line)
        nchunk = g * AF.H * cdiv(nq, 64)
        assert int(blocks) == (cdiv(nchunk, 4) if kernel == "ks1" else nchunk), (g, nq, nk, ws, line)
        seen.add(kernel)
    assert seen == set(names)
    for (G, S, h), line in zip(PARTFLOATS, answers["partfloats"]):
        assert int(line) == G * 4 * S * h * 64 * 68


def test_updater_forms(answers):
    """updater_forms against UW.forms: every n from 1 to 800 at every (S, mask, G, switch values) of the sweep."""
    # the restatement's labels -> the probe's line (form names, then the first template of the time and of the point<-virtual block)
    t_of = {"sep": ("separate", 0), "tile32": ("fused", 101), "tile64": ("fused", 201)}
    p_of = {"sep": ("separate", 0), "frame32": ("frame", 102), "frame64": ("frame", 202), "ctx": ("ctx", 206), "ctx_ragged": ("ctx", 206),
            "segmented": ("segmented", 0)}
    vs_of = {"sep": "separate", "frame_split": "frame", "deferred": "deferred", "segmented": "segmented"}
    lines = answers["upd"]
    assert len(lines) == len(UPD_CASES) * len(UPD_N)
    memo, seen, at = {}, set(), 0
    for S, G, mask, ts, fs in UPD_CASES:
        for n in UPD_N:
            f = UW.forms(n, S, mask, G, time_small=bool(ts), frame_small=bool(fs))
            k = (f["time"], f["v2p"], f["vself"], f["p2v"])
            want = memo.get(k)
            if want is None:
                seen.add(k)
                assert f["p2v"] != "ctx_ragged" or n % 64
                want = memo[k] = f"{t_of[k[0]][0]} {k[1]} {vs_of[k[2]]} {p_of[k[3]][0]} {t_of[k[0]][1]} {p_of[k[3]][1]}"
            assert lines[at] == want, (n, S, G, mask, ts, fs, lines[at], want)
            at += 1
    assert {k[0] for k in seen} == set(t_of) and {k[3] for k in seen} == set(p_of)
    assert {k[1] for k in seen} == {"plain", "partials", "segmented"} and {k[2] for k in seen} == set(vs_of)
