"""The exact suites once more under every tuning switch that a process reads only once.

The library reads a handful of tuning variables as `static const ... = getenv("MVT_...")`, once per process: on the first call of
the entry that holds the line, or -- the four of the block kernels, which block_fused.hip keeps together in block_switches() -- on
the first call of any block entry or of the composite updater, and MVT_ROWS_NW8 / MVT_FOLD_DOWNSAMPLE, which conv_rows.hip keeps in
conv_switches(), on the first bf16 convolution, slot query or composite encoder call.  `monkeypatch.setenv` inside the pytest process cannot reach them, and the code behind them -- row tiles of 16 and of 4 output rows,
1 / 2 / 4 / 8 kNN queries per wave on either side of the default, the 64-row block tiles on a few rows and the 32-row ones on many,
the folded context form at a few hundred tracks, the generic bf16 apply / concat kernels, the unfolded strided blocks of the
composite encoder -- is what the next change of a threshold or a default puts under production shapes.  The exact suites give
answers that do not depend on the variant (integers, planted decodes), so each row of SWITCHES runs a selection of them in a fresh
child process with the row's variables set (rows on disjoint source files share a child, see SWITCHES).

A row passes only if the child exits with 0, its summary line reports exactly the expected number of passed tests, and nothing was
skipped, deselected, failed or errored.  Children run one at a time; the parent tests of this module do not touch the GPU.  After a
child that ended by signal, by abort (134 / -6), by segmentation fault (139 / -11), at its time limit, or whose output reports a
GPU memory fault, FAULTED makes every later row fail at once without starting another child.

What a row proves.  Where the switch shows through the ABI the child asserts it (the `test_child_*` tests below; each is guarded
by a skipif on its variable, only its row selects it, and the zero-skipped rule makes sure it ran):
  * MVT_ROWS_NW8: mvt_conv2d_stat_slots counts tiles of 16 rows (=1, Ho % 16 == 0) and of 4 rows (=2), and every selected
    statistics test compares the library's slot count with the restatement, which follows the switch;
  * MVT_KNN_Q=3: the entries refuse, and write nothing.
For the other switches no ABI call tells which kernel ran: MVT_BLOCK_NMB, MVT_BLOCK_NOSPLIT, MVT_TIME_NMB1, MVT_FRAME_NMB1,
MVT_APPLY_GENERIC, MVT_CONCAT_GENERIC, MVT_FOLD_DOWNSAMPLE, and MVT_KNN_Q at a compiled value.  (For MVT_FRAME_NMB1=0 the child
asserts that a per-frame block call of fewer than 4096 rows without a workspace is refused; that is the rule of the split path
and holds under the default too, where the small-tile form also starts at 4096 rows, so it pins the refusal, not the switch.)
Their guarantee is `test_switched_cases_reach_the_switched_variant`: the dispatch restatements of the five exact files take the
switch values as arguments, every row's selected cases reach the (variant, size class) the row claims under the row's values, and no
default-environment case of the same file does.  `test_table_names_every_once_per_process_switch` ties the table to the source:
a `static ... getenv("MVT_...")` without a row fails it.

Timeouts are safety stops for a loaded machine (about four times the measured time of the child, DESIGN.md "Tuning switches under
test"), not performance bars.
"""
import collections
import glob
import os
import re
import subprocess
import sys

import pytest
import torch

import test_gpu_corr_exact as KC
import test_gpu_encoder_norm_exact as EN
import test_gpu_encoder_wiring as EW
import test_gpu_matmul_exact as MM
import test_gpu_updater_wiring_exact as UW

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAN = float("nan")
THIS = "tests/test_gpu_tuning_switches.py"


def cdiv(a, b):
    return (a + b - 1) // b


def nodes(path, test, params=None):
    return [f"tests/{path}::{test}"] if params is None else [f"tests/{path}::{test}[{p}]" for p in params]


# ================================================================== the selections

# ---- MVT_ROWS_NW8: the 3x3 / stride-1 row tiles
# matmul file: every bf16 3x3 / stride-1 case that stays on the row tiles (no big tile); each runs Ho = 9, 8, 7, 16, 17: Ho % 16 == 0,
# Ho % 16 != 0 (falls back to 8 rows at =1) and Ho % 4 != 0
MM_ROWS = [c for c in MM.CONV_CASES if c.prec == "bf16" and c.k == 3 and c.s == 1
           and all(MM.conv_variant(c, *g, nw8=0)[0] == "rows" for g in MM.conv_geos(c))]
# encoder-norm file: every bf16 3x3 / stride-1 case -- the row-tile ones and the 256-channel ones, which take statistics and
# therefore leave the big tile where the switch changes the slot layout (Ho = 5, 8, 9, 13)
EN_ROWS = [c for c in EN.CONV_CASES if c.prec == "bf16" and c.k == 3 and c.s == 1]
EN_NORM = [c for c in EN_ROWS if c.norm]
# ... and what those sizes cannot give: Ho % 16 == 0 with statistics (test_child_sixteen_row_tile_statistics), one and two tiles
SIXTEEN_GEOS = [(16, 40), (32, 33)]
SIXTEEN_CASES = [EN.Conv("bf16", "bb", 64, 64, 3, 1), EN.Conv("bf16", "ff", 32, 64, 3, 1, ldo_extra=2), EN.Conv("bf16", "fb", 32, 96, 3, 1),
                 EN.Conv("bf16", "bb", 64, 64, 3, 1, norm=True), EN.Conv("bf16", "bb", 32, 256, 3, 1)]
# composite encoder: latent_dim 32 (conv2 on 64-channel row tiles) and short workgroups (conv2's 256 channels on row tiles: the
# widest partials), each ragged (H/2 = 18) and whole (H/2 = 16: the 16-row tile at =1)
EW_CASES = [c for c in EW.CASES if c.C == 32 or c.swg == 1]
EW_SEQ = ["3-36-68-128", "3-36-68-32", "2-16-16-160", "3-36-68-160"]

ROWS_NODES = (nodes("test_gpu_matmul_exact.py", "test_conv_exact", map(MM.conv_id, MM_ROWS))
              + nodes("test_gpu_encoder_norm_exact.py", "test_conv_statistics_exact", map(EN.conv_id, EN_ROWS))
              + nodes("test_gpu_encoder_norm_exact.py", "test_normalise_on_load_equals_two_steps", map(EN.conv_id, EN_NORM))
              + nodes("test_gpu_encoder_wiring.py", "test_segments", map(EW.case_id, EW_CASES))
              + nodes("test_gpu_encoder_wiring.py", "test_workspace_contents_do_not_matter", [128, 32])
              + nodes("test_gpu_encoder_wiring.py", "test_equals_python_sequence", EW_SEQ)
              + nodes(os.path.basename(THIS), "test_child_stat_slots_follow_rows_nw8"))

# ---- MVT_KNN_Q: all of section B of the corr file.  Its N in (1, 3, 9) give N < Q, N % Q == 1 and a ragged last query group for
# Q = 2, 4, 8 (test_knn_cases_straddle_every_query_group)
KNN_NODES = (nodes("test_gpu_corr_exact.py", "test_knn_shapes", KC.KNN_P)
             + nodes("test_gpu_corr_exact.py", "test_knn_orders", [f"{k}-{m}" for k in KC.ORDERS for m in KC.MODES])
             + nodes("test_gpu_corr_exact.py", "test_knn_seeds", [f"{k}-16" for k in KC.SEEDS] + ["true-5"])
             + nodes("test_gpu_corr_exact.py", "test_knn_fewer_than_k_finite"))


def knn_selected_cases():
    return KC.all_knn_cases()  # (the four selected tests are exactly the cases of all_knn_cases)


# ---- MVT_BLOCK_NMB / MVT_BLOCK_NOSPLIT: the three block stages over BLOCK_MS
_BM = [f"{M}-{ws}" for M, ws in MM.BLOCK_MS]
BLOCK_NODES = (nodes("test_gpu_matmul_exact.py", "test_block_attention_projection_exact", [f"{b}-{a}" for a in ("att-fp32", "att-bf16") for b in _BM])
               + nodes("test_gpu_matmul_exact.py", "test_block_mlp_exact", [f"{b}-{H}" for H in (256, 1024) for b in _BM])
               + nodes("test_gpu_matmul_exact.py", "test_block_followup_projections_exact", [f"{b}-{r}" for r in ("all-rows", "row-ranges") for b in _BM]))

# ---- MVT_TIME_NMB1=0: the time chains at a handful of tracks and at the first size of the frame forms; other window lengths
TIME_N, TIME_S = (5, 37, 342), (7, 16, 32)
TIME_NODES = (nodes("test_gpu_updater_wiring_exact.py", "test_composite_decodes", [f"{c}-{n}" for c in UW.TIME for n in TIME_N])
              + nodes("test_gpu_updater_wiring_exact.py", "test_other_window_lengths_decode", [f"{c}-{S}-21" for c in UW.TIME for S in TIME_S]))

# ---- MVT_FRAME_NMB1=0: the space chains and the two MLP stages whose block changes form, each below / at / inside / at the end of
# the range [342, 672] that takes the small-tile form by default (the updater file runs the MLPs at 341, 448, 512 and 672 for this row)
FRAME_N = (37, 341, 342, 448, 512, 672)
FRAME_MLPS = UW.MLPS_FRAME
FRAME_CASES = [(c, n) for c in UW.SPACE + FRAME_MLPS for n in FRAME_N]
FRAME_HEAD = [(342, 55), (512, 55)]
FRAME_NODES = (nodes("test_gpu_updater_wiring_exact.py", "test_composite_decodes", [f"{c}-{n}" for c, n in FRAME_CASES])
               + nodes("test_gpu_updater_wiring_exact.py", "test_update_head_through_composite", [f"{n}-{m}" for n, m in FRAME_HEAD])
               + nodes("test_gpu_updater_wiring_exact.py", "test_grouped_decodes", ["v2p_vself_p2v@0-group_n0", "v2p_vself_p2v@0-group_n1"])
               + nodes(os.path.basename(THIS), "test_child_frame_block_without_workspace_is_refused"))

# ---- MVT_APPLY_GENERIC / MVT_CONCAT_GENERIC
APPLY_NODES = nodes("test_gpu_encoder_norm_exact.py", "test_instnorm_apply_exact",
                    [f"{p}-{f}" for p in ("fp32", "bf16-16B", "bf16-generic") for f in EN.APPLY_FORMS])
CONCAT_BF16 = [i for i, (ios, _, _) in enumerate(EN.CONCAT) if "b" in ios]
CONCAT_NODES = (nodes("test_gpu_encoder_norm_exact.py", "test_concat_resize_exact", CONCAT_BF16)
                + nodes("test_gpu_ops.py", "test_concat_resize_matches_separate_resizes", ["dt1"]))

# ---- MVT_FOLD_DOWNSAMPLE=0: the composite with its strided blocks unfolded (the Python sequence reads the same variable when the
# model is built, so the comparison stays like against like); and the smallest shape of the end-to-end bit identity
FOLD_NODES = (nodes("test_gpu_encoder_wiring.py", "test_segments", map(EW.case_id, EW_CASES))
              + nodes("test_gpu_encoder_wiring.py", "test_equals_python_sequence", EW_SEQ)
              + nodes("test_gpu_e2e.py", "test_composite_encoder_bit_identical", ["shape0"]))

# ================================================================== the table

Row = collections.namedtuple("Row", "name env reaches nodes expect child timeout marker", defaults=(None, "gpu"))

# One row per (variable, value).  `child`: the rows with the same letter share one child process (CHILDREN below).  One child per
# row measured 89 s on the MI355X -- about 4 s of interpreter start, imports and code-object load per child, 60 s in all -- against
# 43 s for the five exact files themselves, so rows whose variables are read in disjoint source files are merged (DESIGN.md "Tuning
# switches under test" has both sets of times).  No variable of the block kernels (all read in block_fused.hip) shares a child
# with another, nor do the two of encoder.hip: five children, as many as MVT_KNN_Q has values.
# Disjoint source files are not disjoint code paths: the composite-encoder nodes of fold-downsample-0 call mvt_instnorm_apply and so
# also run under MVT_APPLY_GENERIC=1 (child c).  The updater nodes of time-nmb1-0 / frame-nmb1-0 run with the MVT_KNN_Q of their child
# set (d: 8, e: 3), which they never read: the composite updater calls no kNN entry (its correlation features are passed in).
# Both sides of every comparison see the same environment, so the results stand; but a failure in a merged child names the child,
# not the switch: run the failing node again with one variable at a time.
SWITCHES = [
    Row("rows-nw8-1", {"MVT_ROWS_NW8": "1"},
        "conv_rows_bf16<2, TN, 3, 1, INB, 8>: 16-row tiles of eight waves where Ho % 16 == 0 (8 rows elsewhere), plain and staged "
        "epilogue, their statistics slots, inside the composite encoder at H/2 = 16",
        ROWS_NODES + nodes(os.path.basename(THIS), "test_child_sixteen_row_tile_statistics", map(EN.conv_id, SIXTEEN_CASES)), 59, "a"),
    Row("rows-nw8-2", {"MVT_ROWS_NW8": "2"},
        "conv_rows_bf16<1, TN, 3, 1, INB, 4>: four-row tiles, plain epilogue only (the staging tiles do not fit), twice the "
        "statistics slots, inside the composite encoder's partials buffer",
        ROWS_NODES, 54, "b"),
    Row("knn-q-1", {"MVT_KNN_Q": "1"}, "knn_scan_kernel / _levels_kernel / search_levels_kernel <1>", KNN_NODES, 30, "a"),
    Row("knn-q-2", {"MVT_KNN_Q": "2"}, "<2> without tile boxes", KNN_NODES, 30, "b"),
    Row("knn-q-4", {"MVT_KNN_Q": "4"}, "<4>", KNN_NODES, 30, "c"),
    Row("knn-q-8", {"MVT_KNN_Q": "8"}, "<8> with tile boxes", KNN_NODES, 30, "d"),
    Row("knn-q-3", {"MVT_KNN_Q": "3"}, "no kernel: every scan entry refuses and writes nothing",
        nodes(os.path.basename(THIS), "test_child_knn_q3_is_refused"), 1, "e"),
    Row("block-nmb-1", {"MVT_BLOCK_NMB": "1"}, "block_fused_bf16<1, 0, 0> at M >= 4096", BLOCK_NODES, 72, "a"),
    Row("block-nmb-2", {"MVT_BLOCK_NMB": "2"},
        "block_fused_bf16<2, 0, 0> at M < 4096: M = 31 (second 32-row block empty), 33 (one row), 63, 65, and with a workspace", BLOCK_NODES, 72, "b"),
    Row("block-nosplit", {"MVT_BLOCK_NOSPLIT": "1"}, "block_fused_bf16<1, 0, 0> at M = 32, 64, 2048 with a workspace", BLOCK_NODES, 72, "c"),
    Row("time-nmb1-0", {"MVT_TIME_NMB1": "0"}, "the 64-row time tile <2, 0, 1> at 5, 37, 342 tracks and at S = 7, 16, 32", TIME_NODES, 24, "d"),
    Row("frame-nmb1-0", {"MVT_FRAME_NMB1": "0"},
        "n in [342, 672]: the 64-token frame tile <2, 0, 2>, the deferred virtual-self pass 1 and the folded context form <2, 0, 6> "
        "(whole tiles at 448 and 512, a ragged last tile at 342 and 672), each with chains and with the planted MLP of the point<-virtual "
        "and of the virtual-self block", FRAME_NODES, 77, "e"),
    Row("apply-generic", {"MVT_APPLY_GENERIC": "1"}, "instnorm_apply_kernel on bf16 tensors of C % 8 == 0", APPLY_NODES, 12, "c"),
    Row("concat-generic", {"MVT_CONCAT_GENERIC": "1"}, "concat_resize_kernel<1> on bf16 tensors", CONCAT_NODES, 6, "d"),
    Row("fold-downsample-0", {"MVT_FOLD_DOWNSAMPLE": "0"},
        "the strided blocks of the composite encoder as two launches (3x3 / stride-2 row tiles + the 1x1 / stride-2 downsample)", FOLD_NODES, 9, "c"),
]
PER_CALL = {"MVT_PROJ_SEQ", "MVT_CONV_BIG", "MVT_ENC_GROUP"}  # read on every call: ordinary tests switch them with monkeypatch

# time limit per child: about four times its measured wall time on the MI355X, rounded up to a multiple of 30 s
CHILD_TIMEOUT = {"a": 60, "b": 60, "c": 60, "d": 60, "e": 60}  # measured 11.6, 11.1, 11.4, 6.1, 8.3 s alone; up to 12.9, 11.6, 13.4, 7.7, 8.2 s in the whole suite


def merged(child):
    """The rows of one child as one row: every variable set, every node selected, the expected counts added."""
    rows = [r for r in SWITCHES if r.child == child]
    env = {k: v for r in rows for k, v in r.env.items()}
    return Row("+".join(r.name for r in rows), env, "; ".join(r.reaches for r in rows), [n for r in rows for n in r.nodes],
               sum(r.expect for r in rows), child, CHILD_TIMEOUT[child])


CHILDREN = [merged(c) for c in sorted(CHILD_TIMEOUT)]


# ================================================================== the runner

FAULTED = []  # the first child that ended by fault, abort or time limit: no child is started after it
FAULT_CODES = (134, 139, 124, 137)
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Segmentation fault", "Aborted")
BAD_OUTCOMES = ("failed", "skipped", "deselected", "error", "errors", "xfailed", "xpassed")


def summary_counts(out):
    """The counts of pytest's last summary line ("3 passed, 1 skipped in 0.12s") -> {"passed": 3, "skipped": 1}; {} if there is none."""
    for line in reversed(out.splitlines()):
        if re.search(r"\bin \d+(\.\d+)?s\b", line):
            return {k: int(v) for v, k in re.findall(r"(\d+) ([a-z]+)", line.split(" in ")[0])}
    return {}


def is_fault(returncode, out):
    return returncode < 0 or returncode in FAULT_CODES or any(t in out for t in FAULT_TEXT)


def judge(row, returncode, out):
    """None if the child's run passes the row, else why not."""
    counts = summary_counts(out)
    if returncode != 0:
        return f"the child exited with {returncode}"
    if counts.get("passed", 0) != row.expect:
        return f"{counts.get('passed', 0)} tests passed, the row expects {row.expect}"
    bad = {k: v for k, v in counts.items() if k in BAD_OUTCOMES}
    return f"not every selected test ran and passed: {bad}" if bad else None


def run_row(row):
    """Runs the row's child; None if the row passes, else the reason (the tail of the child's output is printed)."""
    if FAULTED:
        return f"not started: {FAULTED[0]}"
    flags = (["-I"] if sys.flags.isolated else (["-s"] if sys.flags.no_user_site else []))
    cmd = [sys.executable, *flags, "-m", "pytest", "-q", "-m", row.marker, "-p", "no:cacheprovider", *row.nodes]
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, **row.env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=row.timeout)
        returncode, out = p.returncode, p.stdout
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        FAULTED.append(f"the child of {row.name} was ended at its time limit of {row.timeout} s")
        returncode = None
    if returncode is not None and is_fault(returncode, out):
        FAULTED.append(f"the child of {row.name} ended by fault or abort (exit {returncode})")
    run_row.last = (returncode, out)
    why = FAULTED[0] if FAULTED else judge(row, returncode, out)
    if why:
        print(f"---- {row.name} {row.env}: {why}\n" + "\n".join(out.splitlines()[-60:]))
    return why


@gpu
@pytest.mark.parametrize("row", CHILDREN, ids=lambda r: r.name)
def test_switch(row):
    why = run_row(row)
    assert why is None, f"{row.name} {row.env} ({row.reaches}): {why}"


# ================================================================== in the child: where the switch shows through the ABI

@pytest.fixture(scope="module")
def hip():
    from mvtracker_amd import hip as h
    assert torch.cuda.is_available()
    return h


def only_under(var, *values):
    return pytest.mark.skipif(os.environ.get(var) not in values, reason=f"runs in the child process of {var} = {' / '.join(values)} only")


SLOT_SIZES = [(16, 32), (16, 33), (32, 40), (48, 100), (8, 32), (9, 33), (17, 20), (5, 7)]


def switched_slots(H, W, k, s, nw8):
    """The slots of a row-tile convolution (k, s) of an H x W image under MVT_ROWS_NW8 = 1 or 2: only the 3x3 / stride-1 tile follows
    the switch (test_conv_plan_host.py holds csrc/conv_plan.h to this on the CPU)."""
    ho, wo = EN.conv_out(H, W, k, s)
    rows = (4 if nw8 == 2 else (16 if ho % 16 == 0 else 8)) if (k, s) == (3, 1) else (4 if k == 3 else 8)
    return cdiv(ho, rows) * cdiv(wo, 32)


@gpu
@only_under("MVT_ROWS_NW8", "1", "2")
def test_child_stat_slots_follow_rows_nw8(hip):
    """mvt_conv2d_stat_slots of a 3x3 / stride-1 / Cin % 32 == 0 convolution counts the tiles of the switched variant; the other
    row-tile kernels keep theirs."""
    nw8 = int(os.environ["MVT_ROWS_NW8"])
    for H, W in SLOT_SIZES:
        for Cin in (32, 64, 416):
            got = hip.conv2d_stat_slots(H, W, Cin, 3, 3, 1, 1)
            assert got == switched_slots(H, W, 3, 1, nw8), (H, W, Cin, got)
        assert hip.conv2d_stat_slots(H, W, 32, 3, 3, 2, 1) == switched_slots(H, W, 3, 2, nw8)
        assert hip.conv2d_stat_slots(H, W, 32, 1, 1, 1, 0) == switched_slots(H, W, 1, 1, nw8)
    assert any(H % 16 == 0 for H, _ in SLOT_SIZES) and any(H % 16 and H % 4 == 0 for H, _ in SLOT_SIZES) and any(H % 4 for H, _ in SLOT_SIZES)


@gpu
@only_under("MVT_ROWS_NW8", "1")
@pytest.mark.parametrize("c", SIXTEEN_CASES, ids=EN.conv_id)
def test_child_sixteen_row_tile_statistics(hip, c, monkeypatch):
    """test_conv_statistics_exact at Ho = 16 and 32, where the 16-row tile runs: output, partials summed over the slots, finished
    statistics.  The 256-channel case asks for the big tile, whose 8-row slots do not match: it has to stay on the row tiles."""
    monkeypatch.setenv("MVT_CONV_BIG", "1")
    for (H, W) in SIXTEEN_GEOS:
        assert EN.conv_variant(c, H, 1)[0] == "rows" and EN.tile_rows(c, H, 1) == 16
        d = EN.case_data(c, H, W)
        Y = d["Y"]
        assert float(Y.abs().max()) <= EN.YMAX
        out, part, mr = EN.run_conv(hip, c, H, W, d["x"], d["w"], d["b"], (d["mean"], d["rstd"]) if c.norm else None)
        assert part.shape[1] == cdiv(H, 16) * cdiv(W, 32)
        what = f"{EN.conv_id(c)} {H}x{W} (16-row tiles)"
        EN.assert_equal(out, Y.to(EN.dt(c.io[1])), what + " output")
        EN.check_partials(part, Y, what)
        EN.check_mean_rstd(mr, *EN.exact_sums(Y), H * W, what)


@gpu
@only_under("MVT_KNN_Q", "3")
def test_child_knn_q3_is_refused(hip):
    """No scan kernel is compiled for 3 queries per wave: every scan entry rejects its arguments and leaves its poisoned outputs as
    they were (the calls are the accepted ones of test_linear_frames_refusals)."""
    r = KC.R.rng("refuse")
    P, N, K = 320, 2, 4
    xyz, coords = KC.T_(KC.cloud4(KC.lattice(r, 1, P, 3)), DEV), KC.T_(KC.lattice(r, N, 1, 3), DEV)
    box = torch.zeros(1, 5, 8, device=DEV)
    hip.tile_aabb(xyz, P, 1, box)
    keys = torch.full((N * K + K,), KC.SENT_K, dtype=torch.int64, device=DEV)
    idx = torch.full((N * K + K,), KC.SENT_I, dtype=torch.int32, device=DEV)
    lv = [dict(xyz=xyz, P=P, keys=keys, nseg=1, box=box, idx_out=idx)]
    calls = [lambda: hip.knn_scan(xyz, P, coords, N, 1, 0, 1, 1, K, 1, keys),
             lambda: hip.knn_scan(xyz, P, coords, N, 1, 0, 1, 1, K, 1, keys, box=box),
             lambda: hip.knn_search(xyz, P, coords, N, 1, 0, 1, 1, K, idx, box),
             lambda: hip.knn_scan_levels(lv, coords, N, 1, 0, 1, 1, K),
             lambda: hip.knn_search_levels(lv, coords, N, 1, 0, 1, 1, K, 0)]
    for f in calls:
        with pytest.raises(hip.HipError, match="arguments rejected"):
            f()
    torch.cuda.synchronize()
    assert bool((keys == KC.SENT_K).all()) and bool((idx == KC.SENT_I).all())
    assert KC.knn_queries_per_wave(True) == KC.knn_queries_per_wave(False) == 3 and 3 not in KC.KNN_Q_COMPILED


@gpu
@only_under("MVT_FRAME_NMB1", "0")
def test_child_frame_block_without_workspace_is_refused(hip):
    """mvt_attn_block_fused_bf16, kind MVT_ATTN_FRAME, ntok * S = 64 < 4096 rows and no workspace: refused, nothing written.  (The
    split path of so few rows needs its workspace.  The default environment refuses the same call -- its small-tile form starts
    at 4096 rows as well -- so this pins the refusal under the switch, it does not tell the switch.)"""
    g = MM.gen_for("frame-refusal")
    C, KO, S, ntok, H = MM.C, MM.KO, 2, 32, 256
    M = ntok * S
    x = torch.full((M, C), 3.0, device=DEV)
    q, k, v = (torch.zeros(M, KO, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    W1, b1, W2, b2 = MM.block_weights(g, H)
    wo, bo = MM.frag(hip, MM.ints(g, (C, KO), 1)), MM.ints(g, (C,), 3).to(DEV)
    with pytest.raises(hip.HipError, match="arguments rejected"):
        hip.attn_block_fused_bf16(x, C, hip.ATTN_FRAME, S, q, KO, k, v, KO, ntok, wo, bo, MM.frag(hip, W1), b1.to(DEV), MM.frag(hip, W2), b2.to(DEV),
                                  H, [], M, C, ws=None)
    torch.cuda.synchronize()
    assert bool((x == 3.0).all())


@pytest.mark.skipif("MVT_SWITCH_PROBE" not in os.environ, reason="selected by test_runner_probes only")
def test_child_sees_the_probe_variable():
    assert os.environ["MVT_SWITCH_PROBE"] == "17"


# ================================================================== CPU: the table against the source

def getenv_sites():
    """{variable: [(file, is_static)]} of every getenv("MVT_...") in the library's sources."""
    sites = collections.defaultdict(list)
    for path in sorted(glob.glob(os.path.join(ROOT, "mvtracker_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "mvtracker_amd", "csrc", "*.h"))):
        for line in open(path):
            for name in set(re.findall(r'getenv\("(MVT_\w+)"\)', line)):
                sites[name].append((os.path.basename(path), re.search(r"\bstatic\b", line) is not None))
    return sites


def test_table_names_every_once_per_process_switch():
    sites = getenv_sites()
    once = {n for n, s in sites.items() if any(st for _, st in s)}
    table = {v for r in SWITCHES for v in r.env}
    assert once == table, (sorted(once - table), sorted(table - once))
    assert all(st for n in once for _, st in sites[n]), "a once-per-process switch is also read per call somewhere"
    assert {n for n in sites if n not in once} == PER_CALL
    assert all(not st for n in PER_CALL for _, st in sites[n])
    # one row per (variable, value), the values the source distinguishes
    want = {("MVT_ROWS_NW8", "1"), ("MVT_ROWS_NW8", "2"), ("MVT_BLOCK_NMB", "1"), ("MVT_BLOCK_NMB", "2"), ("MVT_BLOCK_NOSPLIT", "1"),
            ("MVT_TIME_NMB1", "0"), ("MVT_FRAME_NMB1", "0"), ("MVT_APPLY_GENERIC", "1"), ("MVT_CONCAT_GENERIC", "1"), ("MVT_FOLD_DOWNSAMPLE", "0")}
    want |= {("MVT_KNN_Q", str(q)) for q in KC.KNN_Q_COMPILED + (3,)}
    assert sorted(kv for r in SWITCHES for kv in r.env.items()) == sorted(want) and all(len(r.env) == 1 for r in SWITCHES)
    assert len({r.name for r in SWITCHES}) == len(SWITCHES) and all(r.expect == len(r.nodes) for r in SWITCHES)
    # merged rows: different variables, read in disjoint source files, selecting different tests; every row is in one child
    assert {r.child for r in SWITCHES} == set(CHILD_TIMEOUT) and all(t % 30 == 0 for t in CHILD_TIMEOUT.values())
    for ch in CHILDREN:
        rows = [r for r in SWITCHES if r.child == ch.child]
        files = [f for r in rows for f in sorted({f for v in r.env for f, _ in sites[v]})]
        assert len(ch.env) == len(rows) and len(set(files)) == len(files), (ch.name, files)
        assert len(set(ch.nodes)) == len(ch.nodes) == ch.expect, ch.name
    assert sum(ch.expect for ch in CHILDREN) == sum(r.expect for r in SWITCHES)
    # the sources that hold the switches of two rows are disjoint for every pair the table could merge later
    assert {f for f, _ in sites["MVT_FRAME_NMB1"]} == {"block_fused.hip"} and {f for f, _ in sites["MVT_KNN_Q"]} == {"knn_corr.hip"}


@pytest.mark.parametrize("env", [{}, {"MVT_ROWS_NW8": "1"}, {"MVT_ROWS_NW8": "2"}], ids=lambda e: "-".join(e.values()) or "default")
def test_selected_nodes_exist(env):
    """One collection run over all rows: every node id of the table names exactly one test (an id that matches nothing, or a
    parametrisation that was renamed, fails here on the CPU instead of in a GPU child).  Also under MVT_ROWS_NW8, the one switch
    that the restatements read while the exact files are imported."""
    want = sorted({n for r in SWITCHES for n in r.nodes})
    p = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", *want], cwd=ROOT, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    got = sorted(line.strip() for line in p.stdout.splitlines() if "::" in line and line.startswith("tests/"))
    assert p.returncode == 0 and got == want, (p.returncode, sorted(set(want) - set(got)), sorted(set(got) - set(want)), p.stdout[-2000:])


# ================================================================== CPU: the selected cases reach the switched variants

# ---- convolution row tiles.  Variant = the template instantiation (kernel size, stride, TM, NW, TN, bf16 input, staged epilogue);
# size class = Ho a whole number of tiles or not.

def mm_rows_reach(cases, nw8):
    out = set()
    for c in cases:
        for (n, H, W) in MM.conv_geos(c):
            v = MM.conv_variant(c, n, H, W, nw8=nw8)
            if v[0] == "rows":
                Ho = MM.conv_out(H, W, c.k, c.s)[0]
                tm, nw = MM.rows_tile(c.k, c.s, Ho, nw8)
                out.add(("rows", c.k, c.s, tm, nw, v[3], v[4], v[5], Ho % (tm * nw) == 0))
    return out


def en_rows_reach(cases_geos, nw8):
    """(the statistics path: + normalise-on-load)"""
    out = set()
    for c, geos in cases_geos:
        for (H, W) in geos:
            Ho = EN.conv_out(H, W, c.k, c.s)[0]
            v = EN.conv_variant(c, Ho, nw8)
            if v[0] == "rows":
                tm, nw = EN.rows_tile(c.k, c.s, Ho, nw8)
                out.add(("rows+stats", c.k, c.s, tm, nw, v[3], c.io[0] == "b", v[4], c.norm, Ho % (tm * nw) == 0))
    return out


def composite_launches(n, H, W, C, swg, fold=True):
    """The convolutions with statistics that encoder_run launches on its partials buffer: [(Conv, H, W of its input, halves)];
    halves = 2 for the folded strided launch, whose two outputs share the buffer."""
    out = [(EN.Conv("bf16", "fb", 4, 64, 7, 2), H, W, 1)]
    hh, ww, cin = H // 2, W // 2, 64
    for l, cout in enumerate(EW.R.COUTS):
        s = 1 if l == 0 else 2
        first = EN.Conv("bf16", "bb", cin, cout, 3, s, norm=(l == 0), big=not swg)
        if l and fold:
            out.append((first, hh, ww, 2))
        else:
            out.append((first, hh, ww, 1))
            if l:
                out.append((EN.Conv("bf16", "bb", cin, cout, 1, 2, big=not swg), hh, ww, 1))
        hh, ww = EN.conv_out(hh, ww, 3, s)
        out += [(EN.Conv("bf16", "bb", cout, cout, 3, 1, norm=True, big=not swg), hh, ww, 1),
                (EN.Conv("bf16", "bb", cout, cout, 3, 1, big=not swg), hh, ww, 1),
                (EN.Conv("bf16", "bb", cout, cout, 3, 1, norm=True, big=not swg), hh, ww, 1)]
        cin = cout
    out.append((EN.Conv("bf16", "bb", 416, 2 * C, 3, 1, big=not swg), H // 4, W // 4, 1))
    return out


def ew_rows_reach(cases, nw8):
    return en_rows_reach([(c, [(h, w)]) for cs in cases for c, h, w, _ in composite_launches(cs.n, cs.H, cs.W, cs.C, cs.swg)
                          if c.k == 3 and c.s == 1], nw8)


def test_composite_partials_fit_under_every_row_tile():
    """The partials buffer of the composite encoder is sized as (8 x 32 tiles of the H/2 map) x max(256, 2C) channels.  With
    MVT_ROWS_NW8=2 layer 1 has twice those slots; every launch still fits (the library checks the same and refuses otherwise)."""
    shapes = EW.SHAPES + [(1, 16, 16, 128), (2, 16, 16, 160), (3, 36, 68, 160), (3, 40, 72, 128), (3, 64, 96, 128), (2, 180, 320, 128), (1, 20, 1024, 32)]
    for (n, H, W, C) in shapes:
        floats = EW.plan(n, H, W, C)["part"][1] // 4
        for nw8 in (0, 1, 2):
            for swg in (0, 1):
                for fold in (True, False):
                    for c, h, w, halves in composite_launches(n, H, W, C, swg, fold):
                        assert halves * n * EN.stat_slots(c, h, w, nw8) * c.Cout * 2 <= floats, (n, H, W, C, nw8, swg, c)
    c = EN.Conv("bf16", "bb", 64, 64, 3, 1, norm=True)
    assert EN.stat_slots(c, 18, 34, 2) == 10 > EN.stat_slots(c, 18, 34, 0) == 6  # (more slots than the 8 x 32 tiles of the H/2 map)


# ---- the block kernel.  Size class = (M >= 4096, the split path's condition, what the second 32-row block of the last 64-row tile holds)

def block_reach(nmb, nosplit):
    out = set()
    for M, ws in MM.BLOCK_MS:
        f = tuple(MM.block_forms(M, ws, nmb=nmb, nosplit=nosplit))
        second = None if f != (("block", 2, 0),) else ("whole" if M % 64 == 0 else ("empty" if M % 64 <= 32 else "ragged"))
        out.add((f, M >= 4096, bool(ws) and M <= 2048 and M % 32 == 0, second))
    return out


# ---- kNN: (kernel, queries per wave, with tile boxes)

def knn_reach(q_env):
    return set().union(*(KC.knn_kernels(c, q_env) for c in knn_selected_cases()))


# ---- the updater's forms.  Size class = whether the small-tile form would fit (it is what the default takes then)

def updater_default_cases():
    """(n, S, G) of every composite call of the updater file's GPU tests."""
    out = {(n, 12, 1) for n in UW.N_S12 + UW.N_MLP + UW.N_MLP_FRAME} | {(n, 8, 1) for n in (511, 512)} | {(21, S, 1) for S in (7, 16, 32)}
    out |= {(sum(g), 12, len(g)) for g in UW.GROUPS} | {(n, 12, 1) for n in (341, 342, 384, 37, 740, 449)}
    return sorted(out)


def updater_reach(cases, time_small, frame_small):
    out = set()
    for (n, S, G) in cases:
        M = n * S + G * UW.NV * S
        fits_t, fits_f = cdiv(M, (32 // S) * S) <= 256, n * S >= 4096 and cdiv(n, 32) * S <= 256
        for mask in UW.MASKS:
            f = UW.forms(n, S, mask, G, time_small=time_small, frame_small=frame_small)
            out |= {("time", f["time"], fits_t), ("vself", f["vself"], fits_f), ("p2v", f["p2v"], fits_f)}
    return out


# ---- apply / concat / the strided blocks

def apply_reach(generic):
    return {EN.apply_kernel(io, C, generic) + (C % 8 == 0,) for io, Cs in EN.APPLY_PATHS for C in Cs}


def concat_reach(indices, generic):
    return {EN.concat_kernel(io, sum(d[2] for d in EN.CONCAT[i][1]), generic) for i in indices for io in EN.CONCAT[i][0]}


def strided_launches(cases, fold):
    """(kernel size, Cout, outputs that share the partials buffer) of the stride-2 launches of the composite's strided blocks, from
    the launch list above: one folded launch with two outputs, or the 3x3 and the 1x1 convolution on their own."""
    return {("strided", c.k, c.Cout, halves) for cs in cases for c, _, _, halves in composite_launches(cs.n, cs.H, cs.W, cs.C, cs.swg, fold)
            if c.s == 2 and c.k != 7}


def test_switched_cases_reach_the_switched_variant():
    """For every row: its selected cases reach the claimed (variant, size class) under its values, and NO default-environment case
    of the same file does.  (MVT_FOLD_DOWNSAMPLE has no dispatch rule beside the switch itself, so its claim is derived from the
    composite's launch list with and without the fold; only the source scan ties that row to the library.)"""
    claims = {}

    # MVT_ROWS_NW8
    sel = {nw8: (mm_rows_reach(MM_ROWS, nw8)
                 | en_rows_reach([(c, EN.conv_geos(c)) for c in EN_ROWS] + ([(c, SIXTEEN_GEOS) for c in SIXTEEN_CASES] if nw8 == 1 else []), nw8)
                 | ew_rows_reach(EW_CASES, nw8)) for nw8 in (1, 2)}
    default = (mm_rows_reach(MM.CONV_CASES, 0) | en_rows_reach([(c, EN.conv_geos(c)) for c in EN.CONV_CASES if c.prec == "bf16" and c.Cin != 4], 0)
               | ew_rows_reach(EW.CASES, 0))
    tile = lambda v: v[3:5]
    c1 = {v for v in sel[1] if v[1:3] == (3, 1) and tile(v) == (2, 8)}
    c2 = {v for v in sel[2] if v[1:3] == (3, 1) and tile(v) == (1, 4)}
    claims["rows-nw8-1"], claims["rows-nw8-2"] = (c1, default), (c2, default)
    for kind in ("rows", "rows+stats"):
        k1, k2 = {v for v in c1 if v[0] == kind}, {v for v in c2 if v[0] == kind}
        assert {v[5] for v in k1} == {v[5] for v in k2} == {2, 3}                           # TN
        assert {v[6] for v in k1} == {v[6] for v in k2} == {False, True}                    # bf16 input
        assert {v[7] for v in k1} == {False, True} and {v[7] for v in k2} == {False}         # staged epilogue: never at four rows
        assert {v[-1] for v in k2} == {False, True} and {v[-1] for v in k1} == {True}        # Ho % 4 != 0; a 16-row tile only at Ho % 16 == 0
        assert any(v[0] == kind and v[1:3] == (3, 1) and tile(v) == (2, 4) for v in sel[1])  # =1 falls back to 8 rows where Ho % 16 != 0
        assert not any(v[0] == kind and v[1:3] == (3, 1) and tile(v) == (2, 4) for v in sel[2])
    assert {v[8] for v in c1 if v[0] == "rows+stats"} == {v[8] for v in c2 if v[0] == "rows+stats"} == {False, True}  # normalise-on-load
    # the 256-channel statistics cases leave the big tile exactly where the slot layouts differ
    big = EN.Conv("bf16", "bb", 32, 256, 3, 1)
    assert EN.conv_variant(big, 8, 0) == EN.conv_variant(big, 8, 1) == ("big",) and EN.conv_variant(big, 16, 0) == ("big",)
    assert EN.conv_variant(big, 16, 1)[0] == EN.conv_variant(big, 8, 2)[0] == "rows"
    assert EN.stat_slots(big, 16, 40, 1) == 2 and EN.stat_slots(big, 16, 40, 0) == 4 and EN.stat_slots(big, 13, 45, 2) == 8

    # MVT_KNN_Q
    kd = knn_reach(0)
    assert {v[1:] for v in kd} == {(2, True), (8, False)}
    for q in KC.KNN_Q_COMPILED:
        reach = knn_reach(q)
        assert {v[1] for v in reach} == {q} and {v[2] for v in reach} == {False, True} and {v[0] for v in reach} == {v[0] for v in kd}
        claims[f"knn-q-{q}"] = ({v for v in reach if v not in kd}, kd)
    assert {v[2] for v in claims["knn-q-2"][0]} == {False} and {v[2] for v in claims["knn-q-8"][0]} == {True}
    assert all(len(claims[f"knn-q-{q}"][0]) == 5 for q in (1, 4))  # two scan kernels with and without boxes, the levels search with
    claims["knn-q-3"] = ({("refused", KC.knn_queries_per_wave(b, 3)) for b in (False, True)}, {("refused", q) for q in KC.KNN_Q_COMPILED})

    # MVT_BLOCK_NMB / MVT_BLOCK_NOSPLIT
    bd = block_reach("rule", False)
    one, two, split = (("block", 1, 0),), (("block", 2, 0),), (("block", 1, 1), ("block", 1, 2))
    assert {v[0] for v in bd} == {one, two, split}
    claims["block-nmb-1"] = ({v for v in block_reach(1, False) if v[0] == one and v[1]}, bd)
    claims["block-nmb-2"] = ({v for v in block_reach(2, False) if v[0] == two and not v[1]}, bd)
    claims["block-nosplit"] = ({v for v in block_reach("rule", True) if v[0] == one and v[2]}, bd)
    assert {v[3] for v in claims["block-nmb-2"][0]} == {"whole", "empty", "ragged"} and {v[2] for v in claims["block-nmb-2"][0]} == {False, True}
    assert (two, False, False, "empty") in block_reach(2, False) and MM.block_forms(31, False, nmb=2) == MM.block_forms(33, True, nmb=2) == list(two)
    assert split in {v[0] for v in block_reach(1, False)} and split not in {v[0] for v in block_reach("rule", True)}

    # MVT_TIME_NMB1 / MVT_FRAME_NMB1
    ud = updater_reach(updater_default_cases(), True, True)
    t_sel = updater_reach([(n, 12, 1) for n in TIME_N] + [(21, S, 1) for S in TIME_S], False, True)
    claims["time-nmb1-0"] = ({("time", "tile64", True)} & t_sel, ud)
    assert not any(v[:2] == ("time", "tile32") for v in t_sel)
    f_sel = updater_reach([(n, 12, 1) for n in FRAME_N], True, False)
    want = {("p2v", "frame64", True), ("p2v", "ctx", True), ("p2v", "ctx_ragged", True), ("vself", "deferred", True)}
    claims["frame-nmb1-0"] = (want & f_sel, ud)
    assert want <= f_sel and not any(v[:2] == ("p2v", "frame32") for v in f_sel)
    assert UW.forms(341, 12, 55, frame_small=False)["p2v"] == "sep" and UW.forms(342, 12, 55, frame_small=False)["p2v"] == "ctx_ragged"
    assert [UW.forms(n, 12, 55, frame_small=False)["p2v"] for n in (448, 512, 672)] == ["ctx", "ctx", "ctx_ragged"]
    assert UW.forms(672, 12, 55)["p2v"] == "frame32" and UW.forms(673, 12, 55)["p2v"] == UW.forms(673, 12, 55, frame_small=False)["p2v"]
    # every space chain and every MLP configuration of the two switched blocks runs at every n of the row, so each of them meets
    # the ragged and the whole context tile and the deferred virtual-self pass, and the unswitched forms on either side
    assert sorted(FRAME_MLPS) == sorted(f"mlp_{b}@{L}" for b in ("p2v", "vself") for L in (0, 1))
    for c in UW.SPACE + FRAME_MLPS:
        ns = sorted(n for cc, n in FRAME_CASES if cc == c)
        assert ns == sorted(FRAME_N) and all(f"tests/test_gpu_updater_wiring_exact.py::test_composite_decodes[{c}-{n}]" in FRAME_NODES for n in ns), c
        at = {n: UW.forms(n, 12, 55, frame_small=False) for n in ns}
        assert [at[n]["p2v"] for n in ns] == ["sep", "sep", "ctx_ragged", "ctx", "ctx", "ctx_ragged"], c
        assert [at[n]["vself"] for n in ns] == ["frame_split", "frame_split", "deferred", "deferred", "deferred", "deferred"], c
        assert {at[n]["p2v"] for n in ns if UW.forms(n, 12, 23, frame_small=False)["p2v"] == "frame64"} == {"ctx", "ctx_ragged"}, c
        assert 55 in UW.MASKS and 23 in UW.MASKS  # (test_composite_decodes runs every mask of MASKS on each case)

    # MVT_APPLY_GENERIC / MVT_CONCAT_GENERIC / MVT_FOLD_DOWNSAMPLE
    claims["apply-generic"] = ({("apply", "generic", "b", True)} & apply_reach(True), apply_reach(False))
    claims["concat-generic"] = ({("concat", "generic", "b")} & concat_reach(CONCAT_BF16, True), concat_reach(range(len(EN.CONCAT)), False))
    # (the launch list's `fold` IS the switch: what this claim adds is that the selected composite cases have strided blocks of both
    # widths at all; that the library reads the variable is the source scan's part, test_table_names_every_once_per_process_switch)
    claims["fold-downsample-0"] = (strided_launches(EW_CASES, False), strided_launches(EW.CASES, True))
    assert claims["fold-downsample-0"][0] == {("strided", k, co, 1) for k in (3, 1) for co in set(EW.R.COUTS[1:])}

    assert set(claims) == {r.name for r in SWITCHES}
    for name, (claimed, default_reach) in claims.items():
        assert claimed, f"{name}: its selected cases reach nothing that the row claims"
        assert not (claimed & default_reach), f"{name}: a default-environment case already reaches {sorted(claimed & default_reach, key=str)}"


def test_knn_cases_straddle_every_query_group():
    """N in (1, 3, 9), with and without tile boxes: for Q = 2, 4, 8 there is a case with N < Q, one with N > Q and N % Q == 1, and
    the last query group is ragged (N % Q != 0) in every case (N is odd)."""
    shapes = {(c.coords.shape[0], bool(c.boxed)) for c in knn_selected_cases()}
    assert {n for n, _ in shapes} == {1, 3, 9}
    for boxed in (False, True):
        ns = {n for n, b in shapes if b == boxed}
        assert ns == {1, 3, 9}, (boxed, ns)
        for q in (2, 4, 8):
            assert any(n < q for n in ns) and any(n > q and n % q == 1 for n in ns) and all(n % q for n in ns)
    assert all(KC.knn_queries_per_wave(b, q) == q for b in (False, True) for q in (1, 2, 3, 4, 8))
    assert KC.knn_queries_per_wave(True, 0) == 2 and KC.knn_queries_per_wave(False, 0) == 8


@pytest.mark.parametrize("c", SIXTEEN_CASES, ids=EN.conv_id)
def test_sixteen_row_references_stay_inside(c):
    """The condition of the exact statistics (|Y| <= 180, integers) on the sizes that this module adds."""
    for (H, W) in SIXTEEN_GEOS:
        Y = EN.case_data(c, H, W)["Y"]
        assert float(Y.abs().max()) <= EN.YMAX and torch.equal(Y, Y.round())
        assert H % 16 == 0 and EN.tile_rows(c, H, 1) == 16 and EN.tile_rows(c, H, 0) == 8 and EN.tile_rows(c, H, 2) == 4


# ================================================================== CPU: the runner itself

CPU_NODE = "tests/test_gpu_matmul_exact.py::test_cases_reach_every_variant"
PROBE_NODE = f"{THIS}::test_child_sees_the_probe_variable"


def probe_row(nodes_, expect, env=None):
    return Row("probe", env or {}, "runner probe", nodes_, expect, None, 300, "not gpu")


def test_runner_probes(monkeypatch):
    """The runner passes a good row and fails: a selection that matches no test, a wrong expected count, a child that skips a test;
    and the child really sees the row's variable (the probe test asserts its value and skips without it).  Three children."""
    monkeypatch.setattr(sys.modules[__name__], "FAULTED", [])
    good = probe_row([CPU_NODE, PROBE_NODE], 2, {"MVT_SWITCH_PROBE": "17"})
    assert run_row(good) is None
    for expect in (1, 3, 0):  # the same run against a wrong count
        assert f"expects {expect}" in judge(good._replace(expect=expect), *run_row.last)
    assert "skipped" in run_row(probe_row([CPU_NODE, PROBE_NODE], 1))  # without the variable: one passed, one skipped
    assert run_row(probe_row([CPU_NODE + "_no_such_test"], 1)) is not None and run_row.last[0] != 0
    assert FAULTED == []


def test_judge_and_summary_parsing():
    row = probe_row([CPU_NODE], 3)
    assert summary_counts("...\n3 passed in 0.12s\n") == {"passed": 3}
    assert summary_counts("x\n===== 3 passed, 1 skipped, 2 warnings in 10.01s (0:00:10) =====\n") == {"passed": 3, "skipped": 1, "warnings": 2}
    assert summary_counts("no summary here") == {}
    assert judge(row, 0, "3 passed, 2 warnings in 1.00s") is None
    for rc, out in [(1, "2 passed, 1 failed in 1.00s"), (0, "2 passed in 1.00s"), (0, "3 passed, 1 skipped in 1.00s"), (0, "3 passed, 4 deselected in 1.00s"),
                    (0, "3 passed, 1 error in 1.00s"), (0, "3 passed, 1 xfailed in 1.00s"), (0, ""), (5, "no tests ran in 0.01s"), (2, "3 passed in 1.00s")]:
        assert judge(row, rc, out) is not None, (rc, out)
    assert all(is_fault(rc, "") for rc in (-6, -11, -9, 134, 139, 124, 137)) and not is_fault(0, "3 passed") and not is_fault(1, "1 failed")
    assert is_fault(1, "HIP error: an illegal memory access was encountered")


@pytest.mark.parametrize("ending", [-11, 134, "timeout", "fault text"])
def test_a_faulted_child_stops_every_later_row(ending, monkeypatch):
    """After a child that ended by signal, abort or time limit, or that reported a GPU memory fault, no further child is started."""
    me = sys.modules[__name__]
    monkeypatch.setattr(me, "FAULTED", [])
    started = []

    def fake_run(cmd, **kw):
        started.append(cmd)
        if ending == "timeout":
            raise subprocess.TimeoutExpired(cmd, kw["timeout"], output="1 passed so far")
        if ending == "fault text":
            return subprocess.CompletedProcess(cmd, 1, stdout="E  HIP error: an illegal memory access was encountered\n1 failed in 2.00s\n")
        return subprocess.CompletedProcess(cmd, ending, stdout="")

    monkeypatch.setattr(me.subprocess, "run", fake_run)
    first = run_row(CHILDREN[0])
    assert first is not None and len(started) == 1 and len(me.FAULTED) == 1
    for row in CHILDREN[1:]:
        why = run_row(row)
        assert why is not None and why.startswith("not started") and CHILDREN[0].name in why
    assert len(started) == 1
    # an ordinary failure latches nothing
    monkeypatch.setattr(me, "FAULTED", [])
    monkeypatch.setattr(me.subprocess, "run", lambda cmd, **kw: subprocess.CompletedProcess(cmd, 1, stdout="1 failed in 2.00s\n"))
    assert run_row(CHILDREN[0]) is not None and run_row(CHILDREN[1]) is not None and me.FAULTED == []
