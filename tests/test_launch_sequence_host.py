"""The host code's launch sequence on the mocked library, pinned: entry names in call order, every scalar positional argument
and the result bits of each case of tests/launch_sequence_cases.py against tests/golden/launch_sequence.json -- recorded once
from the tree before the model class was split by concern (tests/golden/make_launch_sequence.py), never from the code under
test.  The grouped and composite paths have no CPU mock; the `-m gpu` suites cover them."""
import json
import os

import pytest

import launch_sequence_cases as L

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_sequence.json")) as f:
    GOLDEN = json.load(f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(L.CASES)


@pytest.mark.parametrize("case", sorted(L.CASES))
def test_launch_sequence(monkeypatch, case):
    got, ref = L.record(monkeypatch, case), GOLDEN[case]
    assert len(got["names"]) == len(ref["names"])
    first = next((i for i, (a, b) in enumerate(zip(got["names"], ref["names"])) if a != b), None)
    assert first is None, f"call {first}: {got['names'][first]} where the fixture has {ref['names'][first]}"
    assert got["records_sha256"] == ref["records_sha256"]  # same entries, another scalar argument somewhere
    assert got["results_sha256"] == ref["results_sha256"]


def test_mlp_fused_branch_is_covered():
    """The 280-track case exists for the rows >= 4096 branch of the unfused bf16 path."""
    assert "mlp_fused_bf16" in GOLDEN["update_former_bf16_unfused_280"]["names"]
    assert "mlp_fused_bf16" not in GOLDEN["update_former_bf16_unfused"]["names"]
