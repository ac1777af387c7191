"""tests/golden/launch_sequence.json: the launch sequence of the host code on the mocked library, per case of
tests/launch_sequence_cases.py (entry names in call order, SHA-256 of the full records, SHA-256 of the result tensors' bytes).

The fixture pins what the host code did BEFORE the model class was split into weights / encoder / updater / frame-store mixins:
it was recorded once, with the ``mvtracker_amd`` of the commit before that split on the path (commit 101f48d), and
tests/test_launch_sequence_host.py compares every later tree with it.  It is never regenerated from the code under test -- a
deliberate change of the launch sequence regenerates it from the commit BEFORE that change only to show what differs, and then
records the new sequence with the reason in the commit message.

    python tests/golden/make_launch_sequence.py [PACKAGE_ROOT]

PACKAGE_ROOT: a checkout whose ``mvtracker_amd`` is recorded (default: this one).  The recording code always comes from this
checkout's tests/.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(TESTS))

import launch_sequence_cases as L  # noqa: E402
import mvtracker_amd  # noqa: E402

out = {}
for case in L.CASES:
    with pytest.MonkeyPatch.context() as mp:
        out[case] = L.record(mp, case)
    print(case, len(out[case]["names"]), "calls")
path = os.path.join(HERE, "launch_sequence.json")
with open(path, "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print("recorded", os.path.dirname(mvtracker_amd.__file__), "->", path, os.path.getsize(path) / 1024, "KiB")
