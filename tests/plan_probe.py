"""Compile-and-run helper of the host-side plan tests (test_launch_plan_host.py, test_conv_plan_host.py).

The plan headers of mvtracker_amd/csrc are HIP-free, so the host compiler alone builds a probe program around one of them
(-Wall -Werror: the compile itself checks that the header needs nothing of HIP); the probe reads one case per line of stdin and
answers on stdout.  Each test module runs its probe ONCE over all of its cases.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_probe(tmp_path_factory, source, lines, timeout=300):
    """Builds tests/<source> and feeds it `lines`; -> its stdout lines.  Skips the test where there is no host C++ compiler."""
    cxx = shutil.which("g++") or next((c for c in ("/opt/rocm/llvm/bin/clang++",) if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp(os.path.splitext(source)[0]) / "probe"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", source), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # (also: the header needs nothing of HIP)
    p = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr
    return p.stdout.splitlines()
