"""CPU (-m "not gpu"): the cases of tests/branch_cases.py still reach the lines they exist for.  tools/emu_coverage.py builds the emulation libraries that hold the lines
(branch_cases.CASE_LIBS) with line counters outside the tree, runs the case tests (branch_cases.CASE_TESTS) in a child pytest and counts; every line named in branch_cases.LINES — found by its text,
so edits above it do not matter — must have been executed.  The listing over the whole suite and its check against tests/emu/unreached.txt stay a tool run."""
import importlib.util
import os
import shutil

import pytest

import branch_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_case_reaches_its_line(oracle_ref):
    if not shutil.which("gcov") or not shutil.which("g++"):
        pytest.skip("gcov is not installed")
    spec = importlib.util.spec_from_file_location("emu_coverage", os.path.join(ROOT, "tools", "emu_coverage.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    merged, rc = tool.measure(list(B.CASE_TESTS), only=B.CASE_LIBS)
    assert rc == 0, "the case tests failed in the counting build"
    counts = {name: tool.count_of(merged, header, fragment) for name, (header, fragment) in B.LINES.items()}
    print(counts)
    assert all(c > 0 for c in counts.values()), counts
    # the tool's own check: a line without counts is reported, a listed line that ran is reported
    text, zero = tool.listing({"zj_simt.h": {1: 0, 2: 5}})
    assert len(zero) == 1 and tool.check(zero, []) and not tool.check(zero, [("zj_simt.h", zero[0][2].strip() or "//", "compiler artefact")])
