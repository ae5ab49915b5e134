"""Which lines of the device headers does the CPU suite never execute?

Builds the lane-serial library with line counters (`make -C tests/emu cov`), runs the given test files in a child `python -m pytest` with ZJNI_EMU_LIB set to it
(the counts are written when that process ends), runs gcov, adds up the template instances of every source line and prints, per header of zstd-jni_amd/csrc/,
the lines whose count is zero.  tests/emu/unreached.txt holds the lines that are allowed to stay at zero (`header | a fragment that singles the line out among the header's unexecuted lines | reason`):
the tool exits 1 when an unexecuted line has no row, and when a row's line was executed after all.

    python tools/emu_coverage.py                          # the CPU files that load the library (DEFAULT_FILES), checked against unreached.txt
    python tools/emu_coverage.py --no-check tests/test_emu_tans.py
    python tools/emu_coverage.py --out listing.txt

Object, library and counter files go to a temporary directory (or --covdir); nothing is written into the tree."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstd-jni_amd", "csrc")
UNREACHED = os.path.join(ROOT, "tests", "emu", "unreached.txt")
REASONS = ("waits for another kernel", "tuning-build switch", "excluded by invariant", "executed in another emulation library", "compiler artefact")
MAX_ROWS = 20
# every CPU test file that calls util.emu_lib(), but test_bench_gloo (it starts the benchmark)
DEFAULT_FILES = ["test_emu_encode.py", "test_emu_level4.py", "test_emu_multiblock.py", "test_emu_cdict.py", "test_emu_seqrecords.py", "test_emu_tans.py", "test_emu_stream.py",
                 "test_emu_decode.py", "test_emu_decode_multiblock.py", "test_emu_seqframes.py", "test_corrupt_frames.py", "test_emu_branches.py"]


def build(covdir):
    out = subprocess.check_output(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "cov", "COVDIR=" + covdir], text=True)
    lib = out.strip().splitlines()[-1]
    assert os.path.exists(lib), out
    return lib


def run_tests(lib, files, quiet=True):
    env = dict(os.environ, ZJNI_EMU_LIB=lib)
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"] + files
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 or not quiet:
        sys.stderr.write(r.stdout[-4000:])
    return r.returncode


def counts(covdir):
    """{header name: {line number: executions, summed over the instances of the line}} for the headers of csrc/"""
    subprocess.check_call(["gcov", "--json-format", "-o", covdir, os.path.join(covdir, "emu.gcda")], cwd=covdir, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    merged = {}
    for name in os.listdir(covdir):
        if not name.endswith(".gcov.json.gz"):
            continue
        with gzip.open(os.path.join(covdir, name), "rt") as f:
            doc = json.load(f)
        for fl in doc["files"]:
            path = os.path.normpath(os.path.join(doc.get("current_working_directory", covdir), fl["file"]))
            if os.path.dirname(path) != CSRC:
                continue
            per = merged.setdefault(os.path.basename(path), {})
            for ln in fl["lines"]:
                per[ln["line_number"]] = per.get(ln["line_number"], 0) + ln["count"]
    return merged


def source_lines(header):
    with open(os.path.join(CSRC, header)) as f:
        return f.read().split("\n")


def measure(files, covdir=None):
    """build, run, count: ({header: {line: count}}, pytest's exit code)"""
    own = covdir is None
    covdir = tempfile.mkdtemp(prefix="zjni_cov_") if own else os.path.abspath(covdir)
    try:
        lib = build(covdir)
        for n in os.listdir(covdir):
            if n.endswith(".gcda"):
                os.remove(os.path.join(covdir, n))
        rc = run_tests(lib, files)
        return counts(covdir), rc
    finally:
        if own:
            shutil.rmtree(covdir, ignore_errors=True)


def count_of(merged, header, fragment):
    """executions of the one line of `header` whose text holds `fragment` (found by text, so edits above it do not matter)"""
    hits = [i + 1 for i, t in enumerate(source_lines(header)) if fragment in t]
    assert len(hits) == 1, f"{header}: {fragment!r} is on {len(hits)} lines, not one"
    assert hits[0] in merged.get(header, {}), f"{header}:{hits[0]} holds no code"
    return merged[header][hits[0]]


def read_rows(path=UNREACHED):
    rows = []
    with open(path) as f:
        for raw in f:
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            header, fragment, reason = (p.strip() for p in line.split("|", 2))
            rows.append((header, fragment, reason))
    return rows


def listing(merged):
    """the text of the listing and [(header, line number, text)] of the unexecuted lines"""
    out, zero = [], []
    for header in sorted(merged):
        per, text = merged[header], source_lines(header)
        miss = sorted(n for n, c in per.items() if c == 0)
        out.append(f"{header}: {len(per) - len(miss)} of {len(per)} lines executed ({100.0 * (len(per) - len(miss)) / max(len(per), 1):.1f} %)")
        for n in miss:
            out.append(f"  {n:5d}: {text[n - 1].strip()[:150]}")
            zero.append((header, n, text[n - 1]))
    return "\n".join(out) + "\n", zero


def check(zero, rows):
    """the complaints: unexecuted lines without a row, rows that single out no unexecuted line (it was executed after all, or its text changed) or more than one,
    rows outside the conditions"""
    bad = []
    if len(rows) > MAX_ROWS:
        bad.append(f"unreached.txt has {len(rows)} rows, {MAX_ROWS} at most")
    hits = [0] * len(rows)
    for header, n, text in zero:
        hit = [k for k, (h, frag, _) in enumerate(rows) if h == header and frag in text]
        if not hit:
            bad.append(f"{header}:{n} never executed and not listed: {text.strip()[:120]}")
        for k in hit:
            hits[k] += 1
    for k, (header, frag, reason) in enumerate(rows):
        if not any(reason.startswith(r) for r in REASONS):
            bad.append(f"row {header} | {frag}: the reason must begin with one of {REASONS}")
        if hits[k] == 0:
            bad.append(f"row {header} | {frag}: no unexecuted line of the header holds this text — it was executed after all (or changed): drop the row")
        elif hits[k] > 1:
            bad.append(f"row {header} | {frag}: {hits[k]} unexecuted lines hold this text, a row names one")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="*", help="test files (default: the CPU files that load the library)")
    ap.add_argument("--covdir", help="where library and counters go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", help="also write the listing to this file")
    ap.add_argument("--no-check", action="store_true", help="print the listing only (a subset of the files leaves more lines out)")
    a = ap.parse_args()
    if not shutil.which("gcov"):
        sys.exit("gcov not found")
    files = a.files or [os.path.join("tests", f) for f in DEFAULT_FILES if os.path.exists(os.path.join(ROOT, "tests", f))]
    merged, rc = measure(files, a.covdir)
    text, zero = listing(merged)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if rc != 0:
        sys.exit(f"the tests failed (pytest exit {rc}): the counts are of a partial run")
    if a.no_check:
        return
    bad = check(zero, read_rows() if os.path.exists(UNREACHED) else [])
    for b in bad:
        print("UNREACHED:", b)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
