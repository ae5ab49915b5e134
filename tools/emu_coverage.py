"""Which lines of the device headers does the CPU suite never execute?

Builds EVERY emulation library under tests/emu*/ (tests/emu/emu.cpp and emu_wave.cpp, tests/emu_<name>/emu_<name>.cpp) with line counters, runs the given test files in
a child `python -m pytest` that loads those builds instead of the tree's (ZJNI_EMU_LIB for the lane-serial library, ZJNI_EMU_LIB_DIR for the others: util.emu_so; the
counts are written when that process ends), runs gcov per library, adds up the template instances of every source line over all libraries — a line counts as executed
if any library ran it — and prints, per header of zstd-jni_amd/csrc/, the lines whose count is zero.  tests/emu/unreached.txt holds the lines that are allowed to stay
at zero (`header | a fragment that singles the line out among the header's unexecuted lines | reason`): the tool exits 1 when an unexecuted line has no row, and when a
row's line was executed after all.

    python tools/emu_coverage.py                          # the CPU files that load the libraries (DEFAULT_FILES), checked against unreached.txt
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
REASONS = ("waits for another kernel", "tuning-build switch", "excluded by invariant", "compiler artefact")
MAX_ROWS = 20
# every CPU test file that loads an emulation library, but test_bench_gloo (it starts the benchmark) and test_emu_sanitizer (it loads builds of its own)
DEFAULT_FILES = ["test_emu_encode.py", "test_emu_level4.py", "test_emu_multiblock.py", "test_emu_cdict.py", "test_emu_seqrecords.py", "test_emu_tans.py", "test_emu_stream.py",
                 "test_emu_decode.py", "test_emu_decode_multiblock.py", "test_emu_seqframes.py", "test_corrupt_frames.py", "test_emu_branches.py",
                 "test_emu_wave.py", "test_emu_negative_levels.py", "test_emu_negative_dict_stream.py", "test_emu_cstream.py", "test_emu_cstream_pieces.py", "test_emu_pieces.py",
                 "test_emu_frames.py", "test_emu_frames_range.py", "test_emu_index.py", "test_emu_index_walk.py", "test_emu_generate.py", "test_emu_sequences.py",
                 "test_emu_sequences_nodelim.py"]


def libraries():
    """[(name, source)]: tests/emu*/emu*.cpp — `name`.cpp builds libzjni_`name`.so (the stand-alone programs beside them, *_main.cpp, are not libraries)"""
    out = []
    tests = os.path.join(ROOT, "tests")
    for d in sorted(os.listdir(tests)):
        if d == "emu" or d.startswith("emu_"):
            for f in sorted(os.listdir(os.path.join(tests, d))):
                if f.startswith("emu") and f.endswith(".cpp"):
                    out.append((f[:-4], os.path.join(tests, d, f)))
    return out


def build(covdir, only=None, jobs=8):
    """every library (or those named in `only`) with counters: objects and counts in covdir/<name>/, the libraries in covdir/lib/.  {name: library path}"""
    libdir = os.path.join(covdir, "lib")
    os.makedirs(libdir, exist_ok=True)
    todo, running, libs = [(n, src) for n, src in libraries() if only is None or n in only], [], {}
    assert todo, "no emulation library found"
    while todo or running:
        while todo and len(running) < jobs:
            name, src = todo.pop(0)
            d = os.path.join(covdir, name)
            os.makedirs(d, exist_ok=True)
            lib = os.path.join(libdir, f"libzjni_{name}.so")
            cmd = f'g++ -O1 -g --coverage -std=c++17 -fPIC -c -o "{d}/{name}.o" "{src}" && g++ --coverage -shared -o "{lib}" "{d}/{name}.o"'
            running.append((name, lib, subprocess.Popen(cmd, shell=True, cwd=d)))
        name, lib, p = running.pop(0)
        assert p.wait() == 0 and os.path.exists(lib), f"building {name} with counters failed"
        libs[name] = lib
    return libs


def run_tests(libs, files, quiet=True):
    env = dict(os.environ, ZJNI_EMU_LIB=libs["emu"], ZJNI_EMU_LIB_DIR=os.path.dirname(libs["emu"]))
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "not gpu", "-p", "no:cacheprovider"] + files
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 or not quiet:
        sys.stderr.write(r.stdout[-4000:])
    return r.returncode


def counts(covdir, libs):
    """{header name: {line number: executions, summed over the instances of the line and over the libraries}} for the headers of csrc/, and the libraries no test loaded"""
    merged, idle = {}, []
    for lib in sorted(libs):
        d = os.path.join(covdir, lib)
        if not os.path.exists(os.path.join(d, lib + ".gcda")):
            idle.append(lib)                                 # (its lines still count, as unexecuted, from the compiler's notes)
        subprocess.check_call(["gcov", "--json-format", "-o", d, os.path.join(d, lib + (".gcda" if lib not in idle else ".gcno"))], cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for name in os.listdir(d):
            if not name.endswith(".gcov.json.gz"):
                continue
            with gzip.open(os.path.join(d, name), "rt") as f:
                doc = json.load(f)
            for fl in doc["files"]:
                path = os.path.normpath(os.path.join(doc.get("current_working_directory", d), fl["file"]))
                if os.path.dirname(path) != CSRC:
                    continue
                per = merged.setdefault(os.path.basename(path), {})
                for ln in fl["lines"]:
                    per[ln["line_number"]] = per.get(ln["line_number"], 0) + ln["count"]
    return merged, idle


def source_lines(header):
    with open(os.path.join(CSRC, header)) as f:
        return f.read().split("\n")


def measure(files, covdir=None, idle=None, only=None):
    """build, run, count: ({header: {line: count}}, pytest's exit code); idle: a list that gets the libraries no test loaded; only: the libraries to count (default
    all — a library that is not counted is loaded from the tree as usual)"""
    own = covdir is None
    covdir = tempfile.mkdtemp(prefix="zjni_cov_") if own else os.path.abspath(covdir)
    try:
        libs = build(covdir, only)
        for lib in libs:
            stale = os.path.join(covdir, lib, lib + ".gcda")
            if os.path.exists(stale):
                os.remove(stale)
        rc = run_tests(libs, files)
        merged, unused = counts(covdir, libs)
        if idle is not None:
            idle += unused
        return merged, rc
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
    ap.add_argument("--libs", help="count these libraries only, e.g. emu,emu_wave (default: all; implies --no-check)")
    ap.add_argument("--no-check", action="store_true", help="print the listing only (a subset of the files leaves more lines out)")
    a = ap.parse_args()
    if not shutil.which("gcov"):
        sys.exit("gcov not found")
    files = a.files or [os.path.join("tests", f) for f in DEFAULT_FILES if os.path.exists(os.path.join(ROOT, "tests", f))]
    idle = []
    only = a.libs.split(",") if a.libs else None
    merged, rc = measure(files, a.covdir, idle, only)
    text, zero = listing(merged)
    text = f"libraries counted: {' '.join(name for name, _ in libraries() if only is None or name in only)}\n" + text
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    if rc != 0:
        sys.exit(f"the tests failed (pytest exit {rc}): the counts are of a partial run")
    if a.no_check or only:
        return
    if idle:
        sys.exit(f"no test loaded the counting build of: {' '.join(idle)}")
    bad = check(zero, read_rows() if os.path.exists(UNREACHED) else [])
    for b in bad:
        print("UNREACHED:", b)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
