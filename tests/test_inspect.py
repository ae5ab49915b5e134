"""CPU (-m "not gpu"): zjni_inspect — one walk over a buffer's frame and block headers — answers what the reference's four header-only
calls answer (ZSTD_findDecompressedSize, ZSTD_decompressBound, ZSTD_findFrameCompressedSize, ZSTD_getDictID_fromFrame), field for
field, for valid, truncated and damaged input alike.  Every buffer is handed over as an exact-size heap copy."""
import collections

import pytest

import inspect_cases as ic


@pytest.fixture(scope="module")
def corpus(zj, oracle_ref):
    cases, valid = ic.build_cases(oracle_ref)
    return cases, valid, ic.setup_ref(oracle_ref)


def code_of(size):
    return (1 << 64) - size if size > (1 << 64) - 121 else 0


def test_inspect_equals_the_reference_on_every_input(zj, corpus):
    cases, _, R = corpus
    codes, contents = collections.Counter(), collections.Counter()
    assert len(cases) > 3500
    for c in cases:
        fi = ic.host_info(zj.lib(), c.data)
        want = ic.ref_info(R, c.data)
        assert (fi.content, fi.bound, fi.firstFrameSize, fi.dictID) == want, (c.name, c.data[:24].hex(), len(c.data))
        codes[code_of(fi.firstFrameSize)] += 1
        contents["unknown" if fi.content == ic.UNKNOWN else "error" if fi.content == ic.ERROR else "size"] += 1
    # the inputs did reach every refusal the walk can give, both sentinels and plain sizes
    for code in (0, 10, 14, 16, 20, 72):
        assert codes[code] > 0, (code, codes)
    assert contents["unknown"] > 0 and contents["error"] > 0 and contents["size"] > 0, contents


def test_counts_and_flags_by_construction(zj, corpus):
    cases, _, _ = corpus
    known = [c for c in cases if c.counts is not None]
    assert len(known) >= 30
    seen = set()
    for c in known:
        fi = ic.host_info(zj.lib(), c.data)
        assert (fi.frames, fi.skippable, fi.flags) == c.counts, (c.name, fi.frames, fi.skippable, fi.flags)
        seen.add(fi.flags)
    assert {0, ic.SINGLE, ic.SINGLE | ic.CHECKSUM, ic.SINGLE | ic.NOSIZE, ic.CHECKSUM | ic.NOSIZE | ic.SINGLE, ic.CHECKSUM, ic.NOSIZE} <= seen


def test_the_facts_the_walk_was_built_on(zj, corpus):
    """the reference's behaviour the issue lists, asked of the reference itself and of the walk"""
    import struct
    _, _, R = corpus
    small = ic.golden("xmlsmall-sized.zst")

    def both(z):
        fi = ic.host_info(zj.lib(), z)
        got = (fi.content, fi.bound, fi.firstFrameSize, fi.dictID)
        assert got == ic.ref_info(R, z), z[:24].hex()
        return got

    assert both(b"") == (0, 0, (1 << 64) - 72, 0)
    for k in (1, 2, 3, 4):
        assert both(small + b"\x00" * k)[:2] == (ic.ERROR, ic.ERROR)
    assert both(small)[:3] == (102, 102, len(small))
    assert code_of(both(b"\x00" + small[1:])[2]) == 10
    assert code_of(both(small[:4] + bytes([small[4] | 8]) + small[5:])[2]) == 14
    assert code_of(both(small[:6] + bytes([small[6] | 6]) + small[7:])[2]) == 20
    assert code_of(both(small[:-1])[2]) == 72
    assert code_of(both(struct.pack("<IBB", 0xFD2FB528, 0x00, 0xB0) + b"\x01\x00\x00")[2]) == 16
    assert both(ic.skippable(b"abc", 15))[3] == 15
    assert code_of(both(struct.pack("<II", 0x184D2A5F, 0xFFFFFFFC) + b"abcd")[2]) == 14
    two = struct.pack("<IBQ", 0xFD2FB528, 0xE0, 1 << 63) + b"\x01\x00\x00"
    assert both(two)[0] == 1 << 63 and both(two + two)[0] == ic.ERROR


def test_python_helper(zj):
    fi = zj.inspect(ic.golden("xmlsmall-sized.zst"))
    assert (fi.content, fi.frames, fi.skippable, fi.flags & zj.INFO_SINGLE) == (102, 1, 0, zj.INFO_SINGLE)
    assert zj.inspect(b"").firstFrameSize == (1 << 64) - 72


def test_walk_under_sanitizers(oracle_ref, tmp_path):
    """zj_frameinfo.h alone under a plain C++ compiler with AddressSanitizer + UndefinedBehaviorSanitizer; tests/inspect_host.cpp walks a malloc copy of
    exactly srcSize bytes, so a read past a truncated buffer's last byte stops the run.  The guard is proven first: the same build with one deliberate
    read of the byte behind the copy (-DINSPECT_OVERREAD) must be stopped on a 7-byte and on a 103-byte buffer — sizes at which a ctypes copy alone,
    living in Python's own small-object arenas, lets such a read pass."""
    import os
    import subprocess
    import sys
    rt = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(rt) and os.path.exists(rt), "the host sanitizer runtime (libasan) is part of the toolchain this suite needs"
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def build(name, *defs):
        so = str(tmp_path / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-shared", "-fPIC",
                               *defs, "-o", so, os.path.join(here, "inspect_host.cpp")])
        return so

    probe = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); z = open(sys.argv[2], 'rb').read()[:int(sys.argv[3])]; out = (C.c_uint64 * 5)(); "
             "L.zjni_inspect.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]; L.zjni_inspect((C.c_ubyte * len(z)).from_buffer_copy(z), len(z), out); print('returned', out[0])")
    small = os.path.join(here, "golden", "xmlsmall-sized.zst")
    bad, good = build("libinspect_overread.so", "-DINSPECT_OVERREAD"), build("libinspect_asan.so")
    for size in (7, 103):
        r = subprocess.run([sys.executable, "-c", probe, bad, small, str(size)], env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr and "returned" not in r.stdout, (size, r.returncode, r.stderr[-1500:])
        r = subprocess.run([sys.executable, "-c", probe, good, small, str(size)], env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "returned" in r.stdout and "AddressSanitizer" not in r.stderr, (size, r.stderr[-1500:])
    r = subprocess.run([sys.executable, os.path.join(here, "inspect_cases.py"), good], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "mismatches=0" in r.stdout, r.stdout[-2000:]
