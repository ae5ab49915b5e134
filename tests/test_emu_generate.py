"""CPU (-m "not gpu"): the matchers' sequences out, the lane-serial build of zstd-jni_amd/csrc/zj_generate.h (tests/emu_generate/): the parse-then-export frame loop
and the export alone on records the test writes.  Every case of tests/generate_cases.py
must answer what the reference's ZSTD_generateSequences answers — the array entry for entry, or its error code.  The emulation's workgroup state (uniforms, LDS,
scratch, tables) is poisoned once and outlives every frame, as a persistent workgroup's does; the source is an exact-size heap block and the slots sit between
canaries the emulation checks itself.  The -m gpu twin is tests/test_gpu_generate.py."""
import ctypes as C
import os

import pytest

from util import emu_so

import generate_cases as GC
import sequences_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOUCHED = 0xFFFFFFFFFFFF0001


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_generate", "libzjni_emu_generate.so"))
    L.emu_generate.restype = C.c_ulonglong
    L.emu_generate.argtypes = [C.c_char_p, C.c_uint, C.c_int, C.c_void_p, C.c_ulonglong, C.c_int]
    L.emu_export_records.restype = C.c_ulonglong
    L.emu_export_records.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_ulonglong]
    L.emu_merge_block_delimiters.restype = C.c_ulonglong
    L.emu_merge_block_delimiters.argtypes = [C.c_void_p, C.c_ulonglong]
    L.emu_generate_refusal.restype = C.c_uint
    L.emu_generate_refusal.argtypes = [C.c_int, C.c_ulonglong]
    return L


@pytest.fixture(scope="module")
def emu_seq():
    L = C.CDLL(emu_so("emu_sequences", "libzjni_emu_sequences.so"))
    L.emu_compress_sequences.restype = C.c_ulonglong
    L.emu_compress_sequences.argtypes = [C.c_char_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_int, C.c_uint]
    return L


def rows(arr, n):
    return [tuple(arr[4 * i:4 * i + 4]) for i in range(n)]


def run(emu, c, route=0, cap=None):
    """the emulation's answer for a case: [(offset, litLength, matchLength, rep)] or -code"""
    if cap is None:
        cap = SC._lib().ZSTD_sequenceBound(len(c.data))
    out = (C.c_uint32 * (4 * max(cap, 1)))()
    r = emu.emu_generate(c.data, len(c.data), c.level, out, cap, route)
    assert r != TOUCHED, (c.name, c.level, cap, "something outside the slots was written")
    if r >= 1 << 63:
        return -((1 << 64) - r)
    assert r <= cap
    return rows(out, r)


@pytest.mark.parametrize("group", GC.GROUPS)
def test_emu_generate_every_case_is_the_references_answer(emu, oracle_ref, group):
    cases = getattr(GC, group)()
    assert len(cases) >= 6
    for c in cases:
        GC.check(c, run(emu, c))


def test_emu_generate_cases_are_what_they_claim(oracle_ref):
    """the reference on the cases themselves: refusals, block cuts, repcodes where the blocks begin, long lengths, blocks of one delimiter"""
    by = {(c.name, c.level): c for c in GC.every_case()}
    for level in GC.EVERY:
        assert GC.expected(by[("text/0", level)]) == []
        for n in (1, 6, GC.BLOCK + 1, GC.BLOCK + 6):
            assert GC.expected(by[(f"text/{n}", level)]) == -GC.E_PRODUCER, (n, level)
        assert GC.expected(by[("text/7", level)]) == [(0, 7, 0, 0)]
        two = GC.blocks_of(GC.expected(by[(f"text/{GC.BLOCK + 7}", level)]))
        assert len(two) == 2 and two[1] == ([], 7)
        assert sum(ll + ml for ll, ml in ((s[1], s[2]) for s in two[0][0])) + two[0][1] == GC.BLOCK
        assert len(GC.blocks_of(GC.expected(by[(f"text/{3 * GC.BLOCK + 5000}", level)]))) == 4
        blocks = GC.blocks_of(GC.expected(by[("periodic/3-blocks", level)]))
        assert len(blocks) == 3
        for b in blocks[1:]:
            assert any(s[3] for s in b[0][:3]), (level, b[0][:3])
        assert any(s[2] >= 65536 for s in GC.expected(by[("ml>=65536", level)]))
        assert any(s[1] >= 65536 for s in GC.expected(by[("ll>=65536", level)]))
        assert GC.expected(by[("noise/1-block", level)]) == [(0, GC.BLOCK, 0, 0)]
        assert len(GC.blocks_of(GC.expected(by[("noise-text-noise-text", level)]))) == 4
    for n in (1, 6, GC.BLOCK + 1, GC.BLOCK + 6):
        assert GC.ref_answer(GC.text(n), 5) == -GC.E_PRODUCER, n


def test_emu_generate_refusals_before_any_parse(emu):
    for level, n, want in ((3, 0, 0), (3, 1, 106), (3, 6, 106), (3, 7, 0), (3, GC.BLOCK + 3, 106), (3, 5 * GC.BLOCK + 6, 106), (3, (2 << 20) + 1, 201), (1, (512 << 10) + 1, 201),
                           (1, 512 << 10, 0), (2, (1 << 20) + 1, 201), (-7, (512 << 10) + 1, 201), (4, GC.BLOCK + 1, 201), (4, GC.BLOCK, 0), (8, GC.BLOCK, 0), (8, GC.BLOCK + 7, 201), (0, 700, 0)):
        assert emu.emu_generate_refusal(level, n) == want, (level, n)


def test_emu_generate_small_random_inputs(emu, oracle_ref):
    cases = GC.small_random()
    assert len(cases) == 300
    for c in cases:
        GC.check(c, run(emu, c))


def test_emu_export_alone_on_hand_written_records(emu):
    for name, recs, last_ll, hist in GC.export_cases():
        n = len(recs)
        flat = [v for k, (ll, ml, ob) in enumerate(recs) for v in (ll | (0x5A << 24), ml | (0x3C << 24), ob | (0x11 << 24), 0xC0000000 + k)]      # code bytes above bit 24 are not the export's
        rec = (C.c_uint32 * max(len(flat), 1))(*flat)
        want = GC.export_model(recs, last_ll, hist)
        for cap in (n + 1, n + 5, n, 0):
            out = (C.c_uint32 * (4 * max(cap, 1)))()
            r = emu.emu_export_records(rec, n, last_ll, hist[0], hist[1], hist[2], out, cap)
            assert r != TOUCHED, (name, cap)
            if cap < n + 1:
                assert r == (1 << 64) - GC.E_DST, (name, cap, r)
            else:
                assert r == n + 1 and rows(out, r) == want, (name, cap)


def test_emu_generate_every_capacity(emu, oracle_ref):
    frames = GC.capacity_frames()
    assert len(GC.blocks_of(GC.expected(frames[2]))) == 2 and len(GC.blocks_of(GC.expected(frames[0]))) == 1
    for c in frames:
        full = GC.expected(c)
        first = len(GC.blocks_of(full)[0][0]) + 1
        seen = set()
        for cap in range(0, len(full) + 2):
            got = run(emu, c, 0, cap)
            GC.check(c, got, cap)
            assert got == (full if cap >= len(full) else -GC.E_DST), (c.name, cap)
            seen.add(cap >= first)
        assert seen == {False, True}                                      # the two-block frame: capacities that hold the first block and not the second answer 70


def test_emu_generate_round_trip_through_compress_sequences(emu, emu_seq, oracle_ref):
    cases = [c for c in GC.sizes() + GC.levels() + GC.repcodes() if isinstance(GC.expected(c), list) and len(c.data) <= GC.BLOCK + 7 and len(c.data)]
    assert len(cases) >= 30
    for c in cases:
        seqs = run(emu, c)
        words = SC.flat(seqs)
        arr = (C.c_uint32 * max(len(words), 1))(*words)
        for flags in (0, SC.REPCODES):
            cap = len(c.data) + (len(c.data) >> 8) + 128 + 3 * (len(seqs) + 1)
            dst = C.create_string_buffer(cap)
            r = emu_seq.emu_compress_sequences(c.data, len(c.data), arr, len(seqs), dst, cap, c.level, flags)
            if r == (1 << 64) - 201:
                assert c.level >= 5 and len(c.data) > GC.BLOCK                # (a second block at a lazy level: the compress-sequences entry's own limit)
                continue
            assert r < 1 << 63, (c.name, c.level, flags, (1 << 64) - r)
            assert oracle_ref.decompress(dst.raw[:r], len(c.data)) == c.data, (c.name, c.level, flags)


def test_emu_merge_block_delimiters_is_the_references(emu, oracle_ref):
    R = SC._lib()
    R.ZSTD_mergeBlockDelimiters.restype = C.c_size_t
    R.ZSTD_mergeBlockDelimiters.argtypes = [C.c_void_p, C.c_size_t]
    for seqs in ([(5, 3, 4, 0), (0, 9, 0, 0)], [(5, 3, 4, 0), (0, 2, 0, 0), (0, 7, 0, 0), (9, 1, 6, 1), (0, 0, 0, 0)], [(5, 3, 4, 0), (7, 0, 5, 2)], [], [(0, 4, 0, 0)],
                 GC.ref_answer(GC.text(3000), 3)):
        words = SC.flat(seqs)
        a = (C.c_uint32 * max(len(words), 1))(*words)
        b = (C.c_uint32 * max(len(words), 1))(*words)
        na, nb = emu.emu_merge_block_delimiters(a, len(seqs)), R.ZSTD_mergeBlockDelimiters(b, len(seqs))
        assert na == nb and list(a) == list(b), seqs[:4]
