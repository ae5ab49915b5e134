"""CPU (-m "not gpu"): frames from the caller's sequences, the lane-serial build of zstd-jni_amd/csrc/zj_sequences.h (tests/emu_sequences/): the conversion of a
ZSTD_Sequence array into the entropy stage's records and block entries, and the frame loop over the caller's blocks.  Every case of tests/sequences_cases.py must
answer what the reference's ZSTD_compressSequences answers — the frame byte for byte, or its error code — and where the reference made a decodable frame, that frame
decodes to the source.  The emulation's workgroup state (uniforms, LDS, scratch) is poisoned once and outlives every frame, as a persistent workgroup's does; source,
sequence array, slots and destination are exact-size heap blocks.  The -m gpu twin is tests/test_gpu_sequences.py."""
import ctypes as C
import os

import pytest

from util import emu_so

import sequences_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_sequences", "libzjni_emu_sequences.so"))
    L.emu_compress_sequences.restype = C.c_ulonglong
    L.emu_compress_sequences.argtypes = [C.c_char_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_int, C.c_uint]
    L.emu_sequence_bound.restype = C.c_ulonglong
    L.emu_sequence_bound.argtypes = [C.c_ulonglong]
    return L


def run(emu, c, cap=None):
    """the emulation's answer for a case: bytes or -code"""
    words = SC.flat(c.seqs)
    arr = (C.c_uint32 * max(len(words), 1))(*words)
    if cap is None:
        cap = len(c.data) + (len(c.data) >> 8) + 128 + 3 * (len(c.seqs) + 1)
    dst = C.create_string_buffer(max(cap, 1))
    r = emu.emu_compress_sequences(c.data, len(c.data), arr, len(c.seqs), dst, cap, c.level, c.flags)
    if r >= 1 << 63:
        return -((1 << 64) - r)
    assert r <= cap
    return dst.raw[:r]


@pytest.mark.parametrize("group", ("smallest", "from_generator", "multi_block", "long_codes"))
def test_emu_sequences_every_case_is_the_references_answer(emu, oracle_ref, group):
    cases = getattr(SC, group)()
    assert len(cases) >= 8
    for c in cases:
        SC.check(c, run(emu, c), oracle_ref)


def test_emu_sequences_other_levels(emu, oracle_ref):
    for c, served in SC.other_levels():
        got = run(emu, c)
        if served:
            SC.check(c, got, oracle_ref)
        else:
            assert got == -201 and isinstance(SC.expected(c), bytes), (c.name, got)


def test_emu_sequences_cases_are_what_they_claim(oracle_ref):
    """the reference on the cases themselves: which blocks become raw, RLE or compressed, and which arrays it refuses"""
    by = {(c.name, c.flags): c for c in SC.multi_block() + SC.long_codes()}

    def block_types(frame):
        """the type of every block of a frame without a dictionary ID"""
        fhd = frame[4]
        single = bool(fhd & 0x20)
        pos = 5 + (0 if single else 1) + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
        out = []
        while True:
            bh = int.from_bytes(frame[pos:pos + 3], "little")
            t, size = (bh >> 1) & 3, bh >> 3
            out.append(t)
            pos += 3 + (1 if t == 1 else size)
            if bh & 1:
                return out
    for flags in (0, SC.REPCODES):
        assert block_types(SC.expected(by[("rle-second", flags)])) == [2, 1]
        assert block_types(SC.expected(by[("rle-first", flags)])) == [2, 2]                      # the frame's first block is never RLE
        assert block_types(SC.expected(by[("rle-second-third", flags)])) == [2, 1, 1]
        assert block_types(SC.expected(by[("run-as-literals-second", flags)])) == [2, 2]         # ZSTD_maybeRLE looks at the sequence store, not at the bytes
        assert block_types(SC.expected(by[("tiny-first-then-run", flags)])) == [0, 2, 1]         # a raw block under 7 bytes leaves "first block" open
        assert block_types(SC.expected(by[("raw-second", flags)])) == [2, 0, 2]
    assert SC.expected(by[("raw-second", 0)]) != SC.expected(by[("raw-second", SC.REPCODES)])
    for name, flags, want in (("block-131073", 0, -107), ("offset-one-too-far", 0, -107), ("offset-one-too-far/rep", SC.REPCODES, -107), ("ml3-minmatch4", 0, -107),
                              ("ml2", 0, -107), ("ml2/L-5", SC.REPCODES, -107), ("offset-too-far-is-no-repcode", 0, -107)):
        assert SC.expected(by[(name, flags)]) == want, name
    for name, flags in (("offset-reaches-before-source", 0), ("offset-reaches-before-source/rep", SC.REPCODES), ("offset-too-far-is-a-repcode", SC.REPCODES)):
        frame = SC.expected(by[(name, flags)])
        assert isinstance(frame, bytes), name                                                    # accepted ...
        with pytest.raises(oracle_ref.ZstdRefError):                                             # ... and no decoder takes it
            oracle_ref.decompress(frame, 400)


def test_emu_sequences_batch_frames_and_refusals(emu, oracle_ref):
    cases = SC.batch()
    refused = 0
    for c in cases:
        got = run(emu, c)
        SC.check(c, got, oracle_ref)
        refused += got == -SC.E_SEQUENCES
        assert isinstance(got, bytes) == c.decodes, c.name
    assert refused == sum(not c.decodes for c in cases) == 18                # every tenth frame, but the two whose damage lies behind the last block


def test_emu_sequences_mixed_skipped_and_served(emu, oracle_ref):
    """the answers of the lists tests/test_gpu_sequences.py puts into one call each: served frames are the reference's, a source just over 128 KiB at level 5 has no
    row here (201) though the reference writes a frame, and a slot without a slice of the array (its offsets descend) is externalSequences_invalid"""
    for cases in SC.mixed_level5():
        skipped = [c for c in cases if c.name.startswith(SC.SKIPPED)]
        assert 2 <= len(skipped) <= 3 and len(cases) - len(skipped) == 36
        assert run(emu, skipped[0]) == -201 and isinstance(SC.expected(skipped[0]), bytes) and len(skipped[0].data) > 131072
        for c in cases:
            if not c.name.startswith(SC.SKIPPED):
                SC.check(c, run(emu, c), oracle_ref)
    emu.emu_compress_no_frame.restype = C.c_ulonglong
    emu.emu_compress_no_frame.argtypes = [C.c_char_p, C.c_uint, C.c_void_p, C.c_uint, C.c_int, C.c_uint]
    for at in (0, 1, 20):
        cases = SC.mixed_descending(at)
        rows, seq_off = SC.descending_rows(cases, at)
        for i, c in enumerate(cases):
            if i == at:
                dst = C.create_string_buffer(256)
                assert emu.emu_compress_no_frame(c.data, len(c.data), dst, 256, c.level, c.flags) == (1 << 64) - SC.E_SEQUENCES
            else:
                assert rows[seq_off[i]:seq_off[i + 1]] == c.seqs               # the slice the call gives the frame is the array the reference is asked about
                SC.check(c, run(emu, c), oracle_ref)


def test_emu_sequences_every_capacity(emu, oracle_ref):
    for c in SC.tight():
        full = SC.expected(c)
        assert isinstance(full, bytes)
        seen = set()
        for cap in range(0, len(full) + 33):
            got = run(emu, c, cap)
            if cap < SC.HEADER_ROOM:
                assert got == -SC.E_DST, (c.name, cap, got)
            else:
                SC.check(c, got, oracle_ref, cap)
            seen.add(got if isinstance(got, int) else "frame")
        assert seen == {-SC.E_DST, "frame"}, (c.name, seen)


def test_emu_sequence_bound(emu, oracle_ref):
    R = SC._lib()
    for n in (0, 1, 1023, 131072, 2 << 20):
        assert emu.emu_sequence_bound(n) == R.ZSTD_sequenceBound(n)
