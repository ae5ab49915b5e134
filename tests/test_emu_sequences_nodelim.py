"""CPU (-m "not gpu"): frames from the caller's sequences without block delimiters (ZJNI_SEQ_NO_DELIMITERS), the lane-serial build of the prefix, cut and emit
passes and the frame loop's no-delimiter instantiation (tests/emu_sequences_nodelim/).  Every case of tests/sequences_nodelim_cases.py must answer what the
reference's ZSTD_compressSequences answers with ZSTD_sf_noBlockDelimiters — the frame byte for byte, or its error code — and where the reference made a decodable
frame, that frame decodes to the source.  The emulation's workgroup state is poisoned once and outlives every frame; source, sequence array, prefix words, slots
and destination are exact-size heap blocks.  The -m gpu twin is tests/test_gpu_sequences_nodelim.py."""
import ctypes as C
import os

import pytest

from util import emu_so

import sequences_nodelim_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_sequences_nodelim", "libzjni_emu_sequences_nodelim.so"))
    L.emu_compress_sequences_nodelim.restype = C.c_ulonglong
    L.emu_compress_sequences_nodelim.argtypes = [C.c_char_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_int, C.c_uint, C.POINTER(C.c_uint)]
    L.emu_nodelim_max_blocks.restype = C.c_uint
    L.emu_nodelim_max_blocks.argtypes = [C.c_uint]
    return L


def run(emu, c, cap=None, flags=None, blocks=None):
    """the emulation's answer for a case: bytes or -code"""
    words = NC.flat(c.seqs)
    arr = (C.c_uint32 * max(len(words), 1))(*words)
    if cap is None:
        cap = len(c.data) + (len(c.data) >> 8) + 128 + 3 * (2 * (len(c.data) >> 17) + 8)
    dst = C.create_string_buffer(max(cap, 1))
    nb = C.c_uint(0)
    r = emu.emu_compress_sequences_nodelim(c.data, len(c.data), arr, len(c.seqs), dst, cap, c.level, c.flags if flags is None else flags, C.byref(nb))
    if blocks is not None:
        blocks.append(nb.value)
    if r >= 1 << 63:
        return -((1 << 64) - r)
    assert r <= cap
    return dst.raw[:r]


@pytest.mark.parametrize("group", ("tile_edges", "no_sequences", "merged_parse", "runs", "invalid_and_odd"))
def test_emu_nodelim_every_case_is_the_references_answer(emu, oracle_ref, group):
    cases = getattr(NC, group)()
    assert len(cases) >= 18
    for c in cases:
        blocks = []
        NC.check(c, run(emu, c, blocks=blocks), oracle_ref)
        assert blocks[0] <= emu.emu_nodelim_max_blocks(len(c.data)), c.name         # the bound the scratch is sized by


def test_emu_nodelim_cases_are_what_they_claim(oracle_ref):
    """the reference on the cases themselves: a match was split, a block was shortened, the minMatch-driven adjustment differs by level, and what is refused"""
    by = {(c.name, c.flags): c for c in NC.every_case()}
    B = NC.BLOCK

    def blocks(name, level):
        frame = NC.expected(by[(f"{name}/L{level}", NC.NO_DELIMITERS)])
        assert isinstance(frame, bytes), (name, level, frame)
        return NC.blocks_of(frame)
    for level in (1, 3):
        four = blocks("run-400000", level)                                                      # one sequence, four blocks: the match was split three times
        assert [b[0] for b in four] == [2, 1, 1, 1] and [b[1] for b in four[1:]] == [B, B, 400000 - 3 * B]
    by.update({(c.name, c.flags): c for c, _ in NC.level5()})
    for name, n in (("run-512KiB", 4), ("run-1MiB", 8)):
        one, three = blocks(name, 1), blocks(name, 3)
        assert len(one) == len(three) == n and [b[0] for b in one[1:]] == [1] * (n - 1)
        assert one[-1][1:] == (131066, 1) and three[-1][1:] == (131068, 1)                      # the second half would be under minMatch (7 and 5): the edge moves back
    for level in NC.LEVELS:
        four = blocks("run-starts-4-before-edge", level)                                        # first half under minMatch: the block is shortened, the run opens the next
        assert len(four) == 4 and four[1][:2] == (1, B) and four[3] == (0, 2, 1)
        eight = blocks("run-starts-8-before-edge", level)                                       # first half over minMatch: split at the edge
        assert len(eight) == 3 and eight[1][:2] == (1, B)
        assert [b[:2] for b in blocks("run-ends-2-behind-edge", level)][1][0] == 1
        assert len(blocks("match-131072-straddles", level)) == 3                                # 1 000 bytes, the match alone, 500 bytes: not split
        assert len(blocks("match-100000-straddles", level)) == 2
        assert len(blocks("literals-280000", level)) == 3
        assert blocks("rle-second-block", level)[1] == (1, 3000, 1)
        assert blocks("last-block-5-bytes", level)[1] == (0, 5, 1)
        assert blocks("covers-more/402", level) == [(0, 8, 1)]                                   # fewer bytes than the header says
        assert blocks("zero-sequences/300000", level)[-1][2] == 1 and len(blocks("zero-sequences/300000", level)) == 3
        assert blocks("last-bit-twice", level) == [(0, 5, 1)]                                    # ... and a second block with the bit behind it
        assert len(NC.expected(by[(f"last-bit-twice/L{level}", NC.NO_DELIMITERS)])) > 6 + 3 + 5 + 3
        for name, want in (("ml2", -107), ("offset-one-too-far", -107), ("stuck", -70)):
            assert NC.expected(by[(f"{name}/L{level}", NC.NO_DELIMITERS)]) == want, name
        for name in ("offset0-ll0", "offset0-ll5", "offset-reaches"):
            frame = NC.expected(by[(f"{name}/L{level}", NC.NO_DELIMITERS)])
            assert isinstance(frame, bytes), name                                                # accepted ...
            if level > 0:                                                                        # (level -5 leaves its literals raw and the block comes out raw)
                with pytest.raises(oracle_ref.ZstdRefError):                                     # ... and no decoder takes it
                    oracle_ref.decompress(frame, 408)
    for size, count in zip(NC.MERGED_SIZES, (1, 1, 2, 3, 4)):
        for level in NC.LEVELS:
            assert len(blocks(f"merged/{size}", level)) == count
    # the reference ignores ZSTD_c_searchForExternalRepcodes in this mode
    for c in NC.merged_parse()[:6] + NC.runs()[:6]:
        assert NC.ref_compress_nodelim(c.data, c.seqs, c.level, c.flags & NC.CHECKSUM, repcodes=False) == NC.expected(c), c.name


def test_emu_nodelim_repcodes_flag_changes_nothing(emu, oracle_ref):
    for c in NC.tile_edges()[::5] + NC.merged_parse()[::7] + NC.runs()[::9]:
        assert run(emu, c, flags=c.flags | NC.REPCODES) == run(emu, c) == NC.expected(c), c.name


def test_emu_nodelim_wrapping_lengths_answer_107(emu):
    for c in NC.wrapping():
        assert NC.undefined_in_reference(c.seqs, len(c.data))
        assert run(emu, c) == -NC.E_SEQUENCES, c.name


def test_emu_nodelim_level5(emu, oracle_ref):
    for c, served in NC.level5():
        got = run(emu, c)
        if served:
            NC.check(c, got, oracle_ref)
        else:
            assert got == -201 and isinstance(NC.expected(c), bytes), (c.name, got)


def test_emu_nodelim_batch_frames_and_refusals(emu, oracle_ref):
    cases = NC.batch()
    refused = 0
    for c in cases:
        got = run(emu, c)
        NC.check(c, got, oracle_ref)
        refused += got == -NC.E_SEQUENCES
    assert 5 <= refused <= 20


def test_emu_nodelim_every_capacity(emu, oracle_ref):
    for c in NC.tight():
        full = NC.expected(c)
        assert isinstance(full, bytes)
        seen = set()
        for cap in range(0, len(full) + 33):
            got = run(emu, c, cap)
            if cap < NC.HEADER_ROOM:
                assert got == -NC.E_DST, (c.name, cap, got)
            else:
                NC.check(c, got, oracle_ref, cap)
            seen.add(got if isinstance(got, int) else "frame")
        assert seen == {-NC.E_DST, "frame"}, (c.name, seen)


def test_emu_nodelim_random_arrays(emu, oracle_ref):
    cases = NC.random_arrays()
    assert len(cases) == 300
    kinds = set()
    for c in cases:
        got = run(emu, c)
        NC.check(c, got, oracle_ref)
        kinds.add(got if isinstance(got, int) else "frame")
    assert {"frame", -NC.E_SEQUENCES} <= kinds
