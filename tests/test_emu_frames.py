"""CPU (-m "not gpu"): the arithmetic of the frames layer (zstd-jni_amd/csrc/zj_frames.h), built lane-serial from tests/emu_frames/emu_frames.cpp.

Frame-parallel decompress: the count walk and the emit walk of zjni_decompress_frames_batch_device over tests/inspect_cases.py's buffers plus crafted ones.  A buffer
is split exactly when (a) it is at most 2^32 - 1 bytes, (b) the walk meets no error, (c) every zstd frame records a content size, (d) there are at least two zstd
frames — expected here from zjni_inspect's frames / flags / bound, which tests/test_inspect.py pins to the reference.  Entry sources are checked against a walk
with the reference's ZSTD_findFrameCompressedSize, entry destinations against a prefix sum of its ZSTD_getFrameContentSize clamped at the slot's end.

Chunked compress: piece counts, piece offsets and scratch destinations of zjni_compress_chunked_batch_device, whole and cut into slices, and
zjni_compressBound_chunked.  The -m gpu twin is tests/test_gpu_frames.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from util import emu_so

import inspect_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU = (1 << 64) - 1
U64P = C.POINTER(C.c_ulonglong)


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_frames", "libzjni_emu_frames.so"))
    L.emu_frames_count.restype = C.c_ulonglong
    L.emu_frames_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p]
    L.emu_frames_emit.restype = None
    L.emu_frames_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
    L.emu_chunks_count.restype = C.c_ulonglong
    L.emu_chunks_count.argtypes = [C.c_void_p, C.c_uint, C.c_ulonglong, C.c_void_p, C.c_void_p]
    L.emu_chunks_emit.restype = None
    L.emu_chunks_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_ulonglong, C.c_void_p, C.c_void_p]
    L.emu_chunk_bound_total.restype = C.c_ulonglong
    L.emu_chunk_bound_total.argtypes = [C.c_ulonglong, C.c_ulonglong]
    return L


def crafted(ref):
    """the buffers the frames layer is about, by name"""
    text = b"large buffers are many frames laid end to end. " * 30
    F = lambda k, **kw: ic.Piece(ref.compress(text[k:k + 300 + 7 * k], 1 + (k & 1) * 2, checksum=bool(k & 2), **kw), text[k:k + 300 + 7 * k])      # noqa: E731
    S = lambda payload, v=3: ic.Piece(ic.skippable(payload, v), b"", kind="s")        # noqa: E731
    empty = ic.Piece(ref.compress(b"", 3), b"")
    nosize = ic.Piece(ref.compress(text[:500], 3, content_size=False), text[:500], nosize=True)
    out = [ic.join("two", [F(0), F(1)]),
           ic.join("forty", [F(k) for k in range(40)]),
           ic.join("skip_first", [S(b"index"), F(2), F(3)]),
           ic.join("skip_middle", [F(2), S(b""), F(3)]),
           ic.join("skip_last", [F(2), F(3), S(b"trailer", 15)]),
           ic.join("skip_and_one_frame", [S(b"a"), F(4), S(b"b")]),          # one zstd frame only: not split
           ic.join("content_zero", [F(5), empty, empty, F(6)]),
           ic.join("empty_twice", [empty, empty]),
           ic.join("one_without_size", [F(7), nosize, F(8)]),
           ic.join("truncated_tail", [F(9), F(10)], tail=F(11).z[:-5]),
           ic.join("bad_second_magic", [F(12)], tail=b"\x29\xB5\x2F\xFD" + F(13).z[4:]),
           ic.join("three_then_stray_byte", [F(1), F(2), F(3)], tail=b"\x00")]
    return out


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    R = ic.setup_ref(oracle_ref)
    R.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    R.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    cases, _ = ic.build_cases(oracle_ref)
    cases = crafted(oracle_ref) + cases
    L = zj.lib()
    for c in cases:
        fi = ic.host_info(L, c.data)
        c.split = len(c.data) <= 0xFFFFFFFF and fi.bound != ic.ERROR and not (fi.flags & ic.NOSIZE) and fi.frames >= 2
        c.entries = []                          # (offset in the buffer, content size) of every frame, by the reference
        if c.split:
            pos = 0
            while pos < len(c.data):
                b = ic.exact(c.data[pos:])
                size = R.ZSTD_findFrameCompressedSize(b, len(c.data) - pos)
                assert size <= len(c.data) - pos, c.name
                c.entries.append((pos, R.ZSTD_getFrameContentSize(b, len(c.data) - pos)))
                pos += size
            assert len(c.entries) == fi.frames + fi.skippable
    by_name = {c.name: c for c in cases}
    for nm in ("two", "forty", "skip_first", "skip_middle", "skip_last", "content_zero", "empty_twice", "forty_tiny_frames", "frame_frame", "skip_between", "sum_overflows"):
        assert by_name[nm].split, nm
    for nm in ("skip_and_one_frame", "one_without_size", "truncated_tail", "bad_second_magic", "three_then_stray_byte", "one", "empty_buffer", "stream", "frame_stream_frame",
               "skip_alone", "frame_cut_in_block"):
        assert not by_name[nm].split, nm
    assert len(by_name["forty"].entries) == 40 and len(by_name["skip_last"].entries) == 3
    return cases


def arr(values):
    return np.array(values, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("capacity", ("exact", "one_short", "generous"))
def test_split_rule_and_entry_arrays(emu, world, capacity):
    cases = world
    n = len(cases)
    blob = b"\xAA" + b"".join(c.data for c in cases)                     # the batch begins at byte 1
    src = np.frombuffer(blob, dtype=np.uint8)
    off = arr(np.cumsum([1] + [len(c.data) for c in cases]))
    caps = []
    for c in cases:
        total = min(sum(min(fcs, MAXU) for _, fcs in c.entries), 1 << 40) if c.split else 1000
        caps.append(total if capacity == "exact" else max(total - 1, 0) if capacity == "one_short" else total + 1000)
    dst_off = arr(np.cumsum([7] + caps, dtype=np.uint64))
    first = np.zeros(n + 1, dtype=np.uint64)
    E = emu.emu_frames_count(ptr(src), ptr(off), n, ptr(first))
    want_first = np.cumsum([0] + [len(c.entries) if c.split else 1 for c in cases])
    assert [int(x) for x in first] == [int(x) for x in want_first]
    assert E == int(want_first[-1]) and sum(c.split for c in cases) > 10
    src_e, dst_e = np.full(E + 1, 0xDEAD, dtype=np.uint64), np.full(E + 1, 0xDEAD, dtype=np.uint64)
    emu.emu_frames_emit(ptr(src), ptr(off), ptr(dst_off), ptr(first), n, ptr(src_e), ptr(dst_e))
    for i, c in enumerate(cases):
        lo, dlo, cap, e0 = int(off[i]), int(dst_off[i]), caps[i], int(first[i])
        if not c.split:
            assert (int(src_e[e0]), int(dst_e[e0])) == (lo, dlo), c.name
            continue
        run = 0
        for k, (pos, fcs) in enumerate(c.entries):
            assert int(src_e[e0 + k]) == lo + pos, (c.name, k)
            assert int(dst_e[e0 + k]) == dlo + min(run, cap), (c.name, k, capacity)
            run = min(run + fcs, MAXU)
    assert int(src_e[E]) == int(off[n]) and int(dst_e[E]) == int(dst_off[n])
    # every entry's extent is the next entry's beginning: interior slots are exactly the content size while the buffer fits
    c = cases[[x.name for x in cases].index("forty")]
    i = cases.index(c)
    if capacity != "one_short":
        for k, (pos, fcs) in enumerate(c.entries[:-1]):
            assert int(dst_e[int(first[i]) + k + 1]) - int(dst_e[int(first[i]) + k]) == fcs


def test_a_buffer_beyond_32_bits_is_not_split(emu):
    """(a): the walk is not even started — the source pointer is never read"""
    off = arr([0, 1 << 32])
    first = np.zeros(2, dtype=np.uint64)
    assert emu.emu_frames_count(None, ptr(off), 1, ptr(first)) == 1


@pytest.mark.parametrize("chunk", (256, 1000, 131072))
def test_chunk_arithmetic(emu, zj, chunk):
    L = zj.lib()
    sizes = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    n = len(sizes)
    off = arr(np.cumsum([3] + sizes))
    first, bbase = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    E = emu.emu_chunks_count(ptr(off), n, chunk, ptr(first), ptr(bbase))
    counts = [1, 1, 1, 1, 2, 4]
    assert E == sum(counts) and [int(x) for x in first] == [int(x) for x in np.cumsum([0] + counts)]
    want_src, want_dst, run = [], [], 0
    for i, s in enumerate(sizes):
        pieces = [min(chunk, s - k * chunk) for k in range(counts[i])] if s else [0]
        assert sum(pieces) == s
        total = sum(L.zjni_compressBound(p) for p in pieces)
        assert L.zjni_compressBound_chunked(s, chunk) == total == emu.emu_chunk_bound_total(s, chunk)
        assert int(bbase[i]) == run
        at = int(off[i])
        for p in pieces:
            want_src.append(at)
            want_dst.append(run)
            at += p
            run += L.zjni_compressBound(p)
    want_src.append(int(off[n]))
    want_dst.append(run)
    assert int(bbase[n]) == run
    for S in (E, 4, 3, 1):                                   # the whole batch, and slices that begin inside a buffer
        for a in range(0, E, S):
            m = min(S, E - a)
            src_s, dst_s = np.full(m + 1, 0xDEAD, dtype=np.uint64), np.full(m + 1, 0xDEAD, dtype=np.uint64)
            emu.emu_chunks_emit(ptr(off), ptr(first), ptr(bbase), n, chunk, a, m, E, ptr(src_s), ptr(dst_s))
            assert [int(x) for x in src_s] == want_src[a:a + m + 1], (S, a)
            assert [int(x) for x in dst_s] == [d - want_dst[a] for d in want_dst[a:a + m + 1]], (S, a)


def test_chunk_size_range(zj):
    L = zj.lib()
    for bad in (0, 255, 131073, 1 << 20):
        r = L.zjni_compressBound_chunked(1000, bad)
        assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 42, bad
    assert L.zjni_compressBound_chunked(0, 256) == L.zjni_compressBound(0)
    assert L.zjni_compressBound_chunked(1 << 30, 1 << 16) == (1 << 14) * L.zjni_compressBound(1 << 16)


def test_skippable_frame_sizes_are_taken_from_the_header(emu):
    """two empty-input frames around a skippable frame with a payload: three entries, all of content size 0"""
    f = struct.pack("<IBB", 0xFD2FB528, 0x20, 0) + b"\x01\x00\x00"
    buf = f + ic.skippable(b"1234567") + f
    src = np.frombuffer(buf, dtype=np.uint8)
    off, dst_off = arr([0, len(buf)]), arr([100, 100])
    first = np.zeros(2, dtype=np.uint64)
    assert emu.emu_frames_count(ptr(src), ptr(off), 1, ptr(first)) == 3
    s, d = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    emu.emu_frames_emit(ptr(src), ptr(off), ptr(dst_off), ptr(first), 1, ptr(s), ptr(d))
    assert [int(x) for x in s] == [0, len(f), len(f) + 15, len(buf)] and [int(x) for x in d] == [100] * 4
