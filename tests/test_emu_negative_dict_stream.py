"""CPU (-m "not gpu"): compression dictionaries and stream frames at negative levels (zstd's --fast=N), through the encoder bodies built lane-serial from
tests/emu_negdict/emu_negdict.cpp.  A CDict of level -N: row 0 of the table its size picks, targetLength = N (levels below -131072 clamped), the fast
digest; its frames byte-identical to the reference's ZSTD_createCDict(dict, -N) + ZSTD_CCtx_refCDict + ZSTD_compress2 (oracle/ref.py CDict.compress) in
attach mode (sources up to 8 KiB: the dictMatchState loop steps N), in copy mode (up to one block: the extDict loop steps N + 1), with raw literals and
the dictionary's sequence tables; 40 where the reference re-derives the parameters, 201 above one block.  Streams at -N: what ZSTD_compressStream2 writes
without a pledged size (oracle/ref.py compress_stream) up to the 512 KiB window.  The -m gpu twin is tests/test_gpu_negative_dict_stream.py."""
import ctypes as C
import os
import random

import pytest

from conftest import golden
from util import json_records, emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [-1, -2, -3, -7, -50, -1000, -131072, -200000]
ZE_FLAG_CHECKSUM, ZE_FLAG_NO_FCS, ZE_FLAG_NO_DICTID = 1, 2, 4
SOURCE_SIZES = [0, 1, 7, 8, 100, 8191, 8192, 8193, 16384, 65536, 131071, 131072]


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_negdict", "libzjni_emu_negdict.so"))
    L.emu_nd_level_word.restype = C.c_uint
    L.emu_nd_level_word.argtypes = [C.c_int]
    L.emu_nd_cdict_create.restype = C.c_void_p
    L.emu_nd_cdict_create.argtypes = [C.c_char_p, C.c_uint, C.c_int]
    L.emu_nd_cdict_free.argtypes = [C.c_void_p]
    L.emu_nd_cdict_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    L.emu_nd_compress_cdict.restype = C.c_ulonglong
    L.emu_nd_compress_cdict.argtypes = [C.c_void_p, C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_uint, C.POINTER(C.c_int)]
    L.emu_nd_compress_stream.restype = C.c_ulonglong
    L.emu_nd_compress_stream.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_uint, C.c_int, C.c_int]
    return L


def _res(r, dst):
    return -((1 << 64) - r) if r >= (1 << 63) else dst.raw[:r]


class NegCDict:
    def __init__(self, L, dictionary, level):
        self.L = L
        self.ptr = L.emu_nd_cdict_create(dictionary, len(dictionary), level)

    def info(self):
        out = (C.c_uint * 10)()
        self.L.emu_nd_cdict_info(self.ptr, out)
        keys = ("dictID", "contentSize", "windowLog", "chainLog", "hashLog", "minMatch", "strategy", "word", "attachStep", "copyStep")
        return dict(zip(keys, out[:]))

    def compress(self, data, checksum=False, dict_id=True, content_size=True, cap=None):
        if cap is None:
            cap = len(data) + (len(data) >> 7) + 256
        dst = C.create_string_buffer(max(cap, 1) + 8)
        flags = (ZE_FLAG_CHECKSUM if checksum else 0) | (0 if dict_id else ZE_FLAG_NO_DICTID) | (0 if content_size else ZE_FLAG_NO_FCS)
        route = C.c_int(-1)
        r = self.L.emu_nd_compress_cdict(self.ptr, data, len(data), dst, cap, flags, C.byref(route))
        return _res(r, dst), route.value

    def __del__(self):
        if self.ptr:
            self.L.emu_nd_cdict_free(self.ptr)
            self.ptr = None


def text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"\"id\":", b"\"name\":", b"compress", b"level", b"\n", b"{", b"}"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


@pytest.fixture(scope="module")
def dictionaries(oracle_ref):
    """a trained dictionary of 110 KiB (BASELINE config 4's size) and one of ~16 KiB, raw content of ~2 KiB, an 8-byte one, and raw content on either side
    of the rSize = size + 499 row limits (16 / 128 / 256 KiB)"""
    rnd = random.Random(41)
    recs = json_records(30000, seed=3)
    samples = [b",".join(recs[i * 13:i * 13 + 200])[:4096] for i in range(1500)] + [text(rnd, 4096) for _ in range(200)]
    out = [("trained110k", oracle_ref.train_dict(samples, 112640)), ("trained16k", oracle_ref.train_dict(samples, 16000)),
           ("raw2k", b",".join(recs[:40])[:2048]), ("eight", b"abcdefgh")]
    blob = b",".join(recs[100:8000])
    for n in (16384 - 499, 16384 - 498, 131072 - 499, 131072 - 498, 262144 - 499, 262144 - 498):
        out.append(("raw%d" % n, blob[:n]))
    return out, recs


def sources(recs, rnd, extra=6):
    sizes = SOURCE_SIZES + [rnd.randrange(0, 131073) for _ in range(extra)] + [rnd.randrange(0, 8193) for _ in range(extra)]
    out = []
    for size in sizes:
        k = rnd.randrange(0, len(recs) - 3000)
        out.append(b",".join(recs[k:k + 3000])[:size])
        if size <= 16384:
            out.append(text(rnd, size))
    return out


def test_level_word_and_row0_digest(emu, oracle_ref, dictionaries):
    """the CDict's parameters: row 0 of the dictionary size's table after the unknown-size adjustment, the acceleration in its word, the two steps"""
    dicts, _ = dictionaries
    assert emu.emu_nd_level_word(-200000) == emu.emu_nd_level_word(-131072)
    assert emu.emu_nd_level_word(-3) & 0xFF == 1 and emu.emu_nd_level_word(2) == 2
    # by hand from clevels.h row 0 and ZSTD_adjustCParams_internal (unknown source size: 513 bytes + the dictionary)
    want = {"raw2k": (12, 12, 13, 5), "raw15885": (14, 12, 13, 5), "raw15886": (15, 12, 12, 5), "trained110k": (17, 12, 12, 5),
            "raw130573": (17, 12, 12, 5), "raw130574": (18, 12, 13, 5), "raw261645": (18, 12, 13, 5), "raw261646": (19, 12, 13, 6)}
    for name, d in dicts:
        for level in (-1, -5, -200000):
            cd = NegCDict(emu, d, level)
            assert cd.ptr, (name, level)
            info = cd.info()
            assert info["strategy"] == 1, (name, level)
            n = min(-level, 131072)
            assert (info["attachStep"], info["copyStep"]) == (min(n, 131071), min(n, 131071) + 1), (name, level, info)
            if name in want:
                assert (info["windowLog"], info["chainLog"], info["hashLog"], info["minMatch"]) == want[name], (name, info)
    assert not NegCDict(emu, b"abcdefg", -1).ptr              # under 8 bytes: no CDict
    assert not NegCDict(emu, dicts[0][1], 4).ptr               # dictionaries at levels 4-8 stay the bundled library's


@pytest.mark.parametrize("level", LEVELS)
def test_negative_cdict_frames(emu, oracle_ref, dictionaries, level):
    dicts, recs = dictionaries
    rnd = random.Random(1000 - level)
    routes = set()
    for name, d in dicts:
        ref = oracle_ref.CDict(d, level)
        cd = NegCDict(emu, d, level)
        content = cd.info()["contentSize"]
        for i, x in enumerate(sources(recs, rnd, extra=2)):
            ck, did = bool(i & 1), not (i % 3 == 2)
            got, route = cd.compress(x, ck, did)
            if len(x) > 131072:
                assert got == -201
                continue
            if len(x) == 131072 and len(x) >= 6 * content:
                assert got == -40 and route == 0, (name, level, len(x))       # the reference re-derives the parameters from the source there
                continue
            want = ref.compress(x, ck, did)
            assert got == want, (name, level, len(x), ck, did, route)
            assert route == (1 if len(x) <= 8192 else 2)
            routes.add(route)
            assert oracle_ref.decompress_using_dict(got, d, len(x)) == x
        got, _ = cd.compress(bytes(131073))
        assert got == -201                                                 # more than one block with a dictionary
        got, _ = cd.compress(b"x" * 100, content_size=False)
        assert got == -40                                                  # no content size with a dictionary: as at levels 1-3
    assert routes == {1, 2}


def test_negative_cdict_tight_destinations(emu, oracle_ref, dictionaries):
    dicts, recs = dictionaries
    d = dicts[0][1]
    for level in (-1, -4):
        ref = oracle_ref.CDict(d, level)
        cd = NegCDict(emu, d, level)
        for x in (b"", b"a", b",".join(recs[5:12])[:700], b",".join(recs[50:200])[:6000], b",".join(recs[300:900])[:20000]):
            full = ref.compress(x)
            for cap in sorted(set(list(range(max(0, len(full) - 3), len(full) + 8)) + [0, 8, 18, len(x) + 3, len(x) + 12])):
                try:
                    want = ref.compress(x, cap=cap)
                except oracle_ref.ZstdRefError as e:
                    want = -e.code
                assert cd.compress(x, cap=cap)[0] == want, (level, len(x), cap)


def _stream(emu, d, level, ck=False, flush_at=(), final=True, known_empty=None):
    if known_empty is None:
        known_empty = final and not d and not flush_at
    cap = len(d) + (len(d) >> 8) + 4096 + 64 * (len(flush_at) + 2)
    dst = C.create_string_buffer(cap)
    arr = (C.c_uint * max(len(flush_at), 1))(*flush_at)
    r = emu.emu_nd_compress_stream(d, len(d), dst, cap, level, 1 if ck else 0, arr, len(flush_at), 1 if final else 0, 1 if known_empty else 0)
    return _res(r, dst)


def stream_inputs(oracle_ref, zj, size, rnd):
    xml = oracle_ref.decompress(golden("xml-1.zst"), 6_000_000)
    o = rnd.randrange(0, len(xml) - size - 1)
    return [xml[o:o + size], b"".join(zj.synth_host(65536, i, 1) for i in range(size // 65536 + 1))[:size]]


def test_negative_stream_frames(emu, oracle_ref, zj):
    rnd = random.Random(23)
    n = 0
    for size in (0, 1, 7, 100, 8192, 131071, 131072, 131073, 200000, 262143, 262144, 262145, 393216, 393217, 524287, 524288):
        for d in stream_inputs(oracle_ref, zj, size, rnd):
            for level in (-1, -3, -7, -50, -131072, -200000):
                ck = bool(n & 1); n += 1
                for chunk in ((50000, 131072) if n % 3 == 0 else (131072,)):
                    got = _stream(emu, d, level, ck)
                    assert got == oracle_ref.compress_stream(d, level, ck, chunk=chunk), (size, level, ck, chunk)
                assert oracle_ref.decompress(got, len(d)) == d
    for level in (-1, -5):
        assert _stream(emu, bytes(524289), level) == -201                  # beyond the 512 KiB window: the bundled library's stream


def test_negative_stream_flushes_and_not_final(emu, oracle_ref, zj):
    rnd = random.Random(29)
    n = 0
    for size in (1000, 50000, 200000, 300000, 524288):
        for d in stream_inputs(oracle_ref, zj, size, rnd):
            for level in (-1, -4):
                for chunk, k in ((50000, 1), (10000, 3), (131072, 1), (65536, 2), (1000, 7)):
                    calls = (size + chunk - 1) // chunk
                    flushes = [min(j * chunk, size) for j in range(1, calls + 1) if j % k == 0]
                    ck = bool(n & 1); n += 1
                    got = _stream(emu, d, level, ck, flushes)
                    assert got == oracle_ref.compress_stream(d, level, ck, chunk=chunk, flush_every=k), (size, level, chunk, k)
                    assert oracle_ref.decompress(got, len(d)) == d
                    if flushes and flushes[-1] < size:
                        # flushed, not closed: the frame's beginning up to the last flush, as the later close() writes it
                        part = _stream(emu, d, level, ck, flushes, final=False)
                        assert isinstance(part, bytes) and got[:len(part)] == part and len(part) < len(got), (size, level, chunk, k)
    # known-empty (closed before anything else) against a stream that was flushed empty first
    for level in (-1, -9):
        assert _stream(emu, b"", level) == oracle_ref.compress_stream(b"", level)
        assert _stream(emu, b"", level, final=False, known_empty=False) == b""
        assert _stream(emu, b"", level, flush_at=[0], known_empty=False) != _stream(emu, b"", level)
