"""CPU (-m "not gpu"): negative compression levels (zstd's --fast=N) through the encoder bodies, built lane-serial from
tests/emu_fast/emu_fast.cpp.  Every frame is byte-identical to the reference's ZSTD_compress2 with ZSTD_c_compressionLevel = L:
row 0 of the size's parameter table, stepSize = -L + 1 in the fast match loop, literals always raw, levels below
ZSTD_minCLevel() (-131072) clamped to it.  Both single-block routes (the fused kernel's one-lane parse with LDS tables, and the
lane-per-frame matcher ZLaneF ahead of the entropy stage) and the multi-block frame loop are checked.  The -m gpu twin is
tests/test_gpu_negative_levels.py."""
import ctypes as C
import os
import random

import pytest

from conftest import golden
from util import edge_inputs, emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [-1, -2, -3, -4, -5, -7, -17, -100, -65536, -131072, -200000]
ZE_FLAG_CHECKSUM, ZE_FLAG_NO_FCS = 1, 2


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_fast", "libzjni_emu_fast.so"))
    L.emu_fast_compress.restype = C.c_ulonglong
    L.emu_fast_compress.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_int, C.c_uint, C.c_int]
    L.emu_fast_params.argtypes = [C.c_int, C.c_uint, C.POINTER(C.c_uint)]
    L.emu_fast_level_word.restype = C.c_uint
    L.emu_fast_level_word.argtypes = [C.c_int]
    return L


def fast_compress(L, data, level, route=0, checksum=False, content_size=True, cap=None):
    if cap is None:
        cap = len(data) + (len(data) >> 8) + 64 + 128
    dst = C.create_string_buffer(max(cap, 1) + 8)
    flags = (ZE_FLAG_CHECKSUM if checksum else 0) | (0 if content_size else ZE_FLAG_NO_FCS)
    r = L.emu_fast_compress(data, len(data), dst, cap, level, flags, route)
    return -((1 << 64) - r) if r >= (1 << 63) else dst.raw[:r]


def text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"compress", b"level", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def inputs(zj):
    """the issue's set: empty, 1 byte, the 16 KiB / 64 KiB / 128 KiB edges, incompressible, RLE, periodic, text, text + noise"""
    rnd = random.Random(5)
    noise = lambda n: bytes(rnd.getrandbits(8) for _ in range(n))
    out = [("empty", b""), ("one", b"x"), ("rle", b"\x07" * 70000), ("periodic", (b"0123456789abcdefghij" * 7000)[:131072]),
           ("incompressible", noise(40000))]
    for n in (16384, 16385, 65536, 65537, 131072):
        out.append(("synth%d" % n, zj.synth_host(n, n, 1)))
    t = text(rnd, 131072)
    out.append(("text", t))
    tn = bytearray(t[:70000])
    for _ in range(3000):
        tn[rnd.randrange(len(tn))] = rnd.getrandbits(8)
    out.append(("text+noise", bytes(tn)))
    out.append(("xml", golden("xmlsmall")[:20000]))
    return out


def test_level_word_and_row0_parameters(emu):
    """row 0 of clevels.h after ZSTD_adjustCParams_internal; the acceleration clamped (-200000 -> -131072 -> the word's cap)"""
    out = (C.c_uint * 7)()
    for size, want in ((1000, (10, 10, 11, 5)), (16384, (14, 12, 13, 5)), (16385, (15, 12, 12, 5)), (131072, (17, 12, 12, 5)),
                       (200000, (18, 12, 13, 5)), (300000, (19, 12, 13, 6))):
        emu.emu_fast_params(-3, size, out)
        assert tuple(out[:4]) == want, (size, tuple(out[:4]))
        assert out[4] == 1 and out[5] == 3 and out[6] == 4
    emu.emu_fast_params(-1, 65536, out); assert (out[5], out[6]) == (1, 2)
    emu.emu_fast_params(1, 65536, out); assert (out[5], out[6]) == (0, 2)      # level 1 keeps step 2
    assert emu.emu_fast_level_word(-200000) == emu.emu_fast_level_word(-131072) == emu.emu_fast_level_word(-131071)
    assert emu.emu_fast_level_word(-5) & 0xFF == 1


@pytest.mark.parametrize("route", [0, 1])
def test_negative_levels_single_block(emu, oracle_ref, zj, route):
    for name, data in inputs(zj):
        for level in LEVELS:
            assert fast_compress(emu, data, level, route) == oracle_ref.compress(data, level), (name, level, route)


@pytest.mark.parametrize("route", [0, 1])
def test_negative_levels_edge_inputs_and_flags(emu, oracle_ref, route):
    for name, data in edge_inputs():
        for level in (-1, -2, -5, -33):
            for ck, cs in ((False, True), (True, True), (True, False)):
                want = oracle_ref.compress(data, level, ck, content_size=cs)
                assert fast_compress(emu, data, level, route, ck, cs) == want, (name, level, route, ck, cs)


def test_negative_levels_random_sizes(emu, oracle_ref, zj):
    rnd = random.Random(17)
    for _ in range(60):
        size = rnd.choice([rnd.randrange(0, 300), rnd.randrange(0, 5000), rnd.randrange(0, 70000), rnd.randrange(0, 131073), 65536, 4096])
        d = zj.synth_host(size, rnd.randrange(0, 100000), 1) if size else b""
        level = rnd.choice([-1, -2, -3, -6, -9, -40, -1000, -70000])
        for route in (0, 1):
            assert fast_compress(emu, d, level, route) == oracle_ref.compress(d, level), (size, level, route)


def test_negative_levels_multi_block(emu, oracle_ref, zj):
    """frames above one block, up to the window (512 KiB): the frame loop with the step carried into every block; beyond it: 201"""
    rnd = random.Random(3)
    t = text(rnd, 600000)
    cases = [("synth", zj.synth_host(524288, 9, 1)), ("text", t[:300000]), ("text256k+1", t[:262145]), ("rle", b"\x01" * 140000),
             ("incompressible", bytes(rnd.getrandbits(8) for _ in range(200000)))]
    for name, data in cases:
        for level in (-1, -3, -7, -100, -131072):
            for ck in (False, True):
                assert fast_compress(emu, data, level, checksum=ck) == oracle_ref.compress(data, level, ck), (name, level, ck)
    assert fast_compress(emu, t[:524289], -1) == -201


def test_negative_levels_tight_destinations(emu, oracle_ref, zj):
    """capacities around the frame's size: the reference's answer (bytes, a raw block instead, or dstSize_tooSmall) for every one"""
    rnd = random.Random(8)
    datas = [b"", b"a", b"abcdefg" * 3, bytes(rnd.randrange(4) for _ in range(120)), golden("xmlsmall")[:3000], zj.synth_host(9000, 5, 1),
             zj.synth_host(65536, 1, 1), b"\x07" * 5000, zj.synth_host(140000, 3, 1)]
    for data in datas:
        for level in (-1, -4):
            full = oracle_ref.compress(data, level)
            caps = list(range(max(0, len(full) - 2), len(full) + 20)) + [0, 8, 18, len(data), len(data) + 3, len(data) + 12]
            for cap in (caps if len(data) < 20000 else caps[::3]):
                try:
                    want = oracle_ref.compress(data, level, cap=cap)
                except oracle_ref.ZstdRefError as e:
                    want = -e.code
                for route in ((0, 1) if len(data) <= 131072 else (0,)):
                    assert fast_compress(emu, data, level, route, cap=cap) == want, (len(data), level, cap, route)
