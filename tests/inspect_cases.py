"""Inputs shared by tests/test_inspect.py (host walk) and tests/test_gpu_inspect.py (device walk): buffers of concatenated zstd and
skippable frames, whole, truncated and damaged, with what the test knows about them by construction, and the reference's four
header-only calls through ctypes."""
import ctypes as C
import glob
import os
import random
import struct

from conftest import GOLDEN, golden
from util import json_records

UNKNOWN, ERROR = (1 << 64) - 1, (1 << 64) - 2
CHECKSUM, NOSIZE, SINGLE = 1, 2, 4            # ZJNI_INFO_*


class Case:
    """data: the buffer.  orig: what it decodes to (None: not known / not valid).  counts: (frames, skippable, flags) when the test
    knows them by construction, else None.  dict: the frames need the test dictionary.  bad: malformed or truncated on purpose."""

    def __init__(self, name, data, orig=None, counts=None, dict=False, bad=False):
        self.name, self.data, self.orig, self.counts, self.dict, self.bad = name, bytes(data), orig, counts, dict, bad


def exact(z):
    """an exact-size copy (the sanitizer build, tests/inspect_host.cpp, makes its own malloc copy of it: small ctypes copies live where no sanitizer looks)"""
    return (C.c_ubyte * len(z)).from_buffer_copy(z) if z else None


def setup_ref(ref):
    R = ref.lib()
    R.ZSTD_findDecompressedSize.restype = C.c_ulonglong
    R.ZSTD_findDecompressedSize.argtypes = [C.c_void_p, C.c_size_t]
    R.ZSTD_decompressBound.restype = C.c_ulonglong
    R.ZSTD_decompressBound.argtypes = [C.c_void_p, C.c_size_t]
    R.ZSTD_findFrameCompressedSize.restype = C.c_size_t
    R.ZSTD_findFrameCompressedSize.argtypes = [C.c_void_p, C.c_size_t]
    R.ZSTD_getDictID_fromFrame.restype = C.c_uint
    R.ZSTD_getDictID_fromFrame.argtypes = [C.c_void_p, C.c_size_t]
    return R


def ref_info(R, z):
    """(content, bound, firstFrameSize, dictID) as the reference answers them"""
    b = exact(z)
    return (R.ZSTD_findDecompressedSize(b, len(z)), R.ZSTD_decompressBound(b, len(z)),
            R.ZSTD_findFrameCompressedSize(b, len(z)), R.ZSTD_getDictID_fromFrame(b, len(z)))


class FrameInfo(C.Structure):
    """zjni_frame_info (include/zjni_amd.h)"""
    _fields_ = [("content", C.c_uint64), ("bound", C.c_uint64), ("firstFrameSize", C.c_uint64),
                ("dictID", C.c_uint32), ("frames", C.c_uint32), ("skippable", C.c_uint32), ("flags", C.c_uint32)]


def host_info(L, z):
    """zjni_inspect of the library L (the product library, or the walk alone under a sanitizer) on an exact-size copy"""
    fi = FrameInfo()
    L.zjni_inspect.restype = C.c_size_t
    L.zjni_inspect.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.zjni_inspect(exact(z), len(z), C.byref(fi)) == 0
    return fi


def skippable(payload, variant=3):
    return struct.pack("<II", 0x184D2A50 + variant, len(payload)) + payload


class Piece:
    def __init__(self, z, orig, kind="z", checksum=False, nosize=False):
        self.z, self.orig, self.kind, self.checksum, self.nosize = z, orig, kind, checksum, nosize


def join(name, pieces, tail=b"", dict=False):
    """complete pieces one after the other, then `tail` (stray bytes or a cut frame: the first malformed spot)"""
    frames = sum(p.kind == "z" for p in pieces)
    skips = sum(p.kind == "s" for p in pieces)
    flags = (CHECKSUM if any(p.checksum for p in pieces) else 0) | (NOSIZE if any(p.nosize for p in pieces) else 0)
    if not tail and frames == 1 and skips == 0:
        flags |= SINGLE
    data = b"".join(p.z for p in pieces) + tail
    orig = None if tail or any(p.orig is None for p in pieces) else b"".join(p.orig for p in pieces)
    return Case(name, data, orig, (frames, skips, flags), dict=dict, bad=bool(tail))


_dictionary = None


def dictionary(ref):
    global _dictionary
    if _dictionary is None:
        recs = json_records(2000, seed=5)
        _dictionary = ref.train_dict(recs[:1500], 4096)
    return _dictionary


def stream_data(size):
    """compressible bytes (JSON-like records)"""
    out, first = [], 0
    while sum(map(len, out)) < size + len(out):
        out += json_records(2000, seed=3, first=first)
        first += 2000
    return b",".join(out)[:size]


def build_cases(ref, with_goldens=True, n_random=3000):
    rnd = random.Random(20)
    cases = []
    small = golden("xmlsmall-sized.zst")
    text = b"the quick brown fox jumps over the lazy dog. " * 40
    one = ref.compress(text, 3)
    one_ck = ref.compress(text[:700], 1, checksum=True)
    empty = ref.compress(b"", 3)
    nosz = ref.compress(text[:900], 3, content_size=False)
    sdata = stream_data(300000)
    stream = ref.compress_stream(sdata, 3, chunk=20000, flush_every=1)        # window descriptor, no content size, many blocks
    stream_ck = ref.compress_stream(text * 3, 1, checksum=True, chunk=1000, flush_every=2)
    d = dictionary(ref)
    recs = json_records(40, seed=11)
    drec = b",".join(recs[:20])
    dframe = ref.compress_using_dict(drec, d, 3)
    P_one, P_ck, P_empty = Piece(one, text), Piece(one_ck, text[:700], checksum=True), Piece(empty, b"")
    P_nosz, P_stream = Piece(nosz, text[:900], nosize=True), Piece(stream, sdata, nosize=True)
    P_stream_ck = Piece(stream_ck, text * 3, checksum=True, nosize=True)
    P_small = Piece(small, None)
    P_dict = Piece(dframe, drec)
    S = lambda payload, v=3: Piece(skippable(payload, v), b"", kind="s")        # noqa: E731

    # ---- whole frames and concatenations
    for nm, p in (("one", P_one), ("checksum", P_ck), ("empty", P_empty), ("nosize", P_nosz), ("stream", P_stream), ("stream_ck", P_stream_ck)):
        cases.append(join(nm, [p]))
    cases.append(join("dict", [P_dict], dict=True))
    cases.append(join("dict_twice_and_plain", [P_dict, S(b"x"), P_dict], dict=True))
    cases.append(join("frame_frame", [P_one, P_ck]))
    cases.append(join("frame_stream_frame", [P_one, P_stream, P_empty]))
    cases.append(join("skip_before", [S(b"hello"), P_one]))
    cases.append(join("skip_between", [P_one, S(b""), P_ck]))
    cases.append(join("skip_after", [P_nosz, S(b"12345678", 15)]))
    cases.append(join("skip_everywhere", [S(b"a", 0), P_one, S(b"bc", 7), P_nosz, S(b"def", 15)]))
    cases.append(join("skip_alone", [S(b"payload", 15)]))
    cases.append(join("skip_alone_empty", [S(b"", 0)]))
    for k in (1, 4, 5):
        cases.append(join("stray_%d" % k, [P_one], tail=b"\x00" * k))
        cases.append(join("stray_magic_%d" % k, [P_ck, S(b"zz")], tail=struct.pack("<I", 0xFD2FB528)[:k] + b"\x24"[:max(0, k - 4)]))
    cases.append(join("skip_short_by_one", [], tail=skippable(b"payload", 15)[:-1]))
    cases.append(join("frame_then_skip_short", [P_one], tail=skippable(b"payload")[:-1]))
    cases.append(join("skip_header_cut", [P_one], tail=skippable(b"payload")[:6]))
    cases.append(join("skip_size_wraps", [], tail=struct.pack("<II", 0x184D2A5F, 0xFFFFFFFC) + b"abcd"))
    cases.append(join("skip_size_wraps_after_frame", [P_one], tail=struct.pack("<II", 0x184D2A51, 0xFFFFFFF8) + b"abcd"))
    cases.append(join("empty_buffer", []))
    tiny = [Piece(ref.compress(bytes([65 + k]) * (k + 1), 1, checksum=bool(k & 1)), bytes([65 + k]) * (k + 1), checksum=bool(k & 1)) for k in range(40)]
    cases.append(join("forty_tiny_frames", tiny))
    cases.append(join("frame_cut_in_block", [P_one], tail=one_ck[:-7]))
    cases.append(join("stream_cut", [], tail=stream[:len(stream) // 2]))
    # a content size field of 8 bytes: two frames whose declared sizes overflow 64 bits when summed, and the two sentinel values as sizes
    for nm, vals in (("sum_overflows", (1 << 63, 1 << 63)), ("declares_unknown", (UNKNOWN,)), ("declares_error", (ERROR,)), ("declares_2_60", (1 << 60,))):
        z = b"".join(struct.pack("<IBQ", 0xFD2FB528, 0xE0, v) + b"\x01\x00\x00" for v in vals)
        cases.append(Case(nm, z, bad=True))
    valid = [c for c in cases if not c.bad]

    # ---- every prefix of the small golden frame
    cases.append(join("xmlsmall", [P_small]))
    for k in range(len(small)):
        cases.append(Case("xmlsmall[:%d]" % k, small[:k], bad=True))
    # ---- every single-bit flip in the first 16 bytes of a one-shot frame and of a stream frame
    stream_small = ref.compress_stream(sdata[:6000], 3, chunk=1000, flush_every=1)
    for nm, z in (("xmlsmall", small), ("stream", stream_small), ("dict", dframe)):
        for bit in range(128):
            zb = bytearray(z)
            zb[bit >> 3] ^= 1 << (bit & 7)
            cases.append(Case("%s^bit%d" % (nm, bit), zb, bad=True))
    # ---- seeded random overwrites and cuts (the style of test_abi.py::test_frame_content_size_on_damaged_headers)
    base = [ref.compress(bytes(rnd.randrange(5) for _ in range(k)), 3, checksum=bool(k & 1)) for k in (0, 1, 100, 255, 256, 300, 70000)]
    base += [skippable(b"hello"), ref.compress_stream(b"abc" * 1000, 3), one + one_ck, skippable(b"") + nosz, dframe, stream_ck]
    for it in range(n_random):
        z = bytearray(rnd.choice(base))
        for _ in range(rnd.randrange(0, 3)):
            z[rnd.randrange(0, min(len(z), 24))] = rnd.getrandbits(8)
        r = rnd.random()
        if r < 0.4:
            z = z[:rnd.randrange(0, min(len(z), 24) + 1)]
        elif r < 0.6:
            z = z[:rnd.randrange(0, len(z) + 1)]
        elif r < 0.7:
            z += bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(1, 9)))
        cases.append(Case("random%d" % it, z, bad=True))
    # ---- the stored frames
    if with_goldens:
        for path in sorted(glob.glob(os.path.join(GOLDEN, "*.zst")) + glob.glob(os.path.join(GOLDEN, "corrupt", "*.zst"))):
            with open(path, "rb") as f:
                cases.append(Case("golden:" + os.path.relpath(path, GOLDEN), f.read(), bad="corrupt" in path))
    return cases, valid


if __name__ == "__main__":
    # inspect_cases.py <library exporting zjni_inspect>: every case against the reference (tests/test_inspect.py runs this under AddressSanitizer)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import ref as _ref
    _L, _R = C.CDLL(sys.argv[1]), setup_ref(_ref)
    _cases, _ = build_cases(_ref)
    _bad = 0
    for _c in _cases:
        _fi = host_info(_L, _c.data)
        _bad += (_fi.content, _fi.bound, _fi.firstFrameSize, _fi.dictID) != ref_info(_R, _c.data)
    print("cases=%d mismatches=%d" % (len(_cases), _bad))
