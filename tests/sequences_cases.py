"""Frames from the caller's sequences (zjni_compress_sequences*, zstd-jni_amd/csrc/zj_sequences.h): the cases tests/test_emu_sequences.py (CPU, the
lane-serial build) and tests/test_gpu_sequences.py (GPU) both run, and the oracle they compare with — the reference's own ZSTD_compressSequences,
called over ctypes on oracle/_ref/libzstd_ref.so.  A case is a source, a ZSTD_Sequence array with explicit block delimiters, a level and a flag
word; what the reference answers for it (a frame, or an error code) is what the entries must answer, byte for byte.
TEST INFRASTRUCTURE."""
import ctypes as C
import random
from collections import namedtuple

from util import json_records

CHECKSUM, REPCODES = 1, 8                      # ZJNI_FRAME_CHECKSUM, ZJNI_SEQ_REPCODES
E_SEQUENCES, E_DST = 107, 70                   # ZSTD_error_externalSequences_invalid, ZSTD_error_dstSize_tooSmall
# ZSTD_writeFrameHeader wants ZSTD_FRAMEHEADERSIZE_MAX bytes and ZSTD_compressSequences adds its answer to the output pointer unchecked
# (N/compress/zstd_compress.c:7077-7081): below 18 bytes the reference is not defined (it crashes), so it is never asked; the entries answer
# dstSize_tooSmall there, which the capacity walks assert directly
HEADER_ROOM = 18

Case = namedtuple("Case", "name data seqs level flags decodes")        # seqs: [(offset, litLength, matchLength, rep)]; decodes: the reference's frame decodes to data


class _Seq(C.Structure):
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


def _lib():
    from oracle import ref
    L = ref.lib()
    L.ZSTD_compressSequences.restype = C.c_size_t
    L.ZSTD_compressSequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(_Seq), C.c_size_t, C.c_void_p, C.c_size_t]
    L.ZSTD_generateSequences.restype = C.c_size_t
    L.ZSTD_generateSequences.argtypes = [C.c_void_p, C.POINTER(_Seq), C.c_size_t, C.c_void_p, C.c_size_t]
    L.ZSTD_sequenceBound.restype = C.c_size_t
    L.ZSTD_sequenceBound.argtypes = [C.c_size_t]
    return L


def _array(seqs):
    arr = (_Seq * max(len(seqs), 1))()
    for i, s in enumerate(seqs):
        arr[i].offset, arr[i].litLength, arr[i].matchLength, arr[i].rep = s
    return arr


def flat(seqs):
    """the array as the C entries take it: 4 uint32 per sequence"""
    return [v for s in seqs for v in s]


def ref_compress_sequences(data, seqs, level, checksum, repcodes, cap=None):
    """ZSTD_compressSequences on a fresh CCtx: the frame (bytes), or -code"""
    from oracle import ref
    L = _lib()
    cctx = L.ZSTD_createCCtx()
    try:
        for p, v in ((100, level), (201, int(bool(checksum))), (1008, 1), (1009, 1), (1016, 1 if repcodes else 2)):
            ref._check(L.ZSTD_CCtx_setParameter(cctx, p, v))
        if cap is None:
            cap = L.ZSTD_compressBound(len(data)) + 64 + 3 * (len(seqs) + 1)
        dst = C.create_string_buffer(max(cap, 1))
        r = L.ZSTD_compressSequences(cctx, dst, cap, _array(seqs), len(seqs), bytes(data), len(data))
        if L.ZSTD_isError(r):
            return -((1 << 64) - r)
        return dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)


def ref_generate_sequences(data, level):
    """ZSTD_generateSequences with explicit block delimiters: the reference's own parse of `data` at `level`"""
    from oracle import ref
    L = _lib()
    cctx = L.ZSTD_createCCtx()
    try:
        ref._check(L.ZSTD_CCtx_setParameter(cctx, 100, level))
        ref._check(L.ZSTD_CCtx_setParameter(cctx, 1008, 1))
        cap = L.ZSTD_sequenceBound(len(data))
        arr = (_Seq * cap)()
        n = ref._check(L.ZSTD_generateSequences(cctx, arr, cap, bytes(data), len(data)))
        return [(arr[i].offset, arr[i].litLength, arr[i].matchLength, arr[i].rep) for i in range(n)]
    finally:
        L.ZSTD_freeCCtx(cctx)


_expected = {}


def expected(c, cap=None):
    key = (c.name, c.level, c.flags, cap)
    if key not in _expected:
        _expected[key] = ref_compress_sequences(c.data, c.seqs, c.level, c.flags & CHECKSUM, c.flags & REPCODES, cap)
    return _expected[key]


def check(c, got, ref, cap=None):
    """got: bytes or -code, from either implementation"""
    want = expected(c, cap)
    if isinstance(want, int) or isinstance(got, int):
        assert got == want, (c.name, c.level, c.flags, cap, got if isinstance(got, int) else len(got), want if isinstance(want, int) else len(want))
        return
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert got == want, (c.name, c.level, c.flags, cap, len(got), len(want), at)
    if c.decodes and cap is None:
        assert ref.decompress(want, len(c.data)) == c.data, c.name


# ---- sources ----
_TEXT = bytes(b"etaoinsh"[b & 7] for b in range(256))


def literals(rnd, n, kind):
    if kind == "rle":
        return b"e" * n
    raw = rnd.randbytes(n)
    return raw if kind == "raw" else raw.translate(_TEXT)


def make(blocks, seed=1):
    """blocks = [([(ll, ml, offset), ...], trailing literals, literal kind)] -> (data, seqs): the content the triples mean (as tests/seqframes.py builds it)
    and the array with a delimiter behind every block"""
    rnd = random.Random(seed)
    out, seqs = bytearray(), []
    for triples, tail, kind in blocks:
        for ll, ml, off in triples:
            out += literals(rnd, ll, kind)
            assert 1 <= off <= len(out)
            seqs.append((off, ll, ml, 0))
            while ml:
                n = min(ml, off)
                s = len(out) - off
                out += out[s:s + n]
                ml -= n
        out += literals(rnd, tail, kind)
        seqs.append((0, tail, 0, 0))
    return bytes(out), seqs


def prose(n, seed=1):
    """the JSON-like records of the dictionary tests, n bytes of them"""
    recs, out = json_records(n // 60 + 8, seed), bytearray()
    for r in recs:
        out += r + b"\n"
    assert len(out) >= n
    return bytes(out[:n])


def generated(data, level, chunk=None):
    """the reference's parse of `data`; chunk: each piece parsed on its own, so that the caller's blocks are the pieces"""
    if chunk is None:
        return ref_generate_sequences(data, level)
    seqs = []
    for at in range(0, len(data), chunk):
        seqs += ref_generate_sequences(data[at:at + chunk], level)
    return seqs


ALL_FLAGS = (0, CHECKSUM, REPCODES, CHECKSUM | REPCODES)
_cases = {}


def _memo(key, fn):
    if key not in _cases:
        _cases[key] = fn()
    return _cases[key]


def smallest():
    def build():
        out = [Case("empty", b"", [], 3, 0, True), Case("empty/checksum", b"", [], 3, CHECKSUM, True), Case("empty/delimiter", b"", [(0, 0, 0, 0)], 1, 0, True),
               Case("lone6", b"abcdef", [(0, 6, 0, 0)], 3, 0, True), Case("lone7", b"abcdefg", [(0, 7, 0, 0)], 3, CHECKSUM, True)]
        for k in (1, 63, 64, 65, 129):                       # tile edges of the conversion and the carry between tiles
            data, seqs = make([([(3 + i % 2, 4 + i % 3, 1 + i % 3) for i in range(k)], 5, "text")], seed=k)
            for flags in (0, REPCODES):
                out.append(Case(f"one-block/{k}", data, seqs, 3, flags, True))
        data, seqs = make([([(9, 6, 2), (4, 5, 7)], 0, "text")])               # a delimiter with litLength 0 directly behind a match
        out += [Case("delimiter-ll0", data, seqs, 3, 0, True), Case("delimiter-ll0/rep", data, seqs, 1, REPCODES, True)]
        return out
    return _memo("smallest", build)


def from_generator():
    def build():
        out = []
        for size in (4096, 65536):
            data = prose(size, seed=size)
            for level in (1, 3, 5, -5):
                seqs = generated(data, level)
                for flags in ALL_FLAGS:
                    out.append(Case(f"generated/{size}/L{level}", data, seqs, level, flags, True))
        return out
    return _memo("generated", build)


def multi_block():
    def build():
        out = []
        text = prose(15000, seed=3)
        for level in (1, 3):
            out.append(Case("three-text-blocks", text, generated(text, level, 5000), level, CHECKSUM, True))
            out.append(Case("three-text-blocks/rep", text, generated(text, level, 5000), level, REPCODES, True))
        run = [([(1, 2999, 1)], 0, "rle")]                    # a run as one literal and one match: ZSTD_maybeRLE holds
        first = [([(30, 8, 3), (12, 40, 17), (25, 9, 5)], 2000, "text")]
        for flags in (0, REPCODES):
            for name, blocks in (("rle-second", first + run), ("rle-first", run + first), ("rle-second-third", first + run + run),
                                 ("run-as-literals-second", first + [([], 3000, "rle")]),                           # 3 000 literals: not ZSTD_maybeRLE, a compressed block of RLE literals
                                 ("run-short-second", first + [([(1, 8, 1)], 0, "rle")]), ("tiny-first-then-run", [([], 5, "text")] + run + run)):
                data, seqs = make(blocks, seed=7)
                out.append(Case(name, data, seqs, 3, flags, True))
            # raw second block WITH a sequence of its own: its history must not be confirmed; block three's offsets are block one's last three
            blocks = [([(40, 8, 11), (20, 9, 23), (31, 7, 37)], 1500, "text"), ([(3000, 4, 100)], 50, "raw"),
                      ([(10, 12, 37), (9, 8, 23), (0, 9, 11), (14, 6, 100), (7, 8, 36)], 900, "text")]
            data, seqs = make(blocks, seed=11)
            out.append(Case("raw-second", data, seqs, 3, flags, True))
            out.append(Case("raw-second/L1", data, seqs, 1, flags, True))
            # one, two, three and more sequences a block (zstd_compress.c:6704-6717), each block's offsets met again in the next
            blocks = [([(50, 8, 9)], 300, "text"), ([(20, 7, 9), (30, 9, 13)], 300, "text"), ([(10, 6, 13), (12, 9, 9), (22, 8, 21)], 300, "text"),
                      ([(5, 7, 21), (0, 8, 9), (9, 9, 13), (11, 6, 4), (3, 8, 21)], 300, "text"), ([(16, 9, 4)], 200, "text")]
            data, seqs = make(blocks, seed=13)
            out.append(Case("history-branches", data, seqs, 3, flags, True))
        big = prose(131073, seed=5)
        out.append(Case("block-131072", big[:131072], generated(big[:131072], 3), 3, CHECKSUM, True))
        out.append(Case("block-131073", big, [(0, 131073, 0, 0)], 3, 0, False))
        out.append(Case("two-blocks-131073", big, generated(big[:131072], 3) + [(0, 1, 0, 0)], 3, REPCODES, True))
        return out
    return _memo("multi", build)


def long_codes():
    def build():
        out = []
        data, seqs = make([([(70000, 4, 1)], 0, "text"), ([(1, 70000, 1)], 5, "text")], seed=17)
        out += [Case("ll70000-ml70000", data, seqs, 3, 0, True), Case("ll70000-ml70000/rep", data, seqs, 1, CHECKSUM | REPCODES, True)]
        # offsets just below the window: level 3 at 200 000 bytes has windowLog 18
        data, seqs = make([([], 100000, "text"), ([], 99000, "text"), ([(10, 100, 199009), (5, 40, 199100), (0, 30, 199000)], 100, "text")], seed=19)
        out += [Case("far-offsets", data, seqs, 3, flags, True) for flags in (0, REPCODES)]
        body = literals(random.Random(23), 400, "text")              # eight letters: the block is emitted compressed, so the offset is in the frame
        # the bound is the position BEHIND the sequence: 4 literals + 8 match bytes end at 12
        out.append(Case("offset-reaches-before-source", body, [(12, 4, 8, 0), (0, 388, 0, 0)], 3, 0, False))
        out.append(Case("offset-reaches-before-source/rep", body, [(12, 4, 8, 0), (0, 388, 0, 0)], 3, REPCODES, False))
        out.append(Case("offset-one-too-far", body, [(13, 4, 8, 0), (0, 388, 0, 0)], 3, 0, False))
        out.append(Case("offset-one-too-far/rep", body, [(13, 4, 8, 0), (0, 388, 0, 0)], 3, REPCODES, False))
        out.append(Case("offset-too-far-is-a-repcode", body, [(8, 1, 4, 0), (0, 395, 0, 0)], 3, REPCODES, False))         # 8 = rep[2]: beyond no bound once it is a repcode
        out.append(Case("offset-too-far-is-no-repcode", body, [(8, 1, 4, 0), (0, 395, 0, 0)], 3, 0, False))
        out.append(Case("ml3-minmatch4", body, [(2, 4, 3, 0), (0, 393, 0, 0)], 3, 0, False))
        out.append(Case("ml2", body, [(2, 4, 2, 0), (0, 394, 0, 0)], 1, 0, False))
        out.append(Case("ml2/L-5", body, [(2, 4, 2, 0), (0, 394, 0, 0)], -5, REPCODES, False))
        return out
    return _memo("long", build)


DAMAGE = ("ml2", "offset", "no-last-delimiter", "past-source", "offset0-with-match", "short-of-source", "block-past-source", "second-block-bad", "ll-huge", "garbage-after-end")


def damaged(seqs, size, kind):
    """one way of breaking a valid array (its last entry is the closing delimiter of a source of `size` bytes)"""
    s = [list(q) for q in seqs]
    first = next(i for i, q in enumerate(s) if q[0] != 0)
    if kind == "ml2": s[first][1] += s[first][2] - 2; s[first][2] = 2
    elif kind == "offset": s[first][0] = s[first][1] + s[first][2] + 1
    elif kind == "no-last-delimiter": s = s[:-1]
    elif kind == "past-source": s[-1][1] += 1
    elif kind == "offset0-with-match": s[first][0] = 0
    elif kind == "short-of-source": s[max(i for i, q in enumerate(s) if q[1] > 0)][1] -= 1                     # the blocks end a byte before the source does
    elif kind == "block-past-source": s[first][1] += size
    elif kind == "second-block-bad": s = s + [[5, 1, 2, 0], [0, 0, 0, 0]]; s[len(seqs) - 1][1] -= 3            # a good first block, then a match of 2
    elif kind == "ll-huge": s[first][1] = 200000
    elif kind == "garbage-after-end": s = s + [[0xFFFFFFFF, 0xFFFFFFFF, 1, 7], [0, 9, 9, 9]]                  # behind the last block: never looked at
    return [tuple(q) for q in s]


def batch(n=200, seed=29):
    """n frames of 1-8 KiB at level 3, every tenth damaged in one of DAMAGE's ways ("garbage-after-end" keeps its frame valid)"""
    def build():
        rnd = random.Random(seed)
        out = []
        for i in range(n):
            size = rnd.randrange(1024, 8193)
            data = prose(size, seed=1000 + i)
            seqs = generated(data, 3, chunk=rnd.choice((None, 3000)))
            name = f"batch/{i}"
            if i % 10 == 5:
                kind = DAMAGE[(i // 10) % len(DAMAGE)]
                if kind == "second-block-bad" and seqs[-1][1] < 3:
                    kind = "ml2"
                seqs = damaged(seqs, size, kind)
                name += "/" + kind
            out.append(Case(name, data, seqs, 3, rnd.choice(ALL_FLAGS), i % 10 != 5 or name.endswith("garbage-after-end")))
        return out
    return _memo(("batch", n, seed), build)


def tight():
    """three small frames for the walk over every capacity: several text blocks with a checksum; RLE and raw blocks behind a compressed one; tiny blocks"""
    def build():
        text = prose(1800, seed=31)
        a = Case("tight/text-blocks", text, generated(text, 3, 600), 3, CHECKSUM, True)
        data, seqs = make([([(30, 8, 3), (12, 40, 17)], 200, "text"), ([(1, 299, 1)], 0, "rle"), ([(100, 4, 50)], 20, "raw"), ([(10, 9, 17)], 120, "text")], seed=37)
        b = Case("tight/rle-raw", data, seqs, 3, REPCODES, True)
        data, seqs = make([([], 3, "text"), ([(4, 5, 2)], 40, "text"), ([], 0, "text"), ([], 6, "text"), ([(8, 30, 3)], 2, "text")], seed=41)
        c = Case("tight/tiny-blocks", data, seqs, 1, CHECKSUM | REPCODES, True)
        return [a, b, c]
    return _memo("tight", build)


SKIPPED = "skipped/"                            # a case's name begins so: the conversion kernel writes the slot's word itself and converts nothing


def mixed_level5():
    """two lists for ONE call each at level 5: 36 served frames of 1-4 KiB and, between them, the same source just over 128 KiB — the level has no row for it, the
    conversion skips the frame (block count 0) and the frame loop answers 201.  The skipped frame sits at indices 0, middle and last of the first list, at 1 and
    the middle of the second; the caller runs both orders, so that a workgroup meets a skipped frame and then served ones (zj_seq_convert_kernel's one lane-0 store)."""
    def build():
        big = prose(131073 + 2000, seed=43)
        skipped = Case(SKIPPED + "level5/133073", big, generated(big, 5), 5, REPCODES, True)
        served = []
        for i in range(36):
            data = prose(1024 + 83 * i, seed=4300 + i)
            served.append(Case(f"mixed5/{i}", data, generated(data, 5), 5, REPCODES, True))
        a = [skipped] + served[:18] + [skipped] + served[18:] + [skipped]
        b = served[:1] + [skipped] + served[1:20] + [skipped] + served[20:]
        return [a, b]
    return _memo("mixed5", build)


def mixed_descending(at, n=40):
    """n frames of 1-4 KiB at level 3 for ONE call in which frame `at`'s pair of sequence offsets descends by one row (run_descending below lays the rows out): the
    frame loop answers 107 for that slot alone (zs_compress_frame: ZS_NO_FRAME -> externalSequences_invalid).  The frame in front of it then owns one row more — the
    first row of the frame behind, which lies behind its closing delimiter and is never looked at; its case says so, so the reference is asked the same."""
    def build():
        out = []
        for i in range(n):
            data = prose(1024 + 71 * i, seed=4700 + i)
            out.append(Case(f"descend{at}/{i}", data, generated(data, 3), 3, 0, True))
        out[at] = out[at]._replace(name=SKIPPED + f"descend{at}/{at}", decodes=False)
        if at > 0:
            out[at - 1] = out[at - 1]._replace(seqs=out[at - 1].seqs + [out[at + 1].seqs[0]])
        return out
    return _memo(("descending", at, n), build)


def descending_rows(cases, at):
    """(rows, seq_off) of a call for mixed_descending(at): frame `at` has no rows of its own and the pair (seq_off[at], seq_off[at + 1]) = (B + 1, B), B the first
    row of frame at + 1; every other pair ascends"""
    rows, seq_off = [], []
    for i, c in enumerate(cases):
        if i == at:
            seq_off.append(len(rows) + 1)
            continue
        seq_off.append(len(rows))
        rows += c.seqs[:-1] if i == at - 1 else c.seqs
    seq_off.append(len(rows))
    if at > 0:
        assert cases[at - 1].seqs[-1] == cases[at + 1].seqs[0] and seq_off[at - 1] + len(cases[at - 1].seqs) == seq_off[at]
    assert [i for i in range(len(cases)) if seq_off[i] > seq_off[i + 1]] == [at] and seq_off[at] - seq_off[at + 1] == 1
    return rows, seq_off


def every_case():
    return smallest() + from_generator() + multi_block() + long_codes()


def other_levels():
    """caller-cut blocks at the other served levels: [(case, served)].  Not served (201, the caller falls back): a second block where the level's row for the size
    is lazy or lazy2 — level 5 to 16 KiB, levels 6 to 8 — because those strategies weigh the previous block's sequence tables (zstd_compress_sequences.c:196-222)"""
    def build():
        out = []
        for size, level, served in ((15000, 4, True), (20000, 4, True), (15000, 5, False), (20000, 5, True), (100000, 5, True), (20000, 6, False), (15000, 7, False),
                                    (15000, -3, True), (200000, -3, True), (200000, 2, True), (4000, 8, True)):
            data = prose(size, seed=size + level)
            chunk = None if size == 4000 else (5000 if size <= 20000 else 50000)              # (4 000 bytes at level 8: one block, lazy2 — served)
            out.append((Case(f"levels/{size}/L{level}", data, generated(data, level, chunk), level, REPCODES if level != 2 else CHECKSUM, True), served))
        return out
    return _memo("levels", build)
