"""Frames from the caller's sequences WITHOUT block delimiters (ZJNI_SEQ_NO_DELIMITERS, zstd-jni_amd/csrc/zj_sequences.h "no block delimiters"): the cases
tests/test_emu_sequences_nodelim.py (CPU, the lane-serial build) and tests/test_gpu_sequences_nodelim.py (GPU) both run, and the oracle they compare with — the
reference's own ZSTD_compressSequences with ZSTD_c_blockDelimiters = ZSTD_sf_noBlockDelimiters (parameter 1008 = 0) and ZSTD_c_validateSequences = 1, over ctypes on
oracle/_ref/libzstd_ref.so.  A case is a source, a ZSTD_Sequence array, a level and a flag word; what the reference answers (a frame, or an error code) is what the
entries must answer, byte for byte.  Helpers come from tests/sequences_cases.py.
TEST INFRASTRUCTURE."""
import ctypes as C
import random

import sequences_cases as SC
from sequences_cases import Case, CHECKSUM, REPCODES, E_SEQUENCES, E_DST, HEADER_ROOM, flat      # noqa: F401  (re-exported for the two test files)

NO_DELIMITERS = 16                              # ZJNI_SEQ_NO_DELIMITERS
LEVELS = (1, 3, -5)
BLOCK = 1 << 17


def ref_compress_nodelim(data, seqs, level, checksum, cap=None, repcodes=True):
    """ZSTD_compressSequences without block delimiters on a fresh CCtx: the frame (bytes), or -code"""
    from oracle import ref
    L = SC._lib()
    cctx = L.ZSTD_createCCtx()
    try:
        for p, v in ((100, level), (201, int(bool(checksum))), (1008, 0), (1009, 1), (1016, 1 if repcodes else 2)):
            ref._check(L.ZSTD_CCtx_setParameter(cctx, p, v))
        if cap is None:
            cap = L.ZSTD_compressBound(len(data)) + 64 + 3 * (2 * (len(data) >> 17) + 8)
        dst = C.create_string_buffer(max(cap, 1))
        r = L.ZSTD_compressSequences(cctx, dst, cap, SC._array(seqs), len(seqs), bytes(data), len(data))
        if L.ZSTD_isError(r):
            return -((1 << 64) - r)
        return dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)


def ref_merge(seqs):
    """ZSTD_mergeBlockDelimiters: the array without its delimiters, each one's literals added to the sequence behind it"""
    L = SC._lib()
    L.ZSTD_mergeBlockDelimiters.restype = C.c_size_t
    L.ZSTD_mergeBlockDelimiters.argtypes = [C.POINTER(SC._Seq), C.c_size_t]
    arr = SC._array(seqs)
    n = L.ZSTD_mergeBlockDelimiters(arr, len(seqs))
    return [(arr[i].offset, arr[i].litLength, arr[i].matchLength, arr[i].rep) for i in range(n)]


_expected = {}


def expected(c, cap=None):
    key = (c.name, c.level, c.flags & CHECKSUM, cap)
    if key not in _expected:
        _expected[key] = ref_compress_nodelim(c.data, c.seqs, c.level, c.flags & CHECKSUM, cap)
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


def blocks_of(frame):
    """[(type, regenerated size, last bit)] of every block up to the first with the last-block bit, of a frame without a dictionary ID"""
    fhd = frame[4]
    single = bool(fhd & 0x20)
    pos = 5 + (0 if single else 1) + ((1 if single else 0), 2, 4, 8)[fhd >> 6]
    out = []
    while True:
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        t, size = (bh >> 1) & 3, bh >> 3
        if t == 2:                                   # a compressed block's header holds its compressed size
            out.append((t, None, bh & 1))
        else:
            out.append((t, size, bh & 1))
        pos += 3 + (1 if t == 1 else size)
        if bh & 1:
            return out


def undefined_in_reference(seqs, size):
    """the two corners where the reference's transfer is not defined, so that it is never asked (zj_sequences.h, header): a reached sequence whose litLength +
    matchLength does not fit 32 bits, and a block that starts INSIDE a match with fewer than minMatch bytes of source left.  A model of the cut for every
    minMatch a served row has (3 to 7); True if any of them meets one.  An offset of 2^32 - 3 anywhere counts too: offset + 3 wraps to offBase 0, which the reference
    stores unchecked (the entries answer 107 for it, as with delimiters)."""
    if any(s[0] == 0xFFFFFFFD for s in seqs):
        return True
    for mm in (3, 4, 5, 6, 7):
        idx, sp, at = 0, 0, 0
        steps = 0
        while at < size:
            steps += 1
            if steps > 64:
                break                                # (stuck: the reference answers dstSize_tooSmall, which is defined)
            T = min(BLOCK, size - at)
            last = T == size - at
            end = sp + T                             # endPosInSequence
            start = sp
            consumed = T
            while end and idx < len(seqs):
                off, ll, ml, _ = seqs[idx]
                if ll + ml >= 1 << 32:
                    return True
                if end >= ll + ml:
                    end -= ll + ml
                    start = 0
                    idx += 1
                    continue
                if end > ll:
                    lt = 0 if start >= ll else ll - start
                    first = end - start - lt
                    if ml > T and first >= mm:
                        second = ml + ll - end
                        if second < mm:
                            end -= mm - second
                            consumed = T - (mm - second)
                    else:
                        if start > ll:
                            return True
                        consumed = T - (end - ll)
                        end = ll
                break
            sp = end
            at += consumed
            if consumed == 0 or (last and (consumed >= 7 or at == size)):
                break
    return False


# ---- cases ----
def nd(triples, tail, kind="text", seed=1):
    """(data, seqs): the content the (ll, ml, offset) triples mean, `tail` bytes behind them that no sequence covers, and the array without any delimiter"""
    data, seqs = SC.make([(triples, tail, kind)], seed=seed)
    return data, seqs[:-1]


def _each(name, data, seqs, decodes=True, levels=LEVELS):
    return [Case(f"{name}/L{level}", data, seqs, level, NO_DELIMITERS | flags, decodes) for level in levels for flags in (0, CHECKSUM)]


def tile_edges():
    def build():
        out = []
        for k in (1, 63, 64, 65, 129):               # tile edges of the prefix and emit passes and the carry between tiles
            data, seqs = nd([(3 + i % 2, 4 + i % 3, 1 + i % 3) for i in range(k)], 5, seed=k)
            out += _each(f"tile/{k}", data, seqs)
        return out
    return SC._memo("nd-tile", build)


def no_sequences():
    def build():
        out = []
        for size in (1, 7, 300000):
            out += _each(f"zero-sequences/{size}", SC.prose(size, seed=size + 2), [])
        return out
    return SC._memo("nd-zero", build)


MERGED_SIZES = (4096, 131072, 131079, 300000, 400000)


def merged_parse():
    """the reference's own parse (ZSTD_generateSequences, then ZSTD_mergeBlockDelimiters) at the case's level"""
    def build():
        out = []
        for size in MERGED_SIZES:
            data = SC.prose(size, seed=size + 1)
            for level in LEVELS:
                seqs = ref_merge(SC.generated(data, level))
                assert all(s[0] != 0 for s in seqs)
                out += _each(f"merged/{size}", data, seqs, levels=(level,))
        return out
    return SC._memo("nd-merged", build)


def runs():
    def build():
        out = []
        out += _each("run-400000", b"e" * 400000, [(1, 17, 399999, 0)], decodes=False)         # (16 bytes more than the source: the last block is a first half too)
        # a run one byte longer than its source: at the last edge the second half would be 1 byte, so the edge moves back by minMatch - 1 — 6 bytes at level 1
        # (minMatch 7), 4 at level 3 (minMatch 5) — and the frame ends short of its source.  1 MiB is beyond the window of levels 1 and -5 (unserved(), below)
        out += _each("run-512KiB", b"e" * (1 << 19), [(1, 2, (1 << 19) - 1, 0)], decodes=False)
        out += _each("run-1MiB", b"e" * (1 << 20), [(1, 2, (1 << 20) - 1, 0)], decodes=False, levels=(3,))
        for before in (4, 8):                        # the first half would be under / over every served minMatch (5 to 7 at these levels and sizes)
            # ... and the tail makes the difference countable: shortened, 2 * 128 KiB + 2 bytes are left behind the first block (three more blocks, the last of
            # 2 bytes); split, 2 * 128 KiB (two more)
            data, seqs = nd([(BLOCK - before, 200000, 1)], 2 * BLOCK - 200000 + (2 if before == 4 else 8), seed=before)
            out += _each(f"run-starts-{before}-before-edge", data, seqs)
        data, seqs = nd([(100, 2 * BLOCK + 2 - 100, 1)], 50, seed=3)             # the second half at the second edge would be 2 bytes
        out += _each("run-ends-2-behind-edge", data, seqs)
        data, seqs = nd([(1000, BLOCK, 7)], 500, seed=4)                           # matchLength == the block's target: not "larger than the block size"
        out += _each("match-131072-straddles", data, seqs)
        data, seqs = nd([(60000, 100000, 9)], 1000, seed=5)
        out += _each("match-100000-straddles", data, seqs)
        data, seqs = nd([(280000, 50, 3)], 100, seed=6)
        out += _each("literals-280000", data, seqs)
        data, seqs = nd([(10, 20, 3), (7, 9, 11)], 5000, seed=7)
        out += _each("covers-less", data, seqs)
        data, seqs = nd([(BLOCK + 1, 2999, 1)], 0, seed=8)                         # the second block is one literal and a run of it: ZSTD_maybeRLE and ZSTD_isRLE hold
        out += _each("rle-second-block", data, seqs)
        data, seqs = nd([(100, 50, 7)], BLOCK + 5 - 150, seed=9)
        out += _each("last-block-5-bytes", data, seqs)
        data, seqs = nd([(10, 20, 3), (5, 9, 4)], 0, seed=10)                      # what lies behind the end of the source is never read
        out += _each("garbage-behind-source", data, seqs + [(0xFFFFFFFF, 0xFFFFFFFF, 1, 7), (0, 9, 9, 9)])
        return out
    return SC._memo("nd-runs", build)


def invalid_and_odd():
    def build():
        out = []
        body = SC.literals(random.Random(23), 408, "text")
        out += _each("covers-more/402", body, [(4, 8, 402, 0)], decodes=False)     # shortened last block: one raw block of 8 bytes ends the frame
        out += _each("covers-more/5000", body, [(4, 8, 5000, 0)], decodes=False)
        out += _each("offset0-ll0", body, [(0, 0, 8, 0)], decodes=False)
        out += _each("offset0-ll5", body, [(0, 5, 8, 0)], decodes=False)
        out += _each("ml2", body, [(2, 4, 2, 0)], decodes=False)
        out += _each("offset-reaches", body, [(12, 4, 8, 0)], decodes=False)
        out += _each("offset-one-too-far", body, [(13, 4, 8, 0)], decodes=False)
        # the transfer's corners on tiny sources (zj_sequences.h, header): a shortened last block under 7 bytes is written with the last-block bit and the loop
        # goes on; with fewer than minMatch bytes left behind it nothing is consumed any more and the reference fills the destination with empty raw blocks
        # (20 bytes: the match of 20 behind 5 literals is no longer than the block's target, so the block ends in front of it, 5 bytes; the next block starts at
        # the match, whose first half is its whole target of 15 and whose second half is 5, not under any minMatch here)
        out += _each("last-bit-twice", body[:20], [(4, 5, 20, 0)], decodes=False)
        out += _each("stuck", body[:6], [(4, 3, 10, 0)], decodes=False)
        return out
    return SC._memo("nd-invalid", build)


def every_case():
    return tile_edges() + no_sequences() + merged_parse() + runs() + invalid_and_odd()


def wrapping():
    """litLength + matchLength beyond 32 bits: undefined in the reference, never asked; the entries answer 107"""
    body = SC.literals(random.Random(29), 400, "text")
    return [Case(f"wrapping/L{level}", body, seqs, level, NO_DELIMITERS | flags, False)
            for level in LEVELS for flags in (0, CHECKSUM)
            for seqs in ([(1, 0xFFFFFFF0, 0x20, 0)], [(3, 10, 8, 0), (1, 0x20, 0xFFFFFFF0, 0)], [(3, 0x80000000, 0x80000000, 0)])]


def level5():
    """[(case, served)]: level 5 is served to 128 KiB; above that the library has no row (201) while the reference gives a frame.  So with the 1 MiB run at
    levels 1 and -5, whose window is 512 KiB: a source beyond the row's window is not served, with or without delimiters."""
    def build():
        out = []
        for size, served in ((4096, True), (300000, False)):
            data = SC.prose(size, seed=size + 5)
            out.append((Case(f"level5/{size}", data, ref_merge(SC.generated(data, 5)), 5, NO_DELIMITERS, True), served))
        for level in (1, -5):
            out.append((Case(f"run-1MiB/L{level}", b"e" * (1 << 20), [(1, 2, (1 << 20) - 1, 0)], level, NO_DELIMITERS, False), False))
        return out
    return SC._memo("nd-level5", build)


ND_DAMAGE = ("ml2", "offset", "ll-grows", "ml-grows", "offset0", "drop-last", "garbage-after-end")


def batch(n=200, seed=31):
    """n frames of 1-8 KiB at level 3 from the reference's merged parse, every tenth damaged in one of ND_DAMAGE's ways (some of which leave a frame)"""
    def build():
        rnd = random.Random(seed)
        out = []
        for i in range(n):
            size = rnd.randrange(1024, 8193)
            data = SC.prose(size, seed=2000 + i)
            seqs = ref_merge(SC.generated(data, 3, chunk=rnd.choice((None, 3000))))
            name = f"nd-batch/{i}"
            good = True
            if i % 10 == 5:
                kind = ND_DAMAGE[(i // 10) % len(ND_DAMAGE)]
                s = [list(q) for q in seqs]
                if kind == "ml2": s[0][1] += s[0][2] - 2; s[0][2] = 2
                elif kind == "offset": s[0][0] = s[0][1] + s[0][2] + 1
                elif kind == "ll-grows": s[len(s) // 2][1] += 7
                elif kind == "ml-grows": s[len(s) // 2][2] += 9
                elif kind == "offset0": s[len(s) // 2][0] = 0
                elif kind == "drop-last": s = s[:-1]
                elif kind == "garbage-after-end": s += [[3, size, 4, 0], [0xFFFFFFFF, 0xFFFFFFFF, 1, 7]]
                seqs = [tuple(q) for q in s]
                assert not undefined_in_reference(seqs, size)
                name += "/" + kind
                good = kind in ("drop-last", "garbage-after-end")
            out.append(Case(name, data, seqs, 3, NO_DELIMITERS | rnd.choice(SC.ALL_FLAGS), good))
        return out
    return SC._memo(("nd-batch", n, seed), build)


def tight():
    """three short frames for the walk over every capacity: text with a checksum; a run and raw bytes behind text; literals only behind a short match"""
    def build():
        text = SC.prose(1800, seed=31)
        a = Case("nd-tight/text", text, ref_merge(SC.generated(text, 3, 600)), 3, NO_DELIMITERS | CHECKSUM, True)
        data, seqs = SC.make([([(30, 8, 3), (12, 40, 17)], 200, "text"), ([(1, 299, 1)], 0, "rle"), ([(100, 4, 50)], 20, "raw"), ([(10, 9, 17)], 120, "text")], seed=37)
        b = Case("nd-tight/run-raw", data, ref_merge(seqs), 3, NO_DELIMITERS | REPCODES, True)
        data, seqs = nd([(4, 5, 2), (8, 30, 3)], 60, seed=41)
        c = Case("nd-tight/short", data, seqs, 1, NO_DELIMITERS | CHECKSUM | REPCODES, True)
        return [a, b, c]
    return SC._memo("nd-tight", build)


def random_arrays(n=300, seed=43):
    """random litLength / matchLength / offset over random text up to 300 KiB, valid (built with their content) and invalid (lengths and offsets drawn freely)"""
    def build():
        rnd = random.Random(seed)
        out = []
        while len(out) < n:
            i = len(out)
            big = i % 12 == 0
            size_goal = rnd.randrange(BLOCK, 300 * 1024) if big else rnd.randrange(1, 20000)
            triples, total = [], 0
            while total < size_goal:
                ll = rnd.choice((0, 0, 1, 3, rnd.randrange(0, 40), rnd.randrange(0, 3000), rnd.randrange(0, 150000) if big else 7))
                ml = rnd.choice((4, 5, 6, 8, rnd.randrange(4, 60), rnd.randrange(4, 2000), rnd.randrange(4, 400000) if big else 9))
                if total + ll == 0:
                    ll = 1 + rnd.randrange(9)
                off = rnd.choice((1, 2, 3, 4, 8, rnd.randrange(1, total + ll + 1)))
                off = min(off, total + ll)
                triples.append((ll, ml, off))
                total += ll + ml
            data, seqs = nd(triples, rnd.choice((0, 0, 5, rnd.randrange(0, 2000))), seed=seed + i)
            if len(data) > 300 * 1024:
                data = data[:300 * 1024]              # (the array then covers more than the source)
            valid = i % 3 != 0
            if not valid:
                s = [list(q) for q in seqs]
                for _ in range(rnd.randrange(1, 4)):
                    k = rnd.randrange(len(s))
                    what = rnd.randrange(5)
                    if what == 0: s[k][0] = rnd.choice((0, 1, len(data), len(data) + 1, rnd.randrange(1 << 20), 0xFFFFFFFD, 0xFFFFFFFF))
                    elif what == 1: s[k][1] = rnd.choice((0, 1, rnd.randrange(1 << 18), rnd.randrange(1 << 22)))
                    elif what == 2: s[k][2] = rnd.choice((0, 1, 2, 3, rnd.randrange(1 << 18), rnd.randrange(1 << 22)))
                    elif what == 3: s = s[:k + 1]
                    else: s.insert(k, [rnd.randrange(1, 9), 0, 0, 0])
                seqs = [tuple(q) for q in s]
            if undefined_in_reference(seqs, len(data)):
                continue
            level = rnd.choice((1, 2, 3, -1, -5, -30) + ((4, 5, 7) if len(data) <= BLOCK else ()))
            out.append(Case(f"random/{i}", data, seqs, level, NO_DELIMITERS | rnd.choice((0, CHECKSUM)), valid and len(data) <= 300 * 1024 and sum(q[1] + q[2] for q in seqs) <= len(data)))
        return out
    return SC._memo(("nd-random", n, seed), build)
