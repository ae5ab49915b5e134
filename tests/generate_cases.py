"""The matchers' sequences out (zjni_generate_sequences*, zstd-jni_amd/csrc/zj_generate.h): the cases tests/test_emu_generate.py (CPU, the lane-serial
build) and tests/test_gpu_generate.py (GPU) both run, and the oracle they compare with — the reference's own ZSTD_generateSequences, called over
ctypes on oracle/_ref/libzstd_ref.so on a fresh CCtx with only the level set.  A case is a source and a level; what the reference answers for it —
the ZSTD_Sequence array with its block delimiters, or an error code — is what the entries must answer, entry for entry.  The reference leaves a
delimiter's `rep` field as the caller's memory held it and the entries write 0: the reference's array is zeroed before the call.  Where the
entries refuse a (level, size) the reference serves (201, as the compress entries), the case says so itself.
TEST INFRASTRUCTURE."""
import ctypes as C
import os
import random
from collections import namedtuple

import sequences_cases as SC

E_PRODUCER, E_DST, E_UNSUPPORTED = 106, 70, 201     # ZSTD_error_sequenceProducer_failed, ZSTD_error_dstSize_tooSmall, the library's "not served"
BLOCK = 1 << 17
KiB = 1 << 10

Case = namedtuple("Case", "name data level want")    # want: None = ask the reference; an int = the code the entries answer themselves (-201)


def ref_answer(data, level, cap=None):
    """ZSTD_generateSequences on a fresh CCtx, the array zeroed first: [(offset, litLength, matchLength, rep)] or -code"""
    from oracle import ref
    L = SC._lib()
    cctx = L.ZSTD_createCCtx()
    try:
        ref._check(L.ZSTD_CCtx_setParameter(cctx, 100, level))
        if cap is None:
            cap = L.ZSTD_sequenceBound(len(data))
        arr = (SC._Seq * max(cap, 1))()
        C.memset(arr, 0, C.sizeof(arr))
        r = L.ZSTD_generateSequences(cctx, arr, cap, bytes(data), len(data))
        if L.ZSTD_isError(r):
            return -((1 << 64) - r)
        return [(arr[i].offset, arr[i].litLength, arr[i].matchLength, arr[i].rep) for i in range(r)]
    finally:
        L.ZSTD_freeCCtx(cctx)


def ref_rows(data, level):
    """the same as a uint32 [k, 4] numpy array (large batches), or -code"""
    import numpy as np
    from oracle import ref
    L = SC._lib()
    cctx = L.ZSTD_createCCtx()
    try:
        ref._check(L.ZSTD_CCtx_setParameter(cctx, 100, level))
        cap = L.ZSTD_sequenceBound(len(data))
        arr = np.zeros((cap, 4), dtype=np.uint32)
        r = L.ZSTD_generateSequences(cctx, C.cast(arr.ctypes.data, C.POINTER(SC._Seq)), cap, bytes(data), len(data))
        if L.ZSTD_isError(r):
            return -((1 << 64) - r)
        return arr[:r].copy()
    finally:
        L.ZSTD_freeCCtx(cctx)


_expected = {}


def expected(c, cap=None):
    if c.want is not None:
        return c.want
    key = (c.name, c.level, cap)
    if key not in _expected:
        _expected[key] = ref_answer(c.data, c.level, cap)
    return _expected[key]


def check(c, got, cap=None):
    """got: [(offset, litLength, matchLength, rep)] or -code, from either implementation"""
    want = expected(c, cap)
    if isinstance(want, int) or isinstance(got, int):
        assert got == want, (c.name, c.level, cap, got if isinstance(got, int) else len(got), want if isinstance(want, int) else len(want))
        return
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert got == want, (c.name, c.level, cap, len(got), len(want), at, got[at:at + 2], want[at:at + 2])


def blocks_of(seqs):
    """the array cut at its delimiters: [[sequences], lastLiterals]"""
    out, cur = [], []
    for s in seqs:
        if s[0] == 0 and s[2] == 0:
            out.append((cur, s[1])); cur = []
        else:
            cur.append(s)
    assert not cur
    return out


# ---- sources ----
_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


def text(n):
    """the first n bytes of one long JSON-like text"""
    big = memo("text", lambda: SC.prose((2 << 20) + 1, seed=71))
    return big[:n]


def noise(n, seed):
    return random.Random(seed).randbytes(n)


def periodic(n, seed):
    """a random 100-byte period with a single-byte change every 150-600 bytes: offsets of 100 again and again, most of them repcodes"""
    rnd = random.Random(seed)
    out = bytearray((rnd.randbytes(100) * (n // 100 + 1))[:n])
    at = rnd.randrange(150, 600)
    while at < n:
        out[at] = (out[at] + 1 + rnd.randrange(255)) & 0xFF
        for k in range(at + 100, n, 100):                   # the change stays in the period, so the match goes on behind it
            out[k] = out[at]
        at += rnd.randrange(150, 600)
    return bytes(out)


def window_of(level):
    return {1: 512 * KiB, 2: 1024 * KiB, 3: 2048 * KiB}.get(level, 512 * KiB if level < 0 else BLOCK)


EVERY = (1, 3, -5)
EDGE_SIZES = (0, 1, 6, 7, 8, 64)
SINGLE_SIZES = (4 * KiB, 64 * KiB, 65537, BLOCK)
BOUNDARY_SIZES = (BLOCK + 1, BLOCK + 6, BLOCK + 7, 3 * BLOCK + 5000)


def sizes():
    def build():
        out = []
        for level in EVERY:
            for n in EDGE_SIZES + SINGLE_SIZES + BOUNDARY_SIZES:
                out.append(Case(f"text/{n}", text(n), level, None))
            out.append(Case("text/window+1", text(window_of(level) + 1), level, -E_UNSUPPORTED))
        return out
    return memo("sizes", build)


def levels():
    def build():
        out = []
        for level in (2, 4, 5, 6, 8):
            for n in (4 * KiB, 16 * KiB + 1):
                out.append(Case(f"text/{n}", text(n), level, None))
        out.append(Case(f"text/{BLOCK}", text(BLOCK), 4, None))
        out.append(Case(f"text/{BLOCK + 7}", text(BLOCK + 7), 4, -E_UNSUPPORTED))
        return out
    return memo("levels", build)


def repcodes():
    def build():
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xmlsmall"), "rb") as f:
            xml = f.read()
        out = []
        for level in EVERY:
            out.append(Case("periodic/3-blocks", periodic(2 * BLOCK + 40000, seed=73), level, None))
            out.append(Case("xmlsmall", xml, level, None))
        return out
    return memo("repcodes", build)


def long_lengths():
    def build():
        head = noise(70000, seed=79)
        return [Case(name, data, level, None) for level in EVERY
                for name, data in (("ml>=65536", b"q" * 70000), ("ll>=65536", head + head[:4096]))]
    return memo("long", build)


def incompressible():
    def build():
        mixed = noise(BLOCK, 83) + text(BLOCK) + noise(BLOCK, 89) + text(2 * BLOCK)[BLOCK:]
        return [Case(name, data, level, None) for level in EVERY for name, data in (("noise/1-block", noise(BLOCK, 97)), ("noise-text-noise-text", mixed))]
    return memo("incompressible", build)


GROUPS = ("sizes", "levels", "repcodes", "long_lengths", "incompressible")


def every_case():
    return [c for grp in GROUPS for c in globals()[grp]()]


def small_random(count=300, seed=101):
    """seeded small inputs, 16 B - 20 KiB, text / periodic / noise mixed piece by piece, at levels 1, 3, 5 and -3 in turn"""
    def build():
        rnd = random.Random(seed)
        out = []
        for i in range(count):
            n = rnd.randrange(16, 20 * KiB + 1) if i % 3 else rnd.randrange(16, 600)
            data = bytearray()
            while len(data) < n:
                piece = rnd.randrange(1, 4000)
                kind = rnd.randrange(3)
                at = rnd.randrange(0, 100000)
                data += text(at + piece)[at:] if kind == 0 else (periodic(piece, rnd.randrange(1 << 30)) if kind == 1 else rnd.randbytes(piece))
            out.append(Case(f"random/{i}", bytes(data[:n]), (1, 3, 5, -3)[i % 4], None))
        return out
    return memo(("random", count, seed), build)


def capacity_frames():
    """three frames for the walk over every capacity; the third has two blocks"""
    return memo("capacity", lambda: [Case("cap/text-700", text(700), 3, None), Case("cap/periodic-2000", periodic(2000, 103), 1, None),
                                     Case("cap/two-blocks", noise(BLOCK - 300, 107) + text(900), 3, None)])


# ---- the export alone: records the test writes ----
def export_model(recs, last_ll, hist):
    """ZSTD_copyBlockSequences (N/compress/zstd_compress.c:3451-3507) restated: recs = [(ll, ml, offBase)], hist = the block-start repcodes"""
    rep, out = list(hist), []
    for ll, ml, ob in recs:
        code = 0
        if ob <= 3:
            code = ob
            raw = rep[ob - 1] if ll else ((rep[0] - 1) & 0xFFFFFFFF if ob == 3 else rep[ob])
            rc = ob - 1 + (0 if ll else 1)                     # ZSTD_updateRep
            if rc:
                cur = (rep[0] - 1) & 0xFFFFFFFF if rc == 3 else rep[rc]
                rep = [cur, rep[0], rep[1] if rc >= 2 else rep[2]]
        else:
            raw = ob - 3
            rep = [raw, rep[0], rep[1]]
        out.append((raw, ll, ml, code))
    return out + [(0, last_ll, 0, 0)]


def export_cases():
    """[(name, [(ll, ml, offBase)], lastLL, history)]: 0, 1, 63, 64, 65 and 129 sequences; every repcode form with and without literals; a chain of 70
    repcodes across a tile edge; a history other than {1, 4, 8}"""
    def build():
        rnd = random.Random(109)
        out = []
        for k in (0, 1, 63, 64, 65, 129):
            out.append((f"plain/{k}", [(rnd.randrange(0, 40), rnd.randrange(3, 60), 4 + rnd.randrange(5000)) for _ in range(k)], rnd.randrange(50), (1, 4, 8)))
            out.append((f"mixed/{k}", [(rnd.randrange(0, 3), rnd.randrange(3, 60), rnd.choice((1, 2, 3, 3, 4 + rnd.randrange(5000)))) for _ in range(k)], 0, (11, 22, 33)))
        forms = [(ll, 5, ob) for ob in (1, 2, 3) for ll in (7, 0)]
        out.append(("forms", [(3, 4, 103), (2, 4, 203), (1, 4, 303)] + forms, 9, (1, 4, 8)))
        out.append(("forms/first", forms, 0, (1000, 2000, 3000)))
        for ob, ll in ((1, 0), (2, 0), (3, 0), (3, 5), (2, 5), (1, 5)):
            out.append((f"lone/ob{ob}/ll{ll}", [(ll, 6, ob)], 1, (500, 600, 700)))
        out.append(("chain-70", [(4, 8, 4 + 96)] * 30 + [(rnd.randrange(0, 2), 9, rnd.choice((1, 2, 3))) for _ in range(70)] + [(1, 5, 50)] * 5, 3, (1, 4, 8)))
        out.append(("long", [(70000, 4, 10), (0, 70000, 1), (0, 131072, 2)], 65536, (1, 4, 8)))
        return out
    return memo("export", build)
