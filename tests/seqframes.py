"""Frames from hand-chosen sequences: the caller writes (literal length, match length, offset) triples and block ends, the
reference's ZSTD_compressSequences (oracle/_ref/libzstd_ref.so) turns them into a frame, and plain Python produces the content
they stand for.  The decoders therefore meet executor and sequence-decoder shapes that no match finder emits on request:
64 chained dependencies in one batch, batches of exactly 4095 / 4096 / 4097 bytes, sources straddling the staged window or the
dictionary's end, every repcode form as a block's first sequence, the first and last value of every long length code.

build()            -> (frame, content, shape): the frame is confirmed by the reference's decoder before anybody else sees it
census()           -> what each batch of 64 sequences (the decoders' unit of execution) holds, lane by lane
families A .. H    -> lists of Case; every pattern is repeated at the lane positions LANES of a batch
seq_bits()         -> how many bits each sequence of a predefined-table block takes from the bitstream
spread(), lanes_where(), chain_starts() -> what the conditions on the inputs are written with (asserted in tests/test_emu_seqframes.py)
TEST INFRASTRUCTURE — used by tests/test_emu_seqframes.py (CPU) and tests/test_gpu_seqframes.py (GPU)."""
import bisect
import ctypes as C
import random
import struct
import zlib
from collections import namedtuple

import dictutil

BATCH = 64                     # ZD_SEQ_BATCH: sequences decoded and executed at a time, counted from a block's start
STAGE = 4096                   # ZD_STAGE_BYTES: a batch of at most this many output bytes is assembled in LDS by the split pipelines
BLOCK_MAX = 131072
LANES = (0, 1, 7, 31, 32, 33, 62, 63)
LETTERS = b"etaoinsr"
_TEXT = bytes(LETTERS[i & 7] for i in range(256))
FORMS = ("rep0", "rep1", "rep2", "rep1_ll0", "rep2_ll0", "rep0m1_ll0")

LL_BASE = [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]          # codes 16 .. 35
LL_BITS = [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]      # codes 32 .. 52
ML_BITS = [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


class _Seq(C.Structure):
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


Dict = namedtuple("Dict", "raw content reps")          # the dictionary as handed to the decoders, the bytes matches may reach, its repcodes


def as_dict(dictionary):
    if dictionary is None or isinstance(dictionary, Dict):
        return dictionary
    assert dictionary[:4] != struct.pack("<I", 0xEC30A437)
    return Dict(bytes(dictionary), bytes(dictionary), (1, 4, 8))         # raw content


def _lib():
    from oracle import ref
    L = ref.lib()
    L.ZSTD_compressSequences.restype = C.c_size_t
    L.ZSTD_compressSequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(_Seq), C.c_size_t, C.c_void_p, C.c_size_t]
    L.ZSTD_CCtx_loadDictionary.restype = C.c_size_t
    L.ZSTD_CCtx_loadDictionary.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return L


def _literals(rnd, n, kind):
    if n == 0:
        return b""
    if kind == "rle":
        return b"e" * n
    raw = rnd.randbytes(n)
    return raw if kind == "raw" else raw.translate(_TEXT)


def build(blocks, level=3, checksum=False, window_log=0, dictionary=None, literals="text", seed=1, ext_rep=True, decodable=True):
    """blocks = [([(ll, ml, offset), ...], trailing literals), ...] -> (frame, content, shape).  The content is what the triples
    mean: ll literal bytes, then ml bytes each equal to the byte `offset` positions back (copied in runs of at most `offset`
    bytes, which is the same as byte by byte), the dictionary's content in front.  literals: "text" eight letters (Huffman),
    "raw" random bytes, "rle" one value; a bytes object: the frame's literal bytes themselves, taken run after run (tests/seqrecords.py
    chooses histograms with it).  ext_rep=False: searchForExternalRepcodes off — every offset is stored as offset + 3, no repcode is written.
    decodable=False: offsets may reach in front of the content (tests/branch_cases.py "wide-codes": an offset code no window allows) — validateSequences is off, the
    reference writes the frame all the same and no decoder takes it; the bytes of such a match are more literal-kind bytes, which no one reads."""
    from oracle import ref
    assert level <= 9                                  # from level 16 on the library may re-split blocks
    L = _lib()
    d = as_dict(dictionary)
    rnd = random.Random(seed)
    if isinstance(literals, (bytes, bytearray)):
        given, taken = bytes(literals), [0]

        def lits(n):
            taken[0] += n
            assert taken[0] <= len(given), "more literals asked for than given"
            return given[taken[0] - n:taken[0]]
    else:
        def lits(n):
            return _literals(rnd, n, literals)
    out = bytearray(d.content if d else b"")
    base = len(out)
    n_seq = sum(len(s) for s, _ in blocks) + len(blocks)
    arr = (_Seq * n_seq)()
    i = 0
    for seqs, tail in blocks:
        for ll, ml, off in seqs:
            out += lits(ll)
            assert ml >= 3 and 1 <= off and (off <= len(out) or not decodable), (ll, ml, off, len(out))
            arr[i].offset, arr[i].litLength, arr[i].matchLength = off, ll, ml
            i += 1
            if off > len(out):
                out += _literals(rnd, ml, "text")
                ml = 0
            while ml:
                n = min(ml, off)
                s = len(out) - off
                out += out[s:s + n]
                ml -= n
        out += lits(tail)
        arr[i].offset, arr[i].litLength, arr[i].matchLength = 0, tail, 0       # the block delimiter
        i += 1
    content = bytes(out[base:])
    cctx = L.ZSTD_createCCtx()
    try:
        params = [(100, level), (201, int(checksum)), (105, 3),                  # compressionLevel, checksumFlag, minMatch
                  (1008, 1), (1009, int(decodable)),                             # blockDelimiters: explicit; validateSequences
                  (1016, 1 if ext_rep else 2)]                                   # searchForExternalRepcodes: on (below level 10 "auto" means off: no repcode would be written); 2 = off
        if window_log:
            params.append((101, window_log))
        for p, v in params:
            ref._check(L.ZSTD_CCtx_setParameter(cctx, p, v))
        if d:
            ref._check(L.ZSTD_CCtx_loadDictionary(cctx, d.raw, len(d.raw)))
        cap = L.ZSTD_compressBound(len(content)) + 64 + 4 * len(blocks)
        dst = C.create_string_buffer(cap)
        r = ref._check(L.ZSTD_compressSequences(cctx, dst, cap, arr, n_seq, content, len(content)))
        frame = dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)
    if decodable:
        back = ref.decompress_using_dict(frame, d.raw, len(content)) if d else ref.decompress(frame, len(content))
        assert back == content, "the reference does not confirm the frame"
    return frame, content, walk(frame)


def walk(frame):
    """the frame's blocks: type (0 raw, 1 RLE, 2 compressed), size, nbSeq, the table modes [LL, OF, ML], where the sequence section starts and the block ends"""
    assert frame[:4] == b"\x28\xB5\x2F\xFD"
    fhd = frame[4]
    single, didc, fcs = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[didc] + (single if fcs == 0 else 1 << fcs)
    blocks, first = [], pos
    while True:
        assert pos + 3 <= len(frame), "the frame ends inside its blocks"
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
        pos += 3
        rec = {"type": typ, "size": size, "nbSeq": 0, "modes": None, "seq_pos": None, "end": pos + (1 if typ == 1 else size)}
        if typ == 2:
            b = frame[pos:pos + size]
            lt, fmt = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:
                lh, n = (1, b[0] >> 3) if fmt in (0, 2) else ((2, int.from_bytes(b[:2], "little") >> 4) if fmt == 1 else (3, int.from_bytes(b[:3], "little") >> 4))
                c = n if lt == 0 else 1
            else:
                w = int.from_bytes(b[:5], "little")
                lh, n, c = ((3, (w >> 4) & 0x3FF, (w >> 14) & 0x3FF) if fmt < 2 else
                            ((4, (w >> 4) & 0x3FFF, (w >> 18) & 0x3FFF) if fmt == 2 else (5, (w >> 4) & 0x3FFFF, (w >> 22) & 0x3FFFF)))
            ip = lh + c
            rec.update(lit_type=lt, lit_size=n, seq_pos=pos + ip)
            nb = b[ip]
            ip += 1
            if nb > 0x7F:
                if nb == 0xFF:
                    nb = int.from_bytes(b[ip:ip + 2], "little") + 0x7F00
                    ip += 2
                else:
                    nb = ((nb - 0x80) << 8) + b[ip]
                    ip += 1
            rec["nbSeq"] = nb
            if nb:
                rec["modes"] = [(b[ip] >> 6) & 3, (b[ip] >> 4) & 3, (b[ip] >> 2) & 3]
        blocks.append(rec)
        pos = rec["end"]
        if last:
            break
    return {"blocks": blocks, "checksum": bool(fhd & 4), "size": pos + (4 if fhd & 4 else 0), "dict_id": didc != 0, "header": first}


def simple(shape):
    """the three-stage pipeline's contract (top of zj_decode_split.h): one compressed block"""
    return len(shape["blocks"]) == 1 and shape["blocks"][0]["type"] == 2


def classify(off, ll, rep):
    """which repcode form the encoder writes for a raw offset (ZSTD_finalizeOffBase) and the history behind it (ZSTD_updateRep)"""
    if ll and off == rep[0]:
        return "rep0", rep
    if off == rep[1]:
        return ("rep1" if ll else "rep1_ll0"), [rep[1], rep[0], rep[2]]
    if off == rep[2]:
        return ("rep2" if ll else "rep2_ll0"), [rep[2], rep[0], rep[1]]
    if not ll and off == rep[0] - 1:
        return "rep0m1_ll0", [rep[0] - 1, rep[0], rep[1]]
    return "off", [off, rep[0], rep[1]]


Lane = namedtuple("Lane", "k ll ml off form first_of_block mp dep depth before at_start dict_n dict_end dict_first lit_tail")
#   dep: the earlier lanes whose match output this match reads, as the executor computes them; depth: the longest such chain
#   before: source bytes in front of the batch's first output byte (the staged window's start); at_start: the source ends exactly there
#   dict_n: bytes taken from the dictionary; dict_end: the source ends on its last byte; dict_first: it starts on its first
#   lit_tail: a run of 1 .. 32 literals that ends within 32 bytes of the literal buffer's end (lp + 32 > litAvail)
Batch = namedtuple("Batch", "block index op0 out_total lanes runs_m1")


def census(blocks, shape=None, dictionary=None):
    """per batch of 64 consecutive sequences from a block's start: the executor's view of every lane.  `shape` tells which blocks
    came out compressed (only those move the repcode history); without it every block with sequences is taken as compressed."""
    d = as_dict(dictionary)
    dsize = len(d.content) if d else 0
    rep = list(d.reps) if d else [1, 4, 8]
    pos = 0
    out = []
    for bi, (seqs, tail) in enumerate(blocks):
        compressed = (shape["blocks"][bi]["type"] == 2) if shape else bool(seqs)
        lit_size = sum(s[0] for s in seqs) + tail
        if not compressed:                               # a raw or RLE block: nothing to decode or execute, the history stays
            pos += sum(s[0] + s[1] for s in seqs) + tail
            continue
        lp = 0
        brep = list(rep)
        run = 0
        for b0 in range(0, len(seqs), BATCH):
            op0 = pos
            starts, ends, depth, lanes, runs = [], [], [], [], []
            for k, (ll, ml, off) in enumerate(seqs[b0:b0 + BATCH]):
                form, brep = classify(off, ll, brep)
                run = run + 1 if form == "rep0m1_ll0" else 0
                runs.append(run)
                mp = pos + ll
                sp = mp - off
                dn = min(ml, -sp) if sp < 0 else 0
                ms = max(sp, 0)
                me = min(ms + ml - dn, mp)
                dep = range(0)
                if ml > dn:
                    jlo = bisect.bisect_right(ends, ms)                  # first j with mEnd_j > ms
                    jhi = max(jlo, bisect.bisect_left(starts, me))       # first j with mStart_j >= me
                    dep = range(jlo, jhi)
                depth.append(1 + max((depth[j] for j in dep), default=0))
                before = max(0, min(op0, sp + ml) - max(sp, 0)) if sp < op0 else 0
                lanes.append(Lane(k, ll, ml, off, form, b0 + k == 0, mp, dep, depth[-1], before, sp < op0 and sp + ml == op0 and ml > dn,
                                  dn, dn > 0 and sp + ml == 0, sp == -dsize and dsize > 0, 0 < ll <= 32 and lp + 32 > lit_size))
                starts.append(mp)
                ends.append(mp + ml)
                pos = mp + ml
                lp += ll
            out.append(Batch(bi, b0 // BATCH, op0, pos - op0, lanes, runs))
        pos += tail
        if compressed:
            rep = brep
    return out


LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]               # the format's predefined distributions
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7


def _ll_code(ll):
    if ll < 16:
        return ll, 0
    i = bisect.bisect_right(LL_BASE, ll) - 1
    return 16 + i, LL_BITS[i]


def _ml_code(ml):
    if ml < 35:
        return ml - 3, 0
    i = bisect.bisect_right(ML_BASE, ml) - 1
    return 32 + i, ML_BITS[i]


def _of_code(lane):
    base = {"off": lane.off + 3, "rep0": 1, "rep1": 2, "rep2": 3, "rep1_ll0": 1, "rep2_ll0": 2, "rep0m1_ll0": 3}[lane.form]
    return base.bit_length() - 1


def seq_bits(shape, cen):
    """{block: [(T, wide), ...]} for the blocks whose three tables are the predefined ones: T = the bits one sequence takes from the bitstream (its extra bits and, unless
    it is the block's last, the bits of the three state updates), wide = at least 16 bytes of bitstream lie below it (zd_seq_batch's flag).  A symbol of probability
    1 or "less than 1" owns one cell of nbBits = tableLog, so T is known exactly for sequences made of such symbols; T is None where a more frequent symbol occurs."""
    out = {}
    for bi, blk in enumerate(shape["blocks"]):
        if blk["modes"] != [0, 0, 0]:
            continue
        lanes = [l for bt in cen if bt.block == bi for l in bt.lanes]
        ts = []
        for i, l in enumerate(lanes):
            (lc, lx), (mc, mx), oc = _ll_code(l.ll), _ml_code(l.ml), _of_code(l)
            t = lx + mx + oc
            if i + 1 < len(lanes):
                t = None if abs(LL_DEF[lc]) != 1 or abs(ML_DEF[mc]) != 1 or abs(OF_DEF[oc]) != 1 else t + 6 + 6 + 5
            ts.append(t)
        below, rec = 0, []
        for t in reversed(ts):
            below = None if t is None or below is None else below + t
            rec.append((t, None if below is None else (below + 7) // 8 >= 16))
        out[bi] = rec[::-1]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# writing blocks


class NeedHistory(Exception):
    pass


class Blk:
    """one block being written: positions are relative to the block's start, `hist` bytes (a dictionary) lie in front of it"""

    def __init__(self, hist=0, reps=(1, 4, 8)):
        self.seqs, self.pos, self.hist, self.rep, self.bstart, self.form = [], 0, hist, list(reps), 0, None

    @property
    def n(self):
        return len(self.seqs)

    def add(self, ll, ml, off):
        if off > self.pos + ll + self.hist:
            raise NeedHistory()
        assert off >= 1 and ml >= 3
        if self.n % BATCH == 0:
            self.bstart = self.pos
        self.form, self.rep = classify(off, ll, self.rep)
        self.seqs.append((ll, ml, off))
        self.pos += ll + ml

    def batch_start(self):
        """where the batch of the NEXT sequence starts"""
        return self.pos if self.n % BATCH == 0 else self.bstart

    def filler(self):
        if self.pos < 330:
            self.add(330, 4, 2)                                        # the feeder: history for every offset the patterns use
        else:
            self.add(2, 4, 2 + self.n % 3)

    def mark(self):
        return (len(self.seqs), self.pos, list(self.rep), self.bstart)

    def back(self, m):
        del self.seqs[m[0]:]
        self.pos, self.rep, self.bstart = m[1], m[2], m[3]


class P:
    """a pattern: fn(blk) appends its sequences; the one it is about is the `lead`-th of them (aligned to the lane asked for)"""

    def __init__(self, fn, lead=0, tag=None):
        self.fn, self.lead, self.tag = fn, lead, tag

    def __call__(self, b):
        self.fn(b)


def pack(patterns, lane, limit=16384, hist=0, tails=(0,), closer=None):
    """blocks of at most `limit` bytes holding the patterns, each aligned to `lane` of a batch behind filler sequences"""
    blocks = []
    b = Blk(hist)

    def close():
        nonlocal b
        if closer:
            closer(b)
        blocks.append((b.seqs, tails[len(blocks) % len(tails)]))
        b = Blk(hist)
    for pat in patterns:
        extra = 0
        while True:
            m = b.mark()
            try:
                for _ in range(extra):
                    b.filler()
                while (b.n + pat.lead) % BATCH != lane:
                    b.filler()
                pat(b)
            except NeedHistory:
                b.back(m)
                extra += BATCH
                assert extra <= 2 * BATCH
                continue
            if b.pos > limit and m[0] > 0:
                b.back(m)
                close()
                extra = 0
                continue
            break
    if b.n:
        close()
    return blocks


def one(ll, ml, off):
    return P(lambda b: b.add(ll, ml, off))


Case = namedtuple("Case", "family name blocks level literals dictionary window_log")


def case(family, name, blocks, level=3, literals="text", dictionary=None, window_log=0):
    return Case(family, name, blocks, level, literals, dictionary, window_log)


_built = {}


def build_case(c):
    """(frame, content, shape, census), built once per process"""
    key = (c.family, c.name)
    if key not in _built:
        frame, content, shape = build(c.blocks, level=c.level, dictionary=c.dictionary, literals=c.literals, window_log=c.window_log, seed=zlib.crc32(f"{c.family}/{c.name}".encode()))
        _built[key] = (frame, content, shape, census(c.blocks, shape, c.dictionary))
    return _built[key]


def _singles_and_groups(family, name, blocks, group=4, literals=("text", "text", "raw"), levels=(3, 7)):
    """every block as a frame of its own (the three-stage pipeline and the fused kernel) and the same blocks `group` to a frame (the block stages)"""
    cases = [case(family, f"{name}/{i}", [blk], literals=literals[i % len(literals)]) for i, blk in enumerate(blocks)]
    for g in range(0, len(blocks), group):
        if len(blocks[g:g + group]) > 1:
            cases.append(case(family, f"{name}/mb{g}", blocks[g:g + group], level=levels[(g // group) % len(levels)], literals=literals[(g // group) % len(literals)]))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# A. dependency chains
CHAIN_N = (63, 64, 65, 200)
CHAIN_LINKS = {"next": (0, 3, 3), "next_ll1": (1, 3, 3), "range": (0, 3, 5), "skip": (0, 3, 6), "skip_range": (0, 4, 9)}


def _chain(n, link):
    """(8,3,8), then n matches that each read what the matches just before them wrote (links that reach further back start behind two plain ones)"""
    def fn(b):
        b.add(8, 3, 8)
        warm = 0 if link[2] == 3 else 2
        for _ in range(warm):
            b.add(0, 3, 3)
        for _ in range(n - warm):
            b.add(*link)
    return P(fn)


def _star(lane):
    """lane `lane` writes 16 bytes; every later lane of the batch copies three of them and nothing else"""
    def fn(b):
        c = b.pos + 8
        b.add(8, 16, 8)
        for i in range(BATCH - 1 - lane):
            b.add(3, 3, b.pos + 3 - (c + i % 13))
    return P(fn)


def family_a():
    cases = []
    for lane in LANES:
        pats = [_chain(n, CHAIN_LINKS[k]) for n in CHAIN_N for k in ("next", "next_ll1")] + [_chain(70, CHAIN_LINKS[k]) for k in ("range", "skip", "skip_range")] + [_star(lane)]
        cases += _singles_and_groups("A", f"lane{lane}", pack(pats, lane, limit=4000))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# B. overlap and length classes
OFFSETS = tuple(range(1, 17)) + (31, 32, 33, 63, 64, 65)
MATCHES = (3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 300)
OVER8 = ((15, 8), (16, 9), (17, 13), (63, 8), (64, 31), (64, 63), (9, 8))          # (ml, off): the 8-byte path copying over its own output
WIDE = ((65, 65), (66, 300), (127, 127), (127, 200), (128, 64), (129, 65), (129, 100), (300, 64), (300, 63), (300, 1), (129, 7), (66, 65))      # (ml, off): off >= ml, 64 <= off < ml, off < 64


def family_b():
    cases = []
    for li, lane in enumerate(LANES):
        pats = [one(j % 3, MATCHES[(j + 3 * li) % len(MATCHES)], o) for j, o in enumerate(OFFSETS)]
        pats += [one(j % 2, m, OFFSETS[(j + 5 * li) % len(OFFSETS)]) for j, m in enumerate(MATCHES)]
        pats += [one(j % 2, m, o) for j, (m, o) in enumerate(OVER8 + WIDE)]
        if lane == 0:                                                    # lane 0 of a block's FIRST batch: the history is the sequence's own literals
            for j, o in enumerate(OFFSETS):
                cases.append(case("B", f"first/{o}", [([(o, MATCHES[(j * 7) % len(MATCHES)], o)] + [(2, 4, 2 + i % 3) for i in range(30)], j % 2)], literals=("text", "raw")[j % 2]))
        cases += _singles_and_groups("B", f"lane{lane}", pack(pats, lane))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# C. the staged window
TOTALS = (STAGE - 1, STAGE, STAGE + 1)
BEFORE = (1, 7, 8, 70)


def _exact_total(total, lane):
    """the rest of the batch, so that the batch's output is exactly `total` bytes"""
    def fn(b):
        rest = BATCH - 1 - lane
        x = total - (b.pos - b.batch_start()) - 4 - 6 * rest
        b.add(x, 4, 1)
        for _ in range(rest):
            b.add(2, 4, 2)
    return P(fn)


def _src_before(a, ml, ll):
    """the source starts `a` bytes in front of the batch's first output byte"""
    def fn(b):
        if b.batch_start() + b.hist < a:
            raise NeedHistory()
        b.add(ll, ml, b.pos + ll - b.batch_start() + a)
    return P(fn)


def _src_ends_at_start(ml, ll):
    def fn(b):
        if b.batch_start() + b.hist < ml:
            raise NeedHistory()
        b.add(ll, ml, b.pos + ll - b.batch_start() + ml)
    return P(fn)


def family_c():
    cases = []
    for lane in LANES:
        blocks = []
        for t in TOTALS:
            blocks += pack([_exact_total(t, lane)], lane)                       # the block's first batch
            blocks += pack([one(2, 4, 2), _exact_total(t, lane)], lane)         # a later batch: final output in front of the window
        pats = [_src_before(a, ml, 1 + a % 2) for a in BEFORE for ml in (max(a + 1, 3), 64, 65, 100, 300) if ml > a]
        pats += [_src_ends_at_start(ml, 1) for ml in (20, 64, 65, 100)]
        blocks += pack(pats, lane)
        cases += _singles_and_groups("C", f"lane{lane}", blocks, group=3)
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# D. literal runs
LITS = (0, 1, 7, 8, 9, 31, 32, 33, 64, 200)


def _lits(ll):
    def fn(b):
        if b.pos + ll + b.hist == 0:
            raise NeedHistory()
        b.add(ll, 5, min(7, b.pos + ll + b.hist))
    return P(fn)


def family_d():
    cases = []
    for li, lane in enumerate(LANES):
        blocks = pack([_lits(ll) for ll in LITS] * 2, lane, limit=2500, tails=(0, 1, 31, 40, 0, 20), closer=_lits((5, 32, 1)[li % 3]))
        for i, blk in enumerate(blocks):
            for kind in ("text", "raw", "rle") if i == 0 else ("text", "raw"):
                cases.append(case("D", f"lane{lane}/{i}/{kind}", [blk], literals=kind))
        cases.append(case("D", f"lane{lane}/mb", blocks, literals=("text", "raw")[li % 2], level=(3, 7)[li % 2]))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# E. repcodes
SETUP = ((2, 4, 11), (2, 4, 17), (2, 4, 23))            # leaves the history [23, 17, 11], whatever it was
RUNS = (2, 3, 10)


def _form_seq(name, rep):
    return {"rep0": (2, 4, rep[0]), "rep1": (2, 4, rep[1]), "rep2": (2, 4, rep[2]), "rep1_ll0": (0, 4, rep[1]), "rep2_ll0": (0, 4, rep[2]), "rep0m1_ll0": (0, 4, rep[0] - 1)}[name]


def _form(name, run=1):
    def fn(b):
        for s in SETUP:
            b.add(*s)
        for _ in range(run):
            b.add(*_form_seq(name, b.rep))
            assert b.form == name
    return P(fn, lead=3)


def dict_with_reps(reps=(30, 50, 70), seed=5, size=1500):
    rnd = random.Random(seed)
    content = _literals(rnd, size, "text")
    hist = [0] * 256
    for ch in content:
        hist[ch] += 1
    raw = dictutil.build(content, 7000 + seed, hist, dictutil.normalise([1] * 20, 7), 7, dictutil.normalise([3 if i < 20 else 1 for i in range(53)], 8), 8,
                         dictutil.normalise([4 if i < 10 else 1 for i in range(36)], 8), 8, reps=reps)
    return Dict(raw, content, tuple(reps))


def raw_dict(seed=9, size=1000):
    return as_dict(_literals(random.Random(seed), size, "text"))


def family_e():
    cases = []
    for lane in LANES:                                                   # in mid-block, at every lane position
        pats = [_form(f) for f in FORMS] + [_form("rep0m1_ll0", run) for run in RUNS]
        cases += _singles_and_groups("E", f"lane{lane}", pack(pats, lane), literals=("text", "raw"))
    setup = ([(330, 4, 2)] + list(SETUP), 3)
    rep = [23, 17, 11]
    between = {"seq": None, "raw": ([], 5), "rle": ([(1, 200, 1)], 0), "noseq": ([], 200)}
    for f in FORMS:                                                      # as the first sequence of block 2, 3, ... and behind blocks that leave the history alone
        for run in (1,) + (RUNS if f == "rep0m1_ll0" else ()):
            first, r = [], list(rep)
            for _ in range(run):
                first.append(_form_seq(f, r))
                _, r = classify(first[-1][2], first[-1][0], r)
            formblock = (first + list(SETUP), 2)
            for level in (3, 7):
                blocks = [setup]
                for what, blk in between.items():
                    blocks += ([blk] if blk else []) + [formblock]
                blocks.append(formblock)                             # ... and behind a block with sequences, as block 3 or later
                cases.append(case("E", f"first/{f}/{run}/L{level}", blocks, level=level))
    d = dict_with_reps()
    for f in FORMS:                                                      # the frame's first sequence takes each of the dictionary's repcodes
        ll, ml, off = _form_seq(f, list(d.reps))
        cases.append(case("E", f"dictrep/{f}", [([(ll, 5, off), (2, 4, 9), (2, 4, 3)], 1)], dictionary=d))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# F. codes and counts
COUNTS = (127, 128, 0x7EFF, 0x7F00, 0x7F01)
WIDE_SEQ = (40000, 70000, 1100000)                      # LL code 34, ML code 52, OF code 20: 15 + 16 + 20 extra bits in one sequence


def code_values():
    """(kind, code, value) for the first and last value of every long length code that a 128 KiB block can hold"""
    out = []
    for i, (base, bits) in enumerate(zip(LL_BASE, LL_BITS)):
        out += [("ll", 16 + i, base), ("ll", 16 + i, base + (1 << bits) - 1)]
    for i, (base, bits) in enumerate(zip(ML_BASE, ML_BITS)):
        out += [("ml", 32 + i, base), ("ml", 32 + i, base + (1 << bits) - 1)]
    return [v for v in out if v[2] + 8 <= BLOCK_MAX - 64 * 6 - 400]       # (room for the fillers in front): drops the last value of LL code 35 and of ML code 52 only


def _count_block(n, seed):
    rnd = random.Random(seed)
    seqs = [(8, 3, 8)]
    for i in range(1, n):
        seqs.append((1 if i % 8 == 0 else 0, 3 + (rnd.randrange(4) == 0), rnd.choice((1, 2, 3, 5, 8, 11))))
    return (seqs, seed % 3)


def family_f():
    cases = []
    for li, lane in enumerate(LANES):
        pats = []
        vals = code_values()
        vals = [v for pair in zip(vals[:len(vals) // 2], vals[len(vals) // 2:]) for v in pair] + ([vals[-1]] if len(vals) % 2 else [])       # long literal runs and long matches in turn: every block gains
        for j, (kind, code, v) in enumerate(vals):
            pats.append(one(v, 4, (1, 2, 41)[j % 3]) if kind == "ll" else one(2, v, (1, 2, 41, 81, 300)[j % 5]))
        blocks = pack(pats, lane, limit=BLOCK_MAX)
        for i, blk in enumerate(blocks):
            cases.append(case("F", f"codes/lane{lane}/{i}", [blk], literals=("text", "raw")[(i + li) % 2]))
        cases.append(case("F", f"codes/lane{lane}/mb", blocks[-4:], literals=("raw", "text")[li % 2], level=(3, 7)[li % 2]))
    for n in COUNTS:
        blk = _count_block(n, n)
        cases.append(case("F", f"count/{n}", [blk]))
        cases.append(case("F", f"count/{n}/twice", [blk, blk], level=7))          # the second block repeats the first one's statistics: repeat-mode tables
    same = ([(12, 5, (5, 7, 9, 11)[i % 4]) for i in range(127)], 0)               # one code each (four offsets in turn: none is a repcode): RLE tables
    cases.append(case("F", "rle_tables", [same]))
    cases.append(case("F", "rle_tables/twice", [same, same], level=7))
    # the widest sequence, as the block's first (its bits lie at the stream's end, far above the start) and as its last (within 16 bytes of the start)
    ll, ml, off = WIDE_SEQ
    big = [([(65536, 65536, 65536)], 0)] * 9                                      # 1 179 648 bytes in front
    tail_fill = [(2, 4, 2 + i % 3) for i in range(300)]
    cases.append(case("F", "wide", big + [([(ll, ml, off)] + tail_fill, 5), (tail_fill[:40] + [(ll, ml, off)], 0)], literals="raw", window_log=21))
    # every width from 57 to 66 bits around zd_seq_batch's 56-bit / 64-bit register path: few sequences of rare codes (predefined tables: 17 state bits each), offset code 20,
    # with at least 16 bytes of bitstream below them; each block ends with one of 57 bits that has fewer below it, and a short last one
    def widths(sums, at):
        seqs = [(LL_BASE[lx - 6 + 9], ML_BASE[mx - 7 + 11], 1100000 + 1000 * (at + i)) for i, (lx, mx) in enumerate(sums)]
        return (seqs + [(LL_BASE[11], ML_BASE[16], 1150000 + 1000 * at), (2, 4, 7)], 3)
    cases.append(case("F", "widths", big + [widths(((8, 12), (8, 13), (9, 13), (10, 13), (11, 13), (12, 13)), 0), widths(((13, 13), (13, 14), (14, 14), (14, 15)), 10)],
                      literals="raw", window_log=21))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# G. dictionary
G_MATCHES = (20, 64, 65, 100)
STRADDLE = (1, 7, 8, 70)


def _dict_pat(kind, ml, big, lane, s=0):
    def fn(b):
        if big and lane != 0:
            b.add(4200, 4, 1)
        mp = b.pos + 2
        off = {"inside": mp + ml + 5, "end": mp + ml, "straddle": mp + ml - s, "first": mp + b.hist}[kind]
        b.add(2, ml, off)
        if big and lane == 0:
            b.add(4200, 4, 1)
    return P(fn, lead=1 if big and lane != 0 else 0)


def family_g():
    cases = []
    dicts = (("raw", raw_dict()), ("full", dict_with_reps(seed=6)))
    for li, lane in enumerate(LANES):
        for dname, d in dicts:
            for big in (False, True):
                pats = []
                for ml in G_MATCHES:
                    pats += [_dict_pat(k, ml, big, lane) for k in ("inside", "end", "first")]
                    pats += [_dict_pat("straddle", ml, big, lane, s) for s in STRADDLE if s < ml]
                for i, blk in enumerate(pack(pats, lane, hist=len(d.content))):
                    cases.append(case("G", f"{dname}/lane{lane}/{'big' if big else 'small'}/{i}", [blk], dictionary=d, literals=("text", "raw")[(i + li) % 2]))
    return cases


# ------------------------------------------------------------------------------------------------------------------------
# H. random programs


def random_program(rnd, n, max_out, hist=0, reps=(1, 4, 8)):
    """one block of up to n sequences and at most max_out bytes, the weights pushed towards the edges of families A .. G"""
    b = Blk(hist, reps)
    prev_ml = 3
    for _ in range(n):
        ll = rnd.choice((0, 0, 0, 1, 1, 2, 3, 7, 8, 9, 31, 32, 33, rnd.randrange(0, 40), rnd.randrange(0, 40), 64, 200))
        ml = rnd.choice((3, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 66, 127, 129, 300, rnd.randrange(3, 40), rnd.randrange(3, 40), rnd.randrange(3, 40)))
        avail = b.pos + ll + hist
        if avail == 0:
            ll = avail = rnd.choice((1, 8, 33))
        mp = b.pos + ll
        k = rnd.randrange(9)
        if k <= 1: off = rnd.randrange(1, 17)
        elif k == 2: off = rnd.choice((31, 32, 33, 63, 64, 65))
        elif k == 3: off = rnd.choice((b.rep[0], b.rep[1], b.rep[2], b.rep[0] - 1))
        elif k == 4: off = rnd.choice((prev_ml + ll, 3, ml, ml + 1))                 # the previous match's output
        elif k == 5: off = rnd.randrange(1, avail + 1)
        elif k == 6: off = mp - b.batch_start() + rnd.choice((0, 1, 7, 8, 70, ml))  # round the batch's first byte
        elif k == 7: off = mp + rnd.choice((0, 1, ml, ml - 1, ml - 7, ml - 8, hist, hist - 1)) if hist else rnd.randrange(1, avail + 1)
        else: off = rnd.randrange(max(1, avail - 40), avail + 1)
        off = max(1, min(off, avail))
        if b.pos + ll + ml > max_out:
            break
        b.add(ll, ml, off)
        prev_ml = ml
    if not b.n:
        b.add(3, 3, 1)
    return (b.seqs, rnd.choice((0, 0, 1, 5, 31, 40)))


def damage(rnd, frame, shape):
    """one bit flipped at or behind a compressed block's sequence header"""
    blks = [k for k in shape["blocks"] if k["type"] == 2]
    k = rnd.choice(blks)
    z = bytearray(frame)
    z[rnd.randrange(k["seq_pos"], k["end"])] ^= 1 << rnd.randrange(8)
    return bytes(z)


def family_h(singles=400, multis=60, dicts=60):
    rnd = random.Random(20261019)
    cases = []
    for i in range(singles):
        n = rnd.choice((3, 20, 64, 65, 130, 200, 400))
        cases.append(case("H", f"single/{i}", [random_program(rnd, n, rnd.choice((600, 4096, 9000, 16000)))], level=rnd.choice((1, 3, 7)), literals=rnd.choice(("text", "text", "raw", "rle"))))
    for i in range(multis):
        blocks = [random_program(rnd, rnd.choice((1, 10, 64, 100, 200)), rnd.choice((300, 2500, 5000))) for _ in range(rnd.randrange(2, 7))]
        if i % 5 == 0:
            blocks = blocks[:5]
            blocks.insert(1 + i % 2, ([], 5))                                     # a raw block in between
        cases.append(case("H", f"multi/{i}", blocks, level=rnd.choice((3, 7)), literals=rnd.choice(("text", "raw"))))
    ds = (raw_dict(), dict_with_reps(seed=6))
    for i in range(dicts):
        d = ds[i % 2]
        cases.append(case("H", f"dict/{i}", [random_program(rnd, rnd.choice((3, 64, 130, 300)), rnd.choice((600, 4096, 12000)), hist=len(d.content), reps=d.reps)], dictionary=d,
                          level=rnd.choice((1, 3, 7)), literals=rnd.choice(("text", "raw"))))
    return cases


def damaged_h(ref, cases):
    """every third case of family H with one flipped bit: [(case, damaged frame, capacity, the portable reference's bytes | -code)]"""
    rnd = random.Random(77)
    out = []
    for i, c in enumerate(cases):
        if i % 3:
            continue
        frame, content, shape, _ = build_case(c)
        if not any(k["type"] == 2 for k in shape["blocks"]):
            continue
        z = damage(rnd, frame, shape)
        try:
            want = ref.decompress_portable(z, len(content), c.dictionary.raw if c.dictionary else None)
        except ref.ZstdRefError as e:
            want = -e.code
        out.append((c, z, len(content), want))
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g, "H": family_h}
_cases = {}


def family(name):
    if name not in _cases:
        _cases[name] = FAMILIES[name]()
    return _cases[name]


# ------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs


def spread(lanes, what, lowest=0):
    """a listed value must occur at 8 or more lane positions, lane 0 (or the lowest lane that can hold it) and lane 63 among them"""
    assert len(lanes) >= 8 and lowest in lanes and 63 in lanes, (what, sorted(lanes))


def lanes_where(cases, pred, batch_pred=None):
    found = set()
    for c in cases:
        for bt in build_case(c)[3]:
            if batch_pred and not batch_pred(bt):
                continue
            found.update(l.k for l in bt.lanes if pred(l))
    return found


def chain_starts(cases, n, link):
    """lanes at which a chain of n links of this kind starts: (8,3,8) followed by n dependent matches, each reading what the lanes before it wrote"""
    found = set()
    for c in cases:
        for seqs, _ in c.blocks:
            for i, s in enumerate(seqs):
                warm = 0 if link[2] == 3 else 2
                if s == (8, 3, 8) and seqs[i + 1:i + 1 + n] == [(0, 3, 3)] * warm + [link] * (n - warm) and (i + 1 + n == len(seqs) or seqs[i + 1 + n] != link):
                    found.add(i % BATCH)
    return found
