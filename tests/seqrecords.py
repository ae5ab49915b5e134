"""The entropy stage of the encoder on hand-written sequences: the caller writes (literal length, match length, offset) triples, a tail and the
literal bytes; records() turns them into what a match finder would have left in a frame slot ({ll, ml, offBase, pos} records, litSize, lastLL),
seqframes.build() has the reference's ZSTD_compressSequences write the frame for the same triples — and that frame is what the stage must produce,
byte for byte.  The stage (zj_encode.h: literal gather, histograms, Huffman build, stream packing, tANS tables, sequence coding, mode selection,
block placement) therefore meets quantities no finder emits on request: literal runs of exactly 64 / 65 bytes, literal sections of 255 / 256,
1023 / 1024, 16383 / 16384 bytes, 127 / 128 and 0x7EFF / 0x7F00 sequences, histograms on the bars of ZSTD_selectEncodingType, blocks whose
compressed size passes through srcSize - minGain.

records()           -> the repcode model (ZSTD_finalizeOffBase / ZSTD_updateRep); self-checking: a mistake in it makes every frame differ
families G L S M W R B U N -> lists of Case (one block each); every case runs at levels 1 and 3, and at 4 and 5 when it fits in 16 KiB
families P, RB      -> lists of MCase: frames of several caller-cut blocks (previous tables, repcodes behind raw and RLE blocks), levels 1 and 3
bound_U()           -> the pipelined parse's upper bound of a block's size and its premises, restated from the records
TEST INFRASTRUCTURE — used by tests/test_emu_seqrecords.py (CPU) and tests/test_gpu_seqrecords.py (GPU)."""
import random
import zlib
from collections import namedtuple

import seqframes as S
from util import equal_count_inputs

POSITIONS = S.LANES + (64, 127, 128, 129)          # the gather takes 2 x 64 records a pass: the lanes of the first half, the second half's first and last, the next pass
CHAIN_MAX = 16384                                   # levels 4 and 5 are restated for frames to 16 KiB (the hash-chain sizes)


def records(seqs, tail, reps=(1, 4, 8), ext_rep=True):
    """(flat [ll, ml, offBase, pos] * n, litSize, repcodes after the block).  ext_rep: N/compress/zstd_compress.c:6622-6636 (ZSTD_finalizeOffBase: the raw offset
    against the running history, the forms shifted by one when ll = 0) and zstd_compress_internal.h:817-835 (ZSTD_updateRep), as ZSTD_transferSequences_wBlockDelim
    applies them (zstd_compress.c:6673-6679).  Without it every offset is stored as offset + 3 and the history becomes the last three offsets (:6700-6718)."""
    rep = list(reps)
    flat, pos, lit = [], 0, 0
    for ll, ml, off in seqs:
        ll0 = ll == 0
        base = off + 3
        if ext_rep:
            if not ll0 and off == rep[0]: base = 1
            elif off == rep[1]: base = 2 - ll0
            elif off == rep[2]: base = 3 - ll0
            elif ll0 and off == rep[0] - 1: base = 3
            if base > 3:
                rep = [off, rep[0], rep[1]]
            else:
                code = base - 1 + ll0
                if code:
                    cur = rep[0] - 1 if code == 3 else rep[code]
                    rep = [cur, rep[0], rep[1] if code >= 2 else rep[2]]
        flat += [ll, ml, base, pos]
        pos += ll + ml
        lit += ll
    if not ext_rep and seqs:
        offs = [s[2] for s in seqs[-3:]][::-1]
        rep = (offs + rep)[:3]
    return flat, lit + tail, rep


def explain(got, want):
    """a difference, for the assertion's message: sizes, the first differing offset, walk() of both frames"""
    if isinstance(got, int):
        return f"error {got}"
    at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    def shape(frame):
        try:
            return S.walk(frame)
        except Exception as e:                                        # noqa: BLE001 (a frame too damaged to walk)
            return repr(e)
    return f"sizes {len(got)} / {len(want)}, first difference at {at}; got {shape(got)}; want {shape(want)}"


Case = namedtuple("Case", "family name seqs tail lits ext_rep")          # lits: "text" / "raw" / "rle" or the literal bytes themselves
Built = namedtuple("Built", "frame content shape rec nb lit_size last_ll")


def case(family, name, seqs, tail=0, lits="text", ext_rep=True):
    return Case(family, name, list(seqs), tail, lits, ext_rep)


def size_of(c):
    return sum(s[0] + s[1] for s in c.seqs) + c.tail


def levels_of(c):
    return (1, 3, 4, 5) if size_of(c) <= CHAIN_MAX else (1, 3)


_built = {}


def built(c, level):
    key = (c.family, c.name, level)
    if key not in _built:
        frame, content, shape = S.build([(c.seqs, c.tail)], level=level, literals=c.lits, seed=zlib.crc32(f"{c.family}/{c.name}".encode()), ext_rep=c.ext_rep)
        flat, lit_size, _ = records(c.seqs, c.tail, ext_rep=c.ext_rep)
        _built[key] = Built(frame, content, shape, flat, len(c.seqs), lit_size, c.tail)
    return _built[key]


def lit_size(c):
    return sum(s[0] for s in c.seqs) + c.tail


def text(n, seed=1):
    return S._literals(random.Random(seed), n, "text")


def ll_bits(ll): return S._ll_code(ll)[1]
def ml_bits(ml): return S._ml_code(ml)[1]
def of_code(base): return base.bit_length() - 1


def extra_bits(flat):
    """per sequence: (ll bits, ml bits, offset bits) — what ZSTD_encodeSequences' flush decisions are taken on"""
    return [(ll_bits(flat[i]), ml_bits(flat[i + 1]), of_code(flat[i + 2])) for i in range(0, len(flat), 4)]


def codes(flat):
    """per table: the code of every sequence, [LL, OF, ML] as walk()'s modes"""
    n = range(0, len(flat), 4)
    return [[S._ll_code(flat[i])[0] for i in n], [of_code(flat[i + 2]) for i in n], [S._ml_code(flat[i + 1])[0] for i in n]]


def bound_U(b):
    """(U, premises hold): zj_encode.h, the pipelined parse of ze_compress_multi_pipe (the `u64 const U64 = ...` line and `certain` behind it) without the
    destination's premise: 3 + litSize + 3 + 3 + 1 + 150 + ((26 nbSeq + extra + 26 + 15) >> 3) + 8, certain when the block has 7 bytes, a sequence,
    256 extra bits and U < blockSize - ((blockSize >> 6) + 2)."""
    extra = sum(sum(e) for e in extra_bits(b.rec))
    size = len(b.content)
    U = 3 + b.lit_size + 3 + 3 + 1 + 150 + ((26 * b.nb + extra + 26 + 15) >> 3) + 8
    return U, size >= 7 and b.nb >= 1 and extra >= 256 and U < size - ((size >> 6) + 2)


# ------------------------------------------------------------------------------------------------------------------------
def with_values(values, n, ml=4):
    """n sequences; sequence i has ll = values[i] where given, else 2 (the first one 330: history for every offset used)"""
    seqs, pos = [], 0
    for i in range(n):
        ll = values.get(i, 330 if i == 0 else 2)
        off = min(2 + i % 3, pos + ll)
        assert off >= 1, "a frame's first sequence needs a literal"
        seqs.append((ll, ml, off))
        pos += ll + ml
    return seqs


G_LL = (0, 1, 7, 8, 9, 63, 64, 65, 66, 200)
G_TAILS = (0, 1, 64, 4096)
G_SIZES = (4095, 4096, 4097, 65536, 65537)


def family_g():
    out = []
    for j, v in enumerate(G_LL):                                      # the value at every position of a pass (and the next pass's first ones); 65, 66, 200: twelve long runs, the ballot loop turns for each
        where = [p for p in POSITIONS if v or p]
        out.append(case("G", f"ll{v}", with_values({p: v for p in where}, 131), tail=G_TAILS[j % 4], ext_rep=bool(j % 2)))
    for count in (1, 63, 64, 65, 127, 128, 129):                      # record counts round the halves of a pass; the last record holds a run of 64 / 65
        out.append(case("G", f"count{count}", with_values({count - 1: 64 + count % 2, 0: 200}, count), tail=count % 3, ext_rep=bool(count % 2)))
    for r in range(1, 8):                                             # the last sequence's short run against the end of the source: its 8-byte load fits (r + 3 + tail >= 8) or not
        for tail in range(8):
            out.append(case("G", f"end/r{r}/t{tail}", with_values({19: 8 * (tail % 3) + r}, 20, ml=3), tail=tail))
    for t in G_TAILS:
        out.append(case("G", f"tail{t}", with_values({}, 40), tail=t, ext_rep=False))
    for n in G_SIZES:                                                 # the LDS-staged path's edge, the 16-bit / 32-bit build's edge
        seqs = with_values({3: 65, 70: 64}, 90)
        used = sum(s[0] + s[1] for s in seqs)
        half = (n - used) // 2
        seqs.append((half, n - used - half - 5, 3))
        out.append(case("G", f"size{n}", seqs, tail=5))
    return out


def histogram_bytes(counts, seed):
    v = [s for s, c in enumerate(counts) for _ in range(c)]
    random.Random(seed).shuffle(v)
    return bytes(v)


def spread_counts(n, top, symbols=256):
    """`symbols` values, sum n, the largest count exactly `top` (one value), the others level below it"""
    rest, k = n - top, symbols - 1
    counts = [top] + [rest // k + (1 if i < rest % k else 0) for i in range(k)]
    assert max(counts[1:]) < top and sum(counts) == n
    return counts


def lit_case(name, lits, nb=2, **kw):
    """a block whose literal section is exactly `lits`: nb short matches between the runs, 2 bytes of tail (sizes of 5 and less: 1 sequence)"""
    n = len(lits)
    nb = max(1, min(nb, (n - 2) // 2))
    tail = min(2, n - 1)
    each = (n - tail) // nb
    seqs = [(each + (n - tail - each * nb if i == 0 else 0), 4, 1 + i % 2) for i in range(nb)]
    return case("L", name, seqs, tail=tail, lits=bytes(lits), **kw)


L_SIZES = (5, 6, 63, 64, 255, 256, 1023, 1024, 16383, 16384)


def family_l():
    out = []
    for j, n in enumerate(L_SIZES):
        out.append(lit_case(f"size{n}", text(n, n), ext_rep=bool(j % 2)))
    flat = histogram_bytes([16] * 256, 3)                             # 4 096 bytes, every value 16 times: the sample's two ends give 32 <= 68
    for n in (40959, 40960):                                          # litSize / nbSeq >= 20: the sampling check runs (huf_compress.c:1369-1383)
        out.append(lit_case(f"sample/rejected/{n}", flat + text(n - 8192, n) + flat, nb=8))
        out.append(lit_case(f"sample/kept/{n}", text(n, n + 1), nb=8))
        out.append(lit_case(f"sample/skipped/{n}", flat + text(n - 8192, n) + flat, nb=n // 19))      # litSize / nbSeq < 20: no sample, the table is built
    out.append(lit_case("rle/300", b"q" * 300))
    out.append(lit_case("rle/70", b"q" * 70))
    out.append(lit_case("rle_but_one/300", b"q" * 150 + b"r" + b"q" * 149))
    out.append(lit_case("rle_but_one/first", b"r" + b"q" * 299))
    out.append(lit_case("rle_but_one/last", b"q" * 1299 + b"r"))
    for n in (1024, 4096, 16384):                                     # the largest count on "not compressible" 's bar and one above
        bar = (n >> 7) + 4
        few = 100 if n == 1024 else 128                               # (few enough values that a table would pay: above the bar the section is compressed)
        out.append(lit_case(f"largest/{n}/at", histogram_bytes(spread_counts(n, bar, few), n)))
        out.append(lit_case(f"largest/{n}/above", histogram_bytes(spread_counts(n, bar + 1, few), n + 1)))
    out.append(lit_case("two_symbols", histogram_bytes([700, 324], 5)))
    out.append(lit_case("two_symbols/far", histogram_bytes([700] + [0] * 254 + [324], 5)))
    out.append(lit_case("flat256", histogram_bytes([16] * 256, 6)))
    out.append(lit_case("geometric/14", histogram_bytes([1] + [1 << i for i in range(14)], 7)))                                   # natural depth 14: HUF_setMaxHeight repairs to 11
    out.append(lit_case("geometric/256", histogram_bytes([1 << max(0, 13 - i // 2) for i in range(28)] + [1] * 228, 8)))
    out.append(lit_case("fibonacci", histogram_bytes([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584], 9)))
    rnd = random.Random(11)
    out.append(lit_case("weights/120", histogram_bytes([1 << rnd.randrange(11) for _ in range(120)], 12)))                     # weights of every value: their tANS stream is the shorter description (direct 4-bit weights: largest/16384/above with 128 values, geometric/14, fibonacci)
    out.append(lit_case("weights/128", histogram_bytes([1 << rnd.randrange(11) for _ in range(128)], 13)))
    out.append(lit_case("weights/255/hard", histogram_bytes([1 << rnd.randrange(9) for _ in range(256)], 14)))                   # maxSymbol 255: only a tANS description exists
    out.append(lit_case("weights/255/easy", histogram_bytes([40] * 8 + [3] * 248, 15)))
    for n in (256, 257, 258, 259, 260):                               # four streams of 64 and of 65 with the last one 3 .. 0 bytes shorter
        out.append(lit_case(f"streams/{n}", text(n, 100 + n)))
    for name, data in equal_count_inputs():
        out.append(lit_case(f"equal/{name}", data, nb=4))
    return out


def count_seqs(n):
    return [(1, 3, 1)] + [(1, 3, 1 + (i * 7) % 4) for i in range(1, n)]


def family_s():
    out = [case("S", "count0", [], tail=500), case("S", "count0/raw", [], tail=500, lits="raw"), case("S", "count0/rle", [], tail=500, lits="rle")]
    for n in (1, 127, 128):
        out.append(case("S", f"count{n}", with_values({}, n), tail=n % 2, ext_rep=bool(n % 2)))
    for n in (0x7EFF, 0x7F00):                                        # the sequence count's two-byte and three-byte forms; the suite's largest blocks
        out.append(case("S", f"count{n}", count_seqs(n), tail=130049 - 4 * 0x7EFF if n == 0x7EFF else 130055 - 4 * 0x7F00))
    return out


def _m_codes(table, codes_, first_ll=40):
    """sequences whose codes in `table` (0 LL, 1 OF, 2 ML) are codes_ (the other two tables vary a little); ext_rep off: offBase = offset + 3"""
    seqs, pos = [], 0
    for i, c in enumerate(codes_):
        ll, ml, off = 1 + i % 3, 3 + i % 4, 5 + i % 3                 # LL codes 1-3, ML codes 0-3, OF code 3 (offBase 8 .. 10)
        if table == 0: ll = c if c < 16 else S.LL_BASE[c - 16]
        if table == 2: ml = c + 3 if c < 32 else S.ML_BASE[c - 32]
        if table == 1: off = (1 << c) - 3 + i % 2 if c > 2 else (1 << c) - 3 + 0
        if i == 0: ll = max(ll, first_ll)
        off = max(off, 1)
        if off > pos + ll:
            ll = off - pos                                            # history for the offset (the LL code under test is then not this one: callers put large codes late)
        seqs.append((ll, ml, off))
        pos += ll + ml
    return seqs


def _level_counts(n, codes_, top=None):
    """n codes drawn evenly from codes_; `top`: the first code that many times exactly and no other one as often"""
    if top is None:
        return [codes_[i % len(codes_)] for i in range(n)]
    rest = codes_[1:]
    out = [codes_[0]] * top + [rest[i % len(rest)] for i in range(n - top)]
    assert max(out.count(c) for c in rest) < top
    return out


M_MIN = {1: {0: 72, 1: 36, 2: 72}, 3: {0: 64, 1: 32, 2: 64}}          # dynamicFse_nbSeq_min = ((1 << defaultNormLog) * (10 - strategy)) >> 3 at levels 1 and 3 (fast, double-fast)
M_NAMES = ("LL", "OF", "ML")
M_SMALL = {0: [1, 2, 3, 4, 5], 1: [3, 4, 5, 6, 7], 2: [1, 2, 3, 4, 5]}


def family_m():
    out = []
    for n in (1, 2, 3):                                               # one code in every table: RLE, but the predefined tables for nbSeq <= 2
        out.append(case("M", f"rle/{n}", [(8, 4, 8)] + [(8, 4, 12)] * (n - 1), tail=300, ext_rep=False))     # (a tail worth compressing: the block must not end raw)
    out.append(case("M", "rle/100", [(8, 4, 8)] + [(8, 4, 12)] * 99, tail=1, ext_rep=False))
    for t in range(3):
        for level in (1, 3):                                          # one below and at dynamicFse_nbSeq_min (the most frequent code well above its bar)
            m = M_MIN[level][t]
            for n in (m - 1, m):
                seqs = _m_codes(t, _level_counts(n, M_SMALL[t], top=n // 2))
                out.append(case("M", f"min/{M_NAMES[t]}/L{level}/{n}", seqs, tail=2, ext_rep=False))
        for last in ("unique", "common"):                             # the last sequence's code occurs once / often: the count[last]-- of ZSTD_buildCTable
            cs = _level_counts(200, M_SMALL[t], top=90)
            cs = cs[:-1] + ([M_SMALL[t][-1] + 3] if last == "unique" else [M_SMALL[t][0]])
            out.append(case("M", f"last/{M_NAMES[t]}/{last}", _m_codes(t, cs), tail=2, ext_rep=False))
    # the most frequent code one below and at nbSeq >> (defaultNormLog - 1).  ML: 160 sequences, bar 5, forty codes four times each / one of them five times.
    ml40 = list(range(40))
    out.append(case("M", "most/ML/below", _m_codes(2, _level_counts(160, ml40)), tail=2, ext_rep=False))
    out.append(case("M", "most/ML/at", _m_codes(2, _level_counts(160, ml40, top=5)), tail=2, ext_rep=False))
    # OF: 272 sequences, bar 17, seventeen codes (offBase 1 .. 2^17 - 1) sixteen times each / one of them seventeen times
    out.append(case("M", "most/OF/below", _of_level(None), tail=2))
    out.append(case("M", "most/OF/at", _of_level(17), tail=2))
    return out


def _of_level(top):
    """272 sequences over the 17 offset codes 0 .. 16, sixteen times each (code 0: repcode 1, code 1: repcode 2, code c >= 2: offBase 2^c .. 2^(c + 1) - 1), with
    ext_rep on; `top`: code 5 that many times (one more than the others), code 6 once less"""
    b = S.Blk()
    b.add(70000, 4, 1)                                                # code 0: repcode 1 of the start history
    plan = []
    for r in range(16):
        plan += list(range(2, 17)) + [1] + ([0] if r else [])
    if top:
        plan[len(plan) - 1 - plan[::-1].index(6)] = 5
    for i, c in enumerate(plan):
        if c == 0: off = b.rep[0]
        elif c == 1: off = b.rep[1]
        else:
            cand = [o for o in range(max(1, (1 << c) - 3), (2 << c) - 3) if o not in b.rep]
            off = cand[(i // 17) % len(cand)]
        b.add(1, 3, off)
    return b.seqs


def family_w():
    out = []
    vals = S.code_values()
    for where in ("first", "middle", "last"):                         # sh.edge[]: the stream's first and last sequence are coded apart from the others
        for j, (kind, code, v) in enumerate(vals):
            fill = [(2, 4, 2 + i % 3) for i in range(70)]
            one = (v, 4, 1) if kind == "ll" else (2, v, 1)
            if where == "first":
                one = (max(one[0], 1), one[1], 1)
                seqs = [one] + fill
            elif where == "middle":
                seqs = [(9, 4, 2)] + fill[:33] + [one] + fill[33:]
            else:
                seqs = [(9, 4, 2)] + fill + [one]
            if j % 3 == ("first", "middle", "last").index(where) or v < 300:      # (every value at one place at least, the short ones everywhere)
                out.append(case("W", f"{kind}{code}/{v}/{where}", seqs, tail=j % 2, lits=("text", "raw")[j % 2], ext_rep=bool(j % 2)))
    for k in range(2, 18):                                            # offBase 2^k - 1, 2^k, 2^k + 1: the last value of code k - 1, the first two of code k
        for d in (-4, -3, -2):
            off = (1 << k) + d
            if off < 1 or off > 131000:
                continue
            for where in ("first", "last"):
                fill = [(2, 4, 2 + i % 3) for i in range(20)]
                lead = (max(off, 9), 4, off)
                seqs = [lead] + fill if where == "first" else [(max(off, 9), 4, 2)] + fill + [(1, 5, off)]
                out.append(case("W", f"of{k}/{d}/{where}", seqs, tail=1, ext_rep=False))
    out.append(case("W", "of17/-4/only", [(131068, 4, 131068)], tail=0, ext_rep=False))      # offBase 2^17 - 1, code 16's last value: the block is full
    # the flush decisions of ZSTD_encodeSequences are taken on extra bits: all three >= 64 - 7 - (9 + 9 + 8) = 31, ll + ml > 24.  The widest sequence a 128 KiB
    # block can hold: ll 32768 (15 bits) + ml 32771 (15) + offset 65537 (16) = 46 bits, 72 with the three state updates
    wide = [((32768, 32771, 65537), "46"), ((16384, 4099, 65537), "ll+ml26/42"), ((2048, 2051, 5), "ll+ml22"), ((4096, 2051, 5), "ll+ml23"), ((4096, 4099, 5), "ll+ml24"), ((8192, 4099, 5), "ll+ml25"),
            ((1024, 1027, 1021), "30"), ((1024, 2051, 1021), "31"), ((2048, 2051, 1021), "32")]
    for (ll, ml, off), name in wide:
        lead = max(off - ll, 0) + 9
        fill = [(2, 4, 2 + i % 3) for i in range(30)]
        out.append(case("W", f"wide/{name}/first", [(max(ll, off), ml, off)] + fill, tail=1, lits="raw", ext_rep=False))
        out.append(case("W", f"wide/{name}/middle", [(lead, 4, 2)] + fill[:15] + [(ll, ml, off)] + fill[15:], tail=1, lits="raw", ext_rep=False))
        out.append(case("W", f"wide/{name}/last", [(lead, 4, 2)] + fill + [(ll, ml, off)], tail=0, lits="raw", ext_rep=False))
    return out


def family_r():
    out = []
    for lane in S.LANES:                                              # every form in mid-block at every lane position, runs of the rep0 - 1 form included
        pats = [S._form(f) for f in S.FORMS] + [S._form("rep0m1_ll0", run) for run in S.RUNS]
        for i, (seqs, tail) in enumerate(S.pack(pats, lane)):
            out.append(case("R", f"lane{lane}/{i}", seqs, tail=tail, lits=("text", "raw")[i % 2]))
    for f, seq in (("rep0", (3, 4, 1)), ("rep1", (5, 4, 4)), ("rep2", (9, 4, 8))):      # the frame's first sequence against the start history 1, 4, 8 (a form with ll = 0 has nothing to copy there)
        out.append(case("R", f"first/{f}", [seq] + [(2, 4, 2 + i % 3) for i in range(10)], tail=1))
        out.append(case("R", f"first/{f}/off", [seq] + [(2, 4, 2 + i % 3) for i in range(10)], tail=1, ext_rep=False))
    return out


B_SHARES = tuple(range(0, 1025, 32))
B_EDGE = tuple(range(3, 60))


def family_b():
    out = []
    for n, nb in ((2000, 10), (12000, 20)):                          # text literals with a growing share of random bytes at fixed sequences: the block's size passes through srcSize - minGain
        rnd = random.Random(n)
        base, noise = text(n, n), rnd.randbytes(n)
        order = list(range(n))
        rnd.shuffle(order)
        for share in B_SHARES:
            lits = bytearray(base)
            for k in order[:n * share // 1024]:
                lits[k] = noise[k]
            out.append(lit_case(f"sweep/{n}/{share}", bytes(lits), nb=nb)._replace(family="B"))
    # raw literals and ten sequences, the last match one byte longer each time (19 .. 34: codes of one price in the predefined table): the source grows, the
    # compressed size stays, so srcSize - minGain walks over it one byte at a time and the block turns compressed exactly where cSize < srcSize - minGain first holds
    c = lit_case("edge", random.Random(77).randbytes(2000), nb=10)._replace(family="B")
    for ml in B_EDGE:
        out.append(c._replace(name=f"edge/{ml}", seqs=c.seqs[:-1] + [(c.seqs[-1][0], ml, c.seqs[-1][2])]))
    for n in range(1, 8):                                             # below ZSTD_buildSeqStore's 7 bytes nothing is compressed
        out.append(case("B", f"tiny/{n}", [], tail=n))
        out.append(case("B", f"tiny/{n}/rle", [], tail=n, lits="rle"))
    out.append(case("B", "tiny/7/seq", [(1, 6, 1)], tail=0))
    out.append(case("B", "tiny/8/seq", [(1, 6, 1)], tail=1))
    return out


def family_u():
    """blocks built to come close to the bound: raw-grade literals, every code present with uneven counts (the largest table descriptions), wide sequences"""
    rnd = random.Random(5)
    b = S.Blk()
    b.add(66000, 3, 1)
    for i in range(2600):
        c = rnd.randrange(2, 17)
        off = (1 << c) - 3 + rnd.randrange(1 << c)
        ll = rnd.choice(tuple(range(16)) + (16, 18, 21, 23, 25, 30, 35, 45, 50, 70, 130, 260, 520) if i % 50 else (1030, 2050))
        ml = rnd.choice(list(range(3, 36)) + [37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131] + ([259, 515] if i % 40 == 0 else []))
        if b.pos + ll + ml > 130000:
            break
        b.add(ll, ml, max(1, min(off, b.pos + ll)))
    out = [case("U", "all_codes/raw", b.seqs, tail=3, lits="raw"), case("U", "all_codes/text", b.seqs, tail=3, lits="text", ext_rep=False)]
    wide = [(16384, 16387, 1)] + [(3, 8195 + 100 * i, 30000 + i) for i in range(10)]
    out.append(case("U", "wide", wide, tail=0, lits="raw", ext_rep=False))
    return out


def _code_values(ll_codes, ml_codes):
    """one sequence per pair of codes: the smallest literal length and match length of each code, offsets 1 .. 9 within what lies before them"""
    seqs, pos = [], 0
    for i, (l, m) in enumerate(zip(ll_codes, ml_codes)):
        ll, ml = l if l < 16 else S.LL_BASE[l - 16], m + 3 if m < 32 else S.ML_BASE[m - 32]
        assert pos + ll >= 1, "a frame's first sequence needs a literal"
        seqs.append((ll, ml, min(1 + (5 * i) % 9, pos + ll)))
        pos += ll + ml
    return seqs


def _shuffled(codes_, seed):
    """a fixed shuffle whose first code is not 0"""
    out = list(codes_)
    random.Random(seed).shuffle(out)
    k = next(i for i, c in enumerate(out) if c)
    return out[k:] + out[:k]


def _without(top, absent):
    return [c for c in range(top + 1) if c not in absent]


def family_n():
    """the two ways out of the table normalisation that no parse of text reaches (branch_cases.tans_histograms; ze_tans_shares_rare's `settled == n` and `left == 0`):
    22, 43 and 44 sequences with every code of a table exactly once, without and with absent codes below the largest.  At level 5 (lazy to 16 KiB) every
    table is normalised for the cost estimate (ZSTD_NCountCost) whichever mode wins; below lazy so few sequences take the predefined tables unseen, and
    the frames are the plain regression they are for every family.  The offset alphabet cannot take part: 22 different offset codes need an offset of 2 MiB, and the
    records hold offBase in 24 bits beside its code, so no code above 23 exists here (the entries refuse offsets beyond the window before the stage sees them).
    The conditions are asserted in tests/test_emu_seqrecords.py."""
    out = []

    def n_case(name, ll, ml, seed):
        out.append(case("N", name, _code_values(_shuffled(ll, seed), _shuffled(ml, seed + 1)), tail=300, ext_rep=bool(seed % 2)))
    n_case("22/settled", range(22), range(22), 1)                                        # LL 22 of 22, ML 22 of 22 at table log 5
    n_case("22/gaps", _without(31, (0, 3, 4, 9, 13, 14, 20, 25, 26, 30)), _without(47, (1, 2, 5, 6, 7, 10, 11, 12, 15, 16, 17, 18, 19, 21, 22, 23, 28, 29, 33, 34, 35, 40, 41, 42, 45, 46)), 4)
    ll_many = [i % 20 for i in range(44)]                                                # (36 literal-length codes: 43 cannot all differ)
    n_case("43/settled", ll_many[:43], range(43), 7)                                     # ML 43 of 43 at table log 6
    n_case("44/settled", ll_many, range(44), 10)
    n_case("44/gaps", ll_many, _without(47, (0, 9, 20, 41)), 13)                         # ML 44 of 48
    n_case("43/gaps", ll_many[:43], _without(45, (3, 17, 33)), 16)                       # ML 43 of 46
    return out


# ------------------------------------------------------------------------------------------------------------------------
# frames of several caller-cut blocks: the state the entropy stage carries from block to block (the previous Huffman table, the previous tANS tables, and — through
# the records — the repcodes, which only a compressed block confirms)
MCase = namedtuple("MCase", "family name blocks lits ext_rep")          # blocks = [(seqs, tail), ...]; lits: the frame's literal bytes, or a kind
MBuilt = namedtuple("MBuilt", "frame content shape rec blk")            # rec: the records of all blocks in order; blk: [size, nbSeq, litSize, lastLL] per block


def mcase(family, name, parts, ext_rep=True):
    """parts = [(seqs, tail, literal bytes of the block), ...]"""
    for seqs, tail, lits in parts:
        assert len(lits) == sum(q[0] for q in seqs) + tail, name
    return MCase(family, name, [(list(p[0]), p[1]) for p in parts], b"".join(p[2] for p in parts), ext_rep)


_mbuilt = {}


def mbuilt(c, level):
    key = (c.family, c.name, level)
    if key not in _mbuilt:
        frame, content, shape = S.build(c.blocks, level=level, literals=c.lits, seed=zlib.crc32(f"{c.family}/{c.name}".encode()), ext_rep=c.ext_rep)
        rep, rec, blk = (1, 4, 8), [], []
        assert len(shape["blocks"]) == len(c.blocks), "the reference cut the blocks otherwise"
        for (seqs, tail), k in zip(c.blocks, shape["blocks"]):
            flat, lit, after = records(seqs, tail, reps=rep, ext_rep=c.ext_rep)
            if k["type"] == 2:                                        # ZSTD_blockState_confirmRepcodesAndEntropyTables: a raw or RLE block leaves the history as it was
                rep = after
            rec += flat
            blk += [sum(q[0] + q[1] for q in seqs) + tail, len(seqs), lit, tail]
        _mbuilt[key] = MBuilt(frame, content, shape, rec, blk)
    return _mbuilt[key]


def msize(c):
    return sum(q[0] + q[1] for seqs, tail in c.blocks for q in seqs) + sum(t for _, t in c.blocks)


def mlevels(c):
    """levels 1 and 3: the library writes frames of several blocks at levels 1 to 3 only (above them a frame is one block of at most 128 KiB), and the block path of
    ze_compress_t restates the literal and table decisions of the strategies below lazy"""
    return (1, 3)


def block_bounds(b):
    """[(U, premises hold, the block's shape)] of every block of a frame of several blocks (bound_U's formula)"""
    out, at = [], 0
    for i, k in enumerate(b.shape["blocks"]):
        size, nb, lit, _ = b.blk[4 * i:4 * i + 4]
        flat = b.rec[at:at + 4 * nb]
        at += 4 * nb
        extra = sum(sum(e) for e in extra_bits(flat))
        U = 3 + lit + 3 + 3 + 1 + 150 + ((26 * nb + extra + 26 + 15) >> 3) + 8
        out.append((U, size >= 7 and nb >= 1 and extra >= 256 and U < size - ((size >> 6) + 2), k))
    return out


def _part(n_lit, seed, nb=30, letters=None, ml=4):
    """a block of nb short matches between n_lit text literals (2 in the tail); letters: another alphabet"""
    nb = max(1, min(nb, (n_lit - 2) // 2))
    each = (n_lit - 2) // nb
    seqs = [(each + (n_lit - 2 - each * nb if i == 0 else 0), ml, 1 + i % 2) for i in range(nb)]
    lits = text(n_lit, seed)
    if letters:
        lits = lits.translate(bytes(letters[LETTER_AT.get(x, 0) % len(letters)] for x in range(256)))
    return (seqs, 2, lits)


def _varied(seed, n=300):
    rnd = random.Random(seed)
    b = S.Blk()
    b.add(60, 5, 7)
    for _ in range(n):
        ll = rnd.choice((0, 1, 1, 2, 3, 4, 5, 6, 8, 11, 17, 20))
        b.add(ll, rnd.choice((3, 3, 4, 4, 5, 6, 7, 9, 12, 20, 36)), rnd.randrange(1, min(300, b.pos + ll) + 1))
    return (b.seqs, 3, text(sum(q[0] for q in b.seqs) + 3, seed))


LETTER_AT = {x: i for i, x in enumerate(S.LETTERS)}
P_PREFER = (1023, 1024, 1025, 1026)


def _skewed(n, seed):
    """the eight letters of text() with very uneven counts: the table a flat block left is valid for them and clearly worse than their own"""
    return histogram_bytes([n - 7 * (n // 64)] + [n // 64] * 7, seed).translate(bytes(S.LETTERS[x % 8] for x in range(256)))


def family_p():
    out = []
    A = _part(3000, 1)
    out.append(mcase("P", "twice", [A, A]))                           # the same statistics again: the previous Huffman table without a description, the previous tANS tables where the level weighs them
    out.append(mcase("P", "thrice_then_new_symbol", [A, A, A, _part(3000, 2, letters=b"etaoinsX")]))     # ... and a block with one value more: the old table cannot serve it
    V = _varied(11)
    out.append(mcase("P", "twice/varied", [V, V, _varied(12)]))       # many codes in every table
    out.append(mcase("P", "four", [A, _part(2000, 3, nb=100), _part(5000, 4, nb=10), A], ext_rep=False))
    for n in P_PREFER:                                                # HUF_flags_preferRepeat: to 1024 bytes a usable previous table is taken unseen, above it only if it is no worse
        seqs = [(n - 2, 4, 1)]
        out.append(mcase("P", f"prefer/{n}", [A, (seqs, 2, _skewed(n, n))]))
    rnd = random.Random(9)
    raw = ([], 700, rnd.randbytes(700))
    rle = ([(1, 299, 1)], 0, b"e")                                    # (one byte throughout, fewer than 4 sequences and 10 literals: ZSTD_maybeRLE — the sequence interface's rule, which the block
                                                                      # compressor's "compressed size below 25" covers; an all-literal run of one byte is an RLE block only for the latter, so it is no case here)
    out.append(mcase("P", "raw_between", [A, raw, A]))
    out.append(mcase("P", "rle_between", [A, rle, A, A]))
    for n in (5, 6, 63, 64):                                          # short literal sections behind a block that left a table
        out.append(mcase("P", f"short/{n}", [A, ([(n - 2, 40, 3)], 2, text(n, n)), A]))
    big = _part(70000, 5, nb=3000)
    out.append(mcase("P", "large", [big, big, _part(70000, 6, nb=200)]))       # above 128 KiB in all: the header this route writes is the reference's
    return out


def family_rb():
    """R and B in frames of several blocks: every repcode form as the first sequence behind a raw block, an RLE block and a block without sequences (none of which
    confirms the repcodes the block before them left), and an all-one-byte block first and later (only a later one may become an RLE block)"""
    out = []
    for c in S.family("E"):
        if c.name.startswith("first/") and c.name.endswith("/L3"):
            out.append(MCase("R", "multi/" + c.name[:-3], c.blocks, "text", True))
            out.append(MCase("R", "multi/" + c.name[:-3] + "/off", c.blocks, "raw", False))
    A = _part(1500, 7)
    nine = ([], 9, b"e" * 9)
    out.append(mcase("B", "multi/rle_block_nine", [A, nine, A]))
    out.append(mcase("B", "multi/rle_block_nine_first", [nine, A]))
    out.append(mcase("B", "multi/rle_block_last", [A, ([(1, 199, 1)], 0, b"e")]))
    out.append(mcase("B", "multi/rle_block_with_match", [A, ([(1, 199, 1)], 0, b"e"), A]))
    out.append(mcase("B", "multi/rle_block_with_match_first", [([(1, 199, 1)], 0, b"e"), A]))
    return out


MFAMILIES = {"P": family_p, "RB": family_rb}
_mcases = {}


def mfamily(name):
    if name not in _mcases:
        _mcases[name] = MFAMILIES[name]()
        names = [c.name for c in _mcases[name]]
        assert len(set(names)) == len(names), "two cases of one name"
    return _mcases[name]


FAMILIES = {"G": family_g, "L": family_l, "S": family_s, "M": family_m, "W": family_w, "R": family_r, "B": family_b, "U": family_u, "N": family_n}
_cases = {}


def family(name):
    if name not in _cases:
        _cases[name] = FAMILIES[name]()
        names = [c.name for c in _cases[name]]
        assert len(set(names)) == len(names), "two cases of one name"
    return _cases[name]


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
