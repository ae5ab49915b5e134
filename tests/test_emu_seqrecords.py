"""CPU (-m "not gpu"): the encoder's entropy stage on hand-written sequences (tests/seqrecords.py) through the lane-serial emulation's
emu_compress_records — ze_compress with `pre`, as zj_encode_kernel runs it in mode 0 — with and without the LDS-staged path of frames to 4 KiB.
The expected bytes are the frame the reference's ZSTD_compressSequences writes for the same triples (seqframes.build, confirmed by the
reference's decoder).  The conditions on the inputs — which branch of the stage each family really reaches — are asserted here from the
reference's frames (walk()) and from the records, so that a later edit of the generators cannot hollow a family out; the same cases meet the
wave64 code in tests/test_gpu_seqrecords.py.

test_bound_of_the_pipelined_parse: the smallest margin U - (block size with header) seen over all families at levels 1 and 3 is 178 bytes
(U/wide at levels 1 and 3: one literal run and eleven long matches; 44 blocks meet the premises, later blocks of frames of several blocks among them); measured, not asserted — the assertion is margin >= 0 wherever the premises hold."""
import ctypes as C

import pytest

import seqframes as S
import seqrecords as R
from util import emu_lib

NO_STAGE = 0x800               # emu_compress_records: the launch's LDS holds the entropy stage only (frames to 4 KiB are not staged)


@pytest.fixture(scope="module")
def emu():
    L = emu_lib()
    L.emu_compress_records.restype = C.c_ulonglong
    L.emu_compress_records.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint), C.c_uint, C.c_uint, C.c_uint, C.c_char_p, C.c_uint, C.c_uint]
    L.emu_compress_records_blocks.restype = C.c_ulonglong
    L.emu_compress_records_blocks.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_uint, C.c_char_p, C.c_uint, C.c_uint]
    return L


def compress_records(L, b, levelword):
    rec = (C.c_uint * max(len(b.rec), 1))(*b.rec)
    cap = len(b.content) + (len(b.content) >> 7) + 512
    dst = C.create_string_buffer(cap)
    r = L.emu_compress_records(b.content, len(b.content), rec, b.nb, b.lit_size, b.last_ll, dst, cap, levelword)
    return dst.raw[:r] if r < (1 << 63) else -((1 << 64) - r)


def compress_blocks(L, b, levelword):
    rec = (C.c_uint * max(len(b.rec), 1))(*b.rec)
    blk = (C.c_uint * len(b.blk))(*b.blk)
    cap = len(b.content) + (len(b.content) >> 7) + 512 + 4 * len(b.blk)
    dst = C.create_string_buffer(cap)
    r = L.emu_compress_records_blocks(b.content, len(b.content), rec, blk, len(b.blk) // 4, dst, cap, levelword)
    return dst.raw[:r] if r < (1 << 63) else -((1 << 64) - r)


PIPE_HEADER = 9                # what the pipelined route's entropy role writes: magic, descriptor, a 4-byte content size (its frames are above 128 KiB)


@pytest.mark.parametrize("name", list(R.MFAMILIES))
def test_frames_of_several_blocks_are_the_references(emu, oracle_ref, name):
    """the reference writes a shorter content size for a frame below 65 792 bytes, which that route never meets: such frames are compared from the first block header on"""
    whole = 0
    for c in R.mfamily(name):
        for level in R.mlevels(c):
            b = R.mbuilt(c, level)
            got = compress_blocks(emu, b, level)
            assert not isinstance(got, int), (c.family, c.name, level, got)
            hdr = b.shape["header"]
            whole += hdr == PIPE_HEADER
            want = b.frame if hdr == PIPE_HEADER else got[:PIPE_HEADER] + b.frame[hdr:]          # (the emulation's own header in front of the reference's blocks)
            assert got == want, (c.family, c.name, level, R.explain(got, want))
    assert whole or name != "P"


@pytest.mark.parametrize("name", list(R.FAMILIES))
def test_family_is_the_references_frame(emu, oracle_ref, name):
    for c in R.family(name):
        for level in R.levels_of(c):
            b = R.built(c, level)
            for word in (level, level | NO_STAGE) if len(b.content) <= 4096 else (level,):
                got = compress_records(emu, b, word)
                assert got == b.frame, (c.family, c.name, hex(word), R.explain(got, b.frame))


def test_refuses_more_records_than_a_slot_holds(emu):
    rec = (C.c_uint * 4)(1, 3, 1, 0)
    dst = C.create_string_buffer(1024)
    assert emu.emu_compress_records(b"a" * 100, 100, rec, 65536 // 4 + 17, 1, 0, dst, 1024, 3) >= 1 << 63
    wide = (C.c_uint * 4)(4, 4, 1 << 24, 0)                          # an offBase that does not fit beside its code in the record
    assert emu.emu_compress_records(b"abcdefgh" * 8, 64, wide, 1, 60, 56, dst, 1024, 3) >= 1 << 63


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs


def blocks_of(name, levels=None):
    for c in R.family(name):
        for level in levels or R.levels_of(c):
            if level in R.levels_of(c):
                yield c, level, R.built(c, level)


def the(name, cname):
    return next(c for c in R.family(name) if c.name == cname)


def blk(c, level):
    return R.built(c, level).shape["blocks"][0]


def test_family_g_holds_its_runs(oracle_ref):
    G = R.family("G")
    for v in R.G_LL:
        c = the("G", f"ll{v}")
        at = {i for i, s in enumerate(c.seqs) if s[0] == v}
        assert at >= {p for p in R.POSITIONS if v or p}, (v, sorted(at))
        if v > 64:
            assert sum(1 for s in c.seqs[:64] if s[0] > 64) >= 2      # several long runs in one half pass: the ballot loop turns more than once
    assert {len(c.seqs) for c in G} >= {1, 63, 64, 65, 127, 128, 129}
    fits = set()
    for c in G:
        if c.name.startswith("end/"):
            ll = c.seqs[-1][0]
            assert 0 < ll % 8 and c.seqs[-1][1] == 3
            fits.add((ll % 8) + 3 + c.tail - 8)                        # >= 0: the last run's 8-byte load ends inside the source
    assert {-4, -1, 0, 1} <= fits
    assert {c.tail for c in G} >= set(R.G_TAILS)
    assert {R.size_of(c) for c in G} >= set(R.G_SIZES)
    assert all(blk(c, 3)["type"] == 2 for c in G)


def test_family_l_holds_its_literal_sections(oracle_ref):
    L = R.family("L")
    assert {R.lit_size(c) for c in L} >= set(R.L_SIZES) | {40959, 40960, 256, 257, 258, 259, 260}
    for c, level, b in blocks_of("L"):
        k = b.shape["blocks"][0]
        if k["type"] == 2:
            assert k["lit_size"] == R.lit_size(c)
    lit = lambda cname, level=3: blk(the("L", cname), level).get("lit_type", 0)       # 0 raw (or the whole block is), 1 RLE, 2 compressed, 3 treeless
    for n in (40959, 40960):                                          # the sample runs from 40 960 bytes on, and rejects what a table serves one byte below and with more sequences
        assert lit(f"sample/rejected/{n}") == (0 if n == 40960 else 2) and lit(f"sample/kept/{n}") == 2 and lit(f"sample/skipped/{n}") == 2
    assert lit("rle/300") == 1 and lit("rle/70") == 1 and lit("rle_but_one/300") == 2 and lit("rle_but_one/last") == 2
    for n in (1024, 4096, 16384):
        assert lit(f"largest/{n}/at") == 0 and lit(f"largest/{n}/above") == 2, n
    assert lit("size63") == 0 and lit("size64") == 2 and lit("size5") == 0 and lit("size6") == 0
    assert lit("flat256") == 0 and lit("two_symbols") == 2 and lit("geometric/14") == 2 and lit("fibonacci") == 2
    assert lit("weights/120") == 2 and lit("weights/128") == 2 and lit("weights/255/easy") == 2 and lit("weights/255/hard") == 2
    for cname, direct in (("largest/16384/above", True), ("geometric/14", True), ("fibonacci", True), ("weights/120", False), ("weights/128", False), ("weights/255/easy", False), ("weights/255/hard", False)):
        b = R.built(the("L", cname), 3)
        k = b.shape["blocks"][0]
        body = b.frame[k["end"] - k["size"]:]
        hdr = 3 + (k["lit_size"] >= 1024) + (k["lit_size"] >= 16384)
        assert (body[hdr] >= 128) == direct, (cname, body[hdr])       # the tree description's first byte: >= 128 direct 4-bit weights, < 128 the size of their tANS stream
    assert sum(blk(c, 3).get("lit_type") == 2 for c in L if c.name.startswith("equal/")) >= 5


def test_family_s_holds_its_counts(oracle_ref):
    want = {"count0": 0, "count1": 1, "count127": 127, "count128": 128, "count32511": 0x7EFF, "count32512": 0x7F00}
    for cname, n in want.items():
        c = the("S", cname)
        for level in R.levels_of(c):
            k = blk(c, level)
            assert k["type"] == 2 and k["nbSeq"] == n, (cname, level, k)
    assert R.size_of(the("S", "count32511")) == 130049 and R.size_of(the("S", "count32512")) == 130055


def test_family_m_sits_on_the_bars(oracle_ref):
    mode = lambda cname, level, t: blk(the("M", cname), level)["modes"][t]
    seen = [set(), set(), set()]
    for c, level, b in blocks_of("M", (1, 3)):
        k = b.shape["blocks"][0]
        assert k["type"] == 2, (c.name, level)
        for t in range(3):
            seen[t].add(k["modes"][t])
    assert all(s >= {0, 1, 2} for s in seen), seen
    for level in (1, 3):
        assert blk(the("M", "rle/1"), level)["modes"] == [0, 0, 0] and blk(the("M", "rle/2"), level)["modes"] == [0, 0, 0]      # the nbSeq <= 2 exception
        assert blk(the("M", "rle/3"), level)["modes"] == [1, 1, 1] and blk(the("M", "rle/100"), level)["modes"] == [1, 1, 1]
        for t in range(3):
            m = R.M_MIN[level][t]
            assert mode(f"min/{R.M_NAMES[t]}/L{level}/{m - 1}", level, t) == 0 and mode(f"min/{R.M_NAMES[t]}/L{level}/{m}", level, t) == 2, (level, t)
        assert mode("most/ML/below", level, 2) == 0 and mode("most/ML/at", level, 2) == 2
        assert mode("most/OF/below", level, 1) == 0 and mode("most/OF/at", level, 1) == 2
    for cname, t, most in (("most/ML/below", 2, 4), ("most/ML/at", 2, 5), ("most/OF/below", 1, 16), ("most/OF/at", 1, 17)):      # one below and at nbSeq >> (defaultNormLog - 1)
        cs = R.codes(R.built(the("M", cname), 3).rec)[t]
        assert max(cs.count(x) for x in set(cs)) == most and len(cs) >> (5 if t == 2 else 4) == (5 if t == 2 else 17), cname
    for t in range(3):
        for last, n in (("unique", 1), ("common", 90)):
            b = R.built(the("M", f"last/{R.M_NAMES[t]}/{last}"), 3)
            cs = R.codes(b.rec)[t]
            assert cs.count(cs[-1]) >= n and (n > 1 or cs.count(cs[-1]) == 1) and b.shape["blocks"][0]["modes"][t] == 2
    # levels 4 and 5 choose by cost: the same inputs, and a table on which they decide otherwise than level 3's bars
    differ = [(c.name, level) for c, level, b in blocks_of("M", (4, 5)) if b.shape["blocks"][0]["modes"] != blk(c, 3)["modes"]]
    assert differ, "the cost-based branch never decided anything"


def test_family_w_holds_its_codes(oracle_ref):
    W = R.family("W")
    ll, ml, of = set(), set(), set()
    edge = {"first": set(), "last": set(), "middle": set()}
    for c in W:
        rec, _, _ = R.records(c.seqs, c.tail, ext_rep=c.ext_rep)
        ex = R.extra_bits(rec)
        for i, s in enumerate(c.seqs):
            ll.add(s[0]); ml.add(s[1]); of.add(rec[4 * i + 2])
            where = "first" if i == 0 else ("last" if i == len(c.seqs) - 1 else "middle")
            edge[where].add((sum(ex[i]) >= 31, ex[i][0] + ex[i][1] > 24))
    for kind, code, v in S.code_values():
        assert v in (ll if kind == "ll" else ml), (kind, code, v)
    for k in range(2, 17):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= of, k
    assert (1 << 17) - 1 in of
    for where, flags in edge.items():                                 # both flush decisions taken and not taken at the stream's first, inner and last sequence
        assert flags >= {(True, True), (False, False)}, (where, flags)
    sums = {sum(e) for c in W if c.name.startswith("wide/") for e in R.extra_bits(R.records(c.seqs, c.tail, ext_rep=False)[0])}
    assert {30, 31, 32, 46} <= sums
    # in bits taken from the stream (seq_bits()' count: extra bits and the three state updates): on the predefined tables the widest sequence's codes (LL 34, OF 16,
    # ML 51) are of probability 1 or "less than 1", a cell of nbBits = tableLog each, so it takes 46 + 6 + 5 + 6 = 63 >= 57 bits wherever it is not the last; 65 needs
    # described tables (up to 9 + 8 + 9 state bits: 72), which the cases with many sequences around it have
    for where in ("first", "middle"):                                 # (as the stream's first sequence its literal run is 65 537 bytes: LL code 35, one bit more)
        c = the("W", f"wide/46/{where}")
        for level in (1, 3) if where == "first" else (1,):            # (32 sequences: at level 3 the offset table of the middle case is described)
            assert blk(c, level)["modes"] == [0, 0, 0], (where, level)
        ll, of, ml = R.codes(R.records(c.seqs, c.tail, ext_rep=False)[0])
        i = next(i for i, e in enumerate(R.extra_bits(R.records(c.seqs, c.tail, ext_rep=False)[0])) if sum(e) >= 46)
        assert abs(S.LL_DEF[ll[i]]) == 1 and abs(S.OF_DEF[of[i]]) == 1 and abs(S.ML_DEF[ml[i]]) == 1 and i + 1 < len(c.seqs) and 46 + 6 + 5 + 6 >= 57
    pairs = {e[0] + e[1] for c in W if c.name.startswith("wide/") for e in R.extra_bits(R.records(c.seqs, c.tail, ext_rep=False)[0])}
    assert {23, 24, 25, 26, 30} <= pairs


def test_family_r_holds_every_form(oracle_ref):
    lanes = {f: set() for f in S.FORMS}
    for c in R.family("R"):
        rep = [1, 4, 8]
        rec, _, _ = R.records(c.seqs, c.tail, ext_rep=c.ext_rep)
        for i, (l, m, off) in enumerate(c.seqs):
            form, rep = S.classify(off, l, rep)
            if form != "off":
                lanes[form].add(i % 64)
                if c.ext_rep:
                    assert rec[4 * i + 2] == {"rep0": 1, "rep1": 2, "rep2": 3, "rep1_ll0": 1, "rep2_ll0": 2, "rep0m1_ll0": 3}[form]      # the two restatements agree
            if not c.ext_rep:
                assert rec[4 * i + 2] == off + 3
    for f in S.FORMS:
        S.spread(lanes[f], f, lowest=0 if f in ("rep0", "rep1", "rep2") else min(lanes[f]))


def test_family_b_passes_through_the_raw_decision(oracle_ref):
    for n in (2000, 12000):
        for level in (1, 3):
            types = [blk(the("B", f"sweep/{n}/{share}"), level)["type"] for share in R.B_SHARES]
            assert set(types) == {0, 2}, (n, level, types)
            assert any(a != b for a, b in zip(types, types[1:]))
    for level in (1, 3, 4, 5):                                        # the edge sweep lands ON the bar: one flip, and the first compressed block is one byte below srcSize - minGain
        edge = [(len(R.built(the("B", f"edge/{ml}"), level).content), blk(the("B", f"edge/{ml}"), level)) for ml in R.B_EDGE]
        flips = [i for i in range(1, len(edge)) if edge[i][1]["type"] != edge[i - 1][1]["type"]]
        assert len(flips) == 1 and edge[0][1]["type"] == 0, (level, flips)
        n, k = edge[flips[0]]
        assert k["size"] == n - ((n >> 6) + 2) - 1, (level, n, k["size"])
    for n in range(1, 7):
        assert blk(the("B", f"tiny/{n}"), 3)["type"] == 0
    assert blk(the("B", "tiny/7/rle"), 3)["type"] == 0 and blk(the("B", "tiny/3/rle"), 3)["type"] == 0      # a frame's first block never becomes an RLE block


def mblocks(level, cname):
    c = next(c for f in R.MFAMILIES for c in R.mfamily(f) if c.name == cname)
    return R.mbuilt(c, level).shape["blocks"]


def test_frames_of_several_blocks_carry_state(oracle_ref):
    lit = lambda level, cname: [k.get("lit_type") for k in mblocks(level, cname)]
    types = lambda level, cname: [k["type"] for k in mblocks(level, cname)]
    for level in (1, 3):
        assert lit(level, "twice") == [2, 3] and lit(level, "thrice_then_new_symbol") == [2, 3, 3, 2]          # treeless while the table serves, a new one for the new value
        assert types(level, "raw_between") == [2, 0, 2] and lit(level, "raw_between")[2] == 3                 # the table outlives a raw block
        assert types(level, "rle_between") == [2, 1, 2, 2] and lit(level, "rle_between")[2:] == [3, 3]         # ... and an RLE block
        # ZSTD_minLiteralsToCompress is 6 only behind a VALID table, which a dictionary leaves; behind a block's table (to be CHECKed) it stays 64: 5, 6 and 63 bytes raw
        assert [lit(level, f"short/{n}")[1] for n in (5, 6, 63, 64)] == [0, 0, 0, 3], level
        assert types(level, "multi/rle_block_with_match") == [2, 1, 2] and types(level, "multi/rle_block_nine") == [2, 1, 2] and types(level, "multi/rle_block_last") == [2, 1]
        assert types(level, "multi/rle_block_with_match_first")[0] != 1 and types(level, "multi/rle_block_nine_first")[0] != 1      # never the frame's first block
        assert len(mblocks(level, "four")) == 4 and len(mblocks(level, "twice/varied")) == 3
        # HUF_flags_preferRepeat (strategy < lazy): the previous table unseen to 1024 bytes, its own table above
        assert [lit(level, f"prefer/{n}")[1] for n in R.P_PREFER] == [3, 3, 2, 2], level
        # a tANS table is repeated (mode 3) below the lazy strategies only when it is VALID, which only a dictionary makes it (ZSTD_selectEncodingType): without one
        # the previous tables must never be chosen, whatever the statistics — "twice/varied" offers them
        modes = [k["modes"] for f in R.MFAMILIES for c in R.mfamily(f) for k in R.mbuilt(c, level).shape["blocks"] if k["modes"]]
        assert modes and not any(3 in m for m in modes)
        assert all(2 in k["modes"] for k in mblocks(level, "twice/varied"))
    forms = {c.name.split("/")[2] for c in R.mfamily("RB") if c.family == "R"}
    assert forms == set(S.FORMS)
    for c in R.mfamily("RB"):                                         # every form behind a raw block, an RLE block and a block without sequences
        if c.family == "R" and c.ext_rep:
            seen = [(k["type"], k["nbSeq"]) for k in R.mbuilt(c, 3).shape["blocks"]]
            assert any(t[0] == 0 for t in seen) and any(t[0] == 1 for t in seen) and any(t == (2, 0) for t in seen), (c.name, seen)


def test_bound_of_the_pipelined_parse(oracle_ref):
    """where the premises of `certain` hold (zj_encode.h, the pipelined parse) the reference's block is compressed and, with its header, at most U"""
    smallest, held = None, 0
    for name in R.FAMILIES:
        for c, level, b in blocks_of(name, (1, 3)):
            U, certain = R.bound_U(b)
            k = b.shape["blocks"][0]
            if certain:
                held += 1
                assert k["type"] == 2 and k["size"] + 3 <= U, (c.family, c.name, level, k["type"], k["size"] + 3, U)
                if smallest is None or U - k["size"] - 3 < smallest[0]:
                    smallest = (U - k["size"] - 3, c.family, c.name, level)
    later = 0
    for f in R.MFAMILIES:                                             # ... and every block of the frames of several blocks: previous tables, repcodes carried in
        for c in R.mfamily(f):
            for level in (1, 3):
                for i, (U, certain, k) in enumerate(R.block_bounds(R.mbuilt(c, level))):
                    if certain:
                        held += 1
                        later += i > 0
                        assert k["type"] == 2 and k["size"] + 3 <= U, (c.family, c.name, level, i, k["type"], k["size"] + 3, U)
                        if U - k["size"] - 3 < smallest[0]:
                            smallest = (U - k["size"] - 3, c.family, c.name, level, i)
    assert later >= 4
    print("blocks with the premises:", held, "smallest margin:", smallest)
    assert held >= 20
    assert any(R.bound_U(R.built(c, 1))[1] for c in R.family("U"))
    for cname in ("all_codes/raw", "all_codes/text"):                 # every code a 128 KiB block can hold, in three described tables: the largest table descriptions
        b = R.built(the("U", cname), 3)
        assert b.shape["blocks"][0]["modes"] == [2, 2, 2], cname
        ll, of, ml = (set(x) for x in R.codes(b.rec))
        assert ll >= set(range(16)) | {16, 18, 20, 22, 24, 25, 26, 27, 28} and ml >= set(range(33)) and of >= set(range(2, 17)), (cname, sorted(ll), sorted(of), sorted(ml))


def test_family_n_takes_the_rare_ways_out(oracle_ref):
    """every frame of family N (level 5, lazy, estimates every table's cost): the reference's model of the normalisation
    (branch_cases.normalise_exit, at the table log FSE_optimalTableLog picks, on the histogram ZSTD_buildCTable would count) takes the way out the case is
    named for — every symbol settled and nothing open, each in the literal-length and the match-length alphabet, at table logs 5 and 6"""
    from branch_cases import normalise_exit
    lib = oracle_ref.lib()
    lib.FSE_optimalTableLog.restype = C.c_uint
    lib.FSE_optimalTableLog.argtypes = [C.c_uint, C.c_size_t, C.c_uint]
    seen = set()
    for c, level, b in blocks_of("N"):
        k = b.shape["blocks"][0]
        assert k["type"] == 2 and len(b.content) < 16384 and set(R.levels_of(c)) == {1, 3, 4, 5}, (c.name, level, k)
        ways = []
        for t, codes in enumerate(R.codes(b.rec)):
            hist = [codes.count(s) for s in range(max(codes) + 1)]
            log = lib.FSE_optimalTableLog((9, 8, 9)[t], len(codes), max(codes))          # LLFSELog, OffFSELog, MLFSELog
            ways.append(normalise_exit(hist, len(codes), log, False)[0])
            seen.add((R.M_NAMES[t], ways[-1], log))
        want = "settled-all" if c.name.endswith("/settled") else "nothing-open"
        assert ways[2] == want and (ways[0] == want or b.nb > 22), (c.name, ways)
    assert {("LL", "settled-all", 5), ("LL", "nothing-open", 5), ("ML", "settled-all", 5), ("ML", "nothing-open", 5), ("ML", "settled-all", 6), ("ML", "nothing-open", 6)} <= seen, seen
