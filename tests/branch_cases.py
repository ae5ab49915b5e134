"""Inputs that exist for ONE line of the device headers each: branches that random text, noise and periodic data never take (tools/emu_coverage.py lists them;
tests/test_emu_reached.py keeps them reached).  Every case names the header and a unique fragment of the line it is for; the CPU tests (lane-serial build)
and the -m gpu tests both run them, and the reference alone decides the expected bytes.  TEST INFRASTRUCTURE."""
import random

# ---- the lines: name -> (header of zstd-jni_amd/csrc/, a fragment of the line's text that no other line of the header holds) ----
LINES = {
    "tans-settled-all": ("zj_encode.h", "share[s] = (short)(share[s] + (i32)cells); }"),
    "tans-nothing-open": ("zj_encode.h", "(rank < cells % holders ? 1 : 0)"),
    "wave-count-back-second-trip": ("zj_match_wavex.h", "if (total + 512u >= limit) return ZJ_UNI(limit);"),
    "lds-wave-count-back-second-trip": ("zj_match_wave.h", "if (total + 512u >= limit) return limit;"),
    "lane-back-goes-on": ("zj_match_lane.h", "vb = true; bp0 = ip - bk; bp1 = mpos - bk;"),
    "gated-lane-back-goes-on": ("zj_match_lane.h", "vb = true; bp0 = ip0 - bk; bp1 = mpos - bk;"),
    "run-back-goes-on": ("zj_match_run.h", "bk += e; more = (e == 8u) && (limit > 8u);"),
    "huffman-window": ("zj_decode.h", "if (o + k < bsize) { if (k < 8u) a |= (u64)bsrc[o + k]"),
    "no-room": ("zj_decode.h", "    GRP_SERIAL(g) { sh.err = ZJ_E_DSTSIZE_TOO_SMALL; } g.sync(); return opos; }"),      # (the blanks: the statement is a line of its own)
    "skippable": ("zj_decode.h", "else { sh.blkType = 1; sh.hdrSize = 8 + ld32(p + 4); }"),
    "pipelined-serial-parse": ("zj_encode.h", "lastLL = ZJ_UNI(sh.tmp[1]); o.n = ZJ_UNI(sh.tmp[2]); o.lit = ZJ_UNI(sh.tmp[3]);"),
    "top64": ("zj_decode_split.h", "return s == 64u ? lo : (lo << (s - 64u));"),
}
# the tests that run the cases (tests/test_emu_reached.py counts the lines over exactly these)
CASE_TESTS = ("tests/test_emu_branches.py", "tests/test_emu_tans.py::test_the_rare_ways_out_equal_the_references", "tests/test_emu_seqrecords.py::test_family_is_the_references_frame[N]",
              "tests/test_emu_wave.py::test_wave_matcher_long_backward_extensions")
# the emulation libraries that hold the lines (tools/emu_coverage.py counts these; the others load from the tree as usual)
CASE_LIBS = ("emu", "emu_wave")

# ---- ze_tans_shares_rare: the ways out of FSE_normalizeCount ----
_RTB = [0, 473195, 504333, 520860, 550000, 700000, 750000, 830000]
EXITS = ("common", "settled-all", "nothing-open", "proportional")


def normalise_exit(count, total, table_log, low):
    """FSE_normalizeCount (N/compress/fse_compress.c:465-523) and its second method FSE_normalizeM2 (:377-462) in python integers: (the way out, whether the bar for
    one cell was raised on the way).  "common": the largest symbol absorbs the rounding surplus and the second method is not entered.  "settled-all": every present
    symbol got the low share or one cell (`distributed == maxSymbolValue + 1`); "nothing-open": the same with an absent symbol in the alphabet (`total == 0`, the
    round robin); "proportional": open symbols share the remaining cells."""
    scale = 62 - table_log; step = (1 << 62) // total; vstep = 1 << (scale - 20)
    still = 1 << table_log; largest = 0; largest_p = 0; norm = [0] * len(count)
    for s, c in enumerate(count):
        if c == 0: continue
        if c <= (total >> table_log): norm[s] = -1 if low else 1; still -= 1
        else:
            p = (c * step) >> scale
            if p < 8 and (c * step) - (p << scale) > vstep * _RTB[p]: p += 1
            if p > largest_p: largest_p = p; largest = s
            norm[s] = p; still -= p
    if not -still >= (norm[largest] >> 1):
        return ("common", False)
    low_threshold = total >> table_log; low_one = (total * 3) >> (table_log + 1)
    distributed = 0; left = total; open_ = []
    for s, c in enumerate(count):
        if c == 0: continue
        if c <= low_threshold or c <= low_one: distributed += 1; left -= c
        else: open_.append(s)
    to_distribute = (1 << table_log) - distributed
    if to_distribute == 0:
        return ("no-cells", False)                              # (returns before either exit: no cell is left to hand out)
    raised = False
    if left // to_distribute > low_one:
        raised = True
        low_one = (left * 3) // (to_distribute * 2)
        for s in list(open_):
            if count[s] <= low_one: open_.remove(s); distributed += 1; left -= count[s]
    if distributed == len(count):
        return ("settled-all", raised)
    if left == 0:
        return ("nothing-open", raised)
    return ("proportional", raised)


def _flat(n, c=1, zeros=(), bumps=()):
    """n slots each counted c, the slots of `zeros` absent, (slot, count) of `bumps` set"""
    h = [c] * n
    for z in zeros: h[z] = 0
    for s, v in bumps: h[s] = v
    return h


def _spread(n, present):
    """n slots, `present` of them counted once: the last slot is present (it is the alphabet's maxSymbolValue), the absent ones lie scattered from slot 0 on"""
    h = [1] * n
    absent, s = n - present, 0
    while absent:
        h[s] = 0; absent -= 1; s = (s + 3) % (n - 1)
        while absent and h[s] == 0: s = (s + 1) % (n - 1)
    assert sum(h) == present and h[-1] == 1
    return h


def tans_histograms():
    """[(name, count[], tableLog)] — the fixed histograms of the two exits of ze_tans_shares_rare that no random family reaches, and their nearest neighbours.
    Why so few: a symbol is settled when count <= 3 * total >> (tableLog + 1), so all of k flat symbols settle only when 3k >= 2^(tableLog + 1); the first method must
    have overdrawn (2^tableLog / k rounds UP past the bar 0.4513 of share 1: k = 22 at log 5, k = 43 or 44 at log 6; log 7 would need 86 symbols, more than any
    alphabet here); and FSE_minTableLog allows log 5 (6) only while total < 32 (64) in alphabets of more than 16 (32) symbols — which a count above 1 among 22 (43)
    present symbols still fits, but 2 <= 3 * total >> (tableLog + 1) then needs total >= 43 (86): so it would stay open in the second method, which then has a symbol to
    give the cells to — and in fact the first method's largest share absorbs the surplus already (the ".../two" neighbours take the common way out).  Every present symbol settled is `settled-all` when the alphabet has no absent symbol, `nothing-open` when it has one — the alphabets of 32, 36 and 53
    slots (offset, literal-length and match-length codes) can therefore only reach the second."""
    out = [("settled-all/22", _flat(22), 5), ("settled-all/43", _flat(43), 6), ("settled-all/44", _flat(44), 6),
           ("nothing-open/22-of-23", _flat(23, zeros=(5,)), 5), ("nothing-open/22-of-23/first-absent", _flat(23, zeros=(0,)), 5),
           ("nothing-open/44-of-45", _flat(45, zeros=(7,)), 6), ("nothing-open/43-of-45", _flat(45, zeros=(0, 30)), 6)]
    for n, present, tl in ((32, 22, 5), (36, 22, 5), (53, 22, 5), (53, 43, 6), (53, 44, 6)):
        out.append((f"nothing-open/{present}-of-{n}", _spread(n, present), tl))
    # neighbours: one symbol more (the first method does not overdraw), and a count of 2 (the largest share absorbs the surplus)
    out += [("neighbour/23", _flat(23), 5), ("neighbour/45", _flat(45), 6), ("neighbour/22/two", _flat(22, bumps=((9, 2),)), 5), ("neighbour/44/two", _flat(44, bumps=((0, 2),)), 6),
            ("neighbour/22-of-23/two", _flat(23, zeros=(5,), bumps=((22, 2),)), 5)]
    return out


# ---- backward extensions: a match found late in a copy of noise ----
def _noise(n, seed):
    return random.Random(seed).randbytes(n)


def late_copy(n, late, seed=1, more=0):
    """n bytes of noise, then the noise from `late` on again (and `more` fresh bytes).  The parse finds nothing in the noise, so its stride has grown to about
    n / 128 when it enters the copy, and of the copy's source only about two positions in (late / 128) was entered into the tables: the copy is found thousands of bytes
    in, and the match is extended backwards over all of them, to the copy's first byte (the byte in front of it differs)."""
    a = _noise(n, seed)
    return a + a[late:] + _noise(more, seed + 1)


def doubled(n, seed=2):
    """the same noise twice: the copy's source begins at the frame's first byte, so the backward extension ends there (a few dozen bytes: the frame's first 256
    positions are all in the tables)"""
    a = _noise(n, seed)
    return a + a


def spliced(n, m, seed=3):
    """noise A, noise B, then A to m followed by B from m on, where A and B share the eight bytes in front of m: the match with A ends at m (the anchor), the match
    with B is found behind it and extended backwards — it would run on over the shared bytes, the anchor stops it"""
    a, b = bytearray(_noise(n, seed)), bytearray(_noise(n, seed + 1))
    b[m - 8:m] = a[m - 8:m]
    return bytes(a + b + a[:m] + b[m:])


def across_blocks(late=70000, seed=4):
    """a frame just over 128 KiB whose copy begins 200 bytes in front of the second block: the first block's parse strides over those 200 bytes, the second block
    finds the copy within its first hundreds of bytes and extends backwards to its own first byte (the anchor) while the source lies deep in the first block"""
    a = _noise(131072 - 200, seed)
    return a + a[late:late + 6000] + _noise(500, seed + 1)


def deep_in_second_block(fresh=30000, late=20000, length=30000, seed=6):
    """a first block of noise, `fresh` bytes of new noise at the head of the second block — the block's parse starts with a stride of 1 and has grown it to about
    fresh / 128 (fresh / 256 at the double-fast levels) when it reaches the copy of the first block's bytes from `late` on, of which only a position or two in
    late / 128 were entered.  The copy is found thousands of bytes in and extended backwards over hundreds of bytes INSIDE the second block: the limit is neither
    the block's first byte (30 000 bytes further down) nor the frame's, the extension ends at the copy's first byte, and the match's source lies in the block before."""
    a = _noise(131072, seed)
    return a + _noise(fresh, seed + 1) + a[late:late + length] + _noise(200, seed + 2)


def backward_inputs():
    """[(name, data)]"""
    return [("late/24000", late_copy(24000, 4000, more=100)), ("late/16000", late_copy(16000, 4000, more=100)), ("doubled/20000", doubled(20000)), ("doubled/3000", doubled(3000)),
            ("spliced/20000", spliced(20000, 15000)), ("across-blocks", across_blocks()), ("second-block/deep", deep_in_second_block())]


# ---- the same for the wave matcher with its tables in LDS (zj_match_wave.h: level 3 with hashLog 14 / chainLog 13, frames to 64 KiB) ----
# Its backward count takes the first 128 bytes in the round that also counts forwards (extend) and the rest in count_back, 512 bytes a trip.  The parse of
# late_copy(24 000, 4 000) finds the copy LDS_WAVE_FOUND bytes into the frame, 1 843 bytes into the copy — measured once on the lane-serial build and asserted since:
# the reference's first sequence of that frame has 24 000 literals (the match begins at the copy's first byte).  One changed byte in the copy, `back` + 1 bytes in
# front of that position, ends the extension there instead: the position where the copy is found does not move (the parse has not found anything yet and strides
# over the changed byte as over the others), so the extension is exactly `back` bytes and the first sequence has LDS_WAVE_FOUND - back literals.
LDS_WAVE_N, LDS_WAVE_LATE, LDS_WAVE_FOUND = 24000, 4000, 25843
# back - 128 is what count_back counts: 384 (a mismatch inside the first trip), 511 / 512 / 513 (the first trip runs through: the line after it asks whether the
# limit is reached, and the second trip ends in its first lane, its first byte or its second), 1 023 / 1 024 / 1 025 (the same around the third trip), 1 715 (the
# copy's first byte, four trips)
LDS_WAVE_BACKS = (512, 639, 640, 641, 1151, 1152, 1153, 1843)


def lds_wave_backward_inputs():
    """[(name, data, back)]: backward extensions of exactly `back` bytes on the LDS wave matcher"""
    base = late_copy(LDS_WAVE_N, LDS_WAVE_LATE, more=100)
    out = []
    for back in LDS_WAVE_BACKS:
        d = bytearray(base)
        if back < LDS_WAVE_FOUND - LDS_WAVE_N:
            d[LDS_WAVE_FOUND - back - 1] ^= 0xFF
        out.append((f"lds-wave/back-{back}", bytes(d), back))
    return out


def lds_wave_first_sequence(data):
    """(offset, litLength, matchLength) of the first sequence of the reference's own parse at level 3 with hashLog 14 / chainLog 13 (ZSTD_generateSequences)"""
    import ctypes as C
    import sequences_cases as SC
    from oracle import ref
    L = SC._lib()
    cctx = L.ZSTD_createCCtx()
    try:
        for p, v in ((100, 3), (102, 14), (103, 13), (1008, 1)):               # ZSTD_c_compressionLevel, ZSTD_c_hashLog, ZSTD_c_chainLog, explicit block delimiters
            ref._check(L.ZSTD_CCtx_setParameter(cctx, p, v))
        cap = L.ZSTD_sequenceBound(len(data))
        arr = (SC._Seq * cap)()
        n = ref._check(L.ZSTD_generateSequences(cctx, arr, cap, bytes(data), len(data)))
        assert n >= 1
        return arr[0].offset, arr[0].litLength, arr[0].matchLength
    finally:
        L.ZSTD_freeCCtx(cctx)


# ---- decoder lines ----
def _skippable(payload, nibble=3):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + payload


def decoder_frames():
    """[(name, line, frame, capacity)] — what a decoder must answer is whatever the reference's portable decoder answers for (frame, capacity): the content or a refusal.
      skippable/*            a skippable frame in front of, between and behind data frames: the fused decoder's own header walk
      no-room-for-sequences  the header's content size is the first block's; the second block brings a sequence when the destination is already full
      short-fourth-stream    2 049 literals in four Huffman streams, no sequence, the jump table changed so that the fourth stream is 20 bytes: its 64-byte decode
                             window reaches past the block's end (a valid stream of 510 literals has 64 bytes, so only a damaged frame gets there)
      wide-codes             literal-length code 34, match-length code 52 and offset code 31 in one sequence: 62 extra bits, so the 64 bits below the bit position begin
                             64 or more bits below the loaded 16 bytes' top; the offset reaches in front of everything, which the decoders find out afterwards"""
    import seqframes as S
    from oracle import ref
    out = []
    text = S._literals(random.Random(7), 3000, "text")
    z = ref.compress(text, 3)
    out.append(("skippable/front", "skippable", _skippable(b"0123456789a") + z, len(text)))
    out.append(("skippable/between", "skippable", z + _skippable(b"", 0) + z + _skippable(b"xyz", 15), 2 * len(text)))
    frame, content, shape = S.build([([], 300), ([(0, 40, 2), (0, 60, 7)], 0)], level=3)          # (no literal in the second block: its literal section needs no room either)
    assert shape["header"] == 7 and len(content) == 400 and [k["type"] for k in shape["blocks"]] == [2, 2]
    out.append(("no-room-for-sequences", "no-room", frame[:5] + (300 - 256).to_bytes(2, "little") + frame[7:], 300))
    rnd = random.Random(8)
    lits = bytes(rnd.choice(b"eeeeeeeeeeeeet") for _ in range(2049))
    frame, content, shape = S.build([([], 2049)], level=3, literals=lits)
    at = shape["header"] + 3
    word = int.from_bytes(frame[at:at + 4], "little")
    assert word & 3 == 2 and (word >> 2) & 3 == 2 and (word >> 4) & 0x3FFF == 2049, "a four-stream Huffman section with a 4-byte header"
    csize = word >> 18
    hb = frame[at + 4]
    jump = at + 5 + (hb if hb < 128 else (hb - 127 + 1) // 2)
    s = [int.from_bytes(frame[jump + 2 * i:jump + 2 * i + 2], "little") for i in range(3)]
    fourth = at + 4 + csize - (jump + 6 + sum(s))
    assert fourth >= 64 and at + 4 + csize + 1 == len(frame), (fourth, "the block ends one byte (no sequences) behind the fourth stream")
    damaged = bytearray(frame)
    damaged[jump + 4:jump + 6] = (s[2] + fourth - 20).to_bytes(2, "little")
    out.append(("short-fourth-stream", "huffman-window", bytes(damaged), 2049))
    frame, content, shape = S.build([([(32768 + 5, 65539 + 100, (1 << 31) - 3 + 77)], 40)], level=3, literals="text", ext_rep=False, decodable=False)
    out.append(("wide-codes", "top64", frame, len(content)))
    return out
