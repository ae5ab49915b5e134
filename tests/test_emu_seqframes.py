"""CPU (-m "not gpu"): frames written from hand-chosen sequences (tests/seqframes.py) through every emulated decode entry — the fused
bodies (emu_decompress, emu_decompress_dict), the three stages (emu_decompress_split, emu_decompress_split_dict) and the block stages
(emu_decompress_mb with and without stage 2b).  The oracle is the content the builder produced in plain Python (confirmed by the
reference before any decoder saw the frame), or the portable reference's answer for a damaged frame.  The lane-serial emulation
compiles the parallel LZ77 executor out, so what these tests pin on the CPU is the three sequence decoders (zd_seq_batch,
ZDSeqLaneT<false>, ZDSeqLaneT<true> with its symbolic repcode history); the same frames meet the executor in
tests/test_gpu_seqframes.py.  The conditions on the inputs — which shapes the families really hold, lane by lane — are asserted here
over the census and the frames' shapes, so that a later edit of the generators cannot hollow a family out."""
import ctypes as C
import os

import pytest

import seqframes as S
from util import emu_lib, emu_decompress, emu_decompress_split, emu_decompress_dict


@pytest.fixture(scope="module")
def emu():
    L = emu_lib()
    L.emu_decompress_mb.restype = C.c_ulonglong
    L.emu_decompress_mb.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_ulonglong, C.POINTER(C.c_int)]
    return L


def mb(L, frame, cap, lit):
    os.environ["EMU_MB_LIT"] = lit
    try:
        dst = C.create_string_buffer(max(cap, 1))
        used = C.c_int(0)
        r = L.emu_decompress_mb(frame, len(frame), dst, cap, C.byref(used))
        return (dst.raw[:r] if r < (1 << 63) else -((1 << 64) - r)), used.value
    finally:
        del os.environ["EMU_MB_LIT"]


def every_entry(L, frame, cap, want, dictionary, shape, who):
    """the frame through each entry that takes it; `shape` (valid frames only) says which pipeline has to serve it"""
    if dictionary is not None:
        assert emu_decompress_dict(L, frame, cap, dictionary.raw) == want, (who, "fused, dictionary")
        assert emu_decompress_dict(L, frame, cap, dictionary.raw, split=True) == want, (who, "three stages, dictionary")
        return
    assert emu_decompress(L, frame, cap) == want, (who, "fused")
    got, used = emu_decompress_split(L, frame, cap)
    assert got == want, (who, "three stages")
    if shape is not None and S.simple(shape):
        assert used in (1, 3), (who, "a simple frame was handed to the fused decoder")
    for lit in ("0", "1"):
        got, used = mb(L, frame, cap, lit)
        assert got == want, (who, "block stages", lit)
        if shape is not None and len(shape["blocks"]) > 1:
            assert used == 1, (who, "a multi-block frame was handed to the fused decoder", lit)


@pytest.mark.parametrize("name", "ABCDEFGH")
def test_family_decodes_to_the_written_content(emu, oracle_ref, name):
    for c in S.family(name):
        frame, content, shape, _ = S.build_case(c)
        every_entry(emu, frame, len(content), content, c.dictionary, shape, (c.family, c.name))


def test_damaged_random_programs_answer_as_the_reference(emu, oracle_ref):
    cases = S.damaged_h(oracle_ref, S.family("H"))
    for c, z, cap, want in cases:
        every_entry(emu, z, cap, want, c.dictionary, None, (c.name, z[:24].hex()))
    refused = sum(isinstance(w, int) for _, _, _, w in cases)
    assert refused >= 30 and len(cases) - refused >= 10, (refused, len(cases))


# ---------------------------------------------------------------------------------------------------------------------------
# conditions on the inputs


def test_family_a_holds_its_chains(oracle_ref):
    A = S.family("A")
    for n in S.CHAIN_N:
        for link in ("next", "next_ll1"):
            S.spread(S.chain_starts(A, n, S.CHAIN_LINKS[link]), (n, link))
    for link in ("range", "skip", "skip_range"):
        S.spread(S.chain_starts(A, 70, S.CHAIN_LINKS[link]), link)
    batches = [bt for c in A for bt in S.build_case(c)[3]]
    assert any(l.depth == 64 for bt in batches for l in bt.lanes)                                  # 64 chained matches inside one batch
    S.spread(S.lanes_where(A, lambda l: len(l.dep) >= 2), "a dependency on a range of lanes", lowest=2)      # (two earlier lanes at the least)
    S.spread(S.lanes_where(A, lambda l: len(l.dep) >= 1 and l.dep[-1] < l.k - 1), "a dependency that skips the lane in front", lowest=2)
    assert any(len(bt.lanes) == 64 and all(l.dep == range(0, 1) for l in bt.lanes[1:]) and len(bt.lanes[0].dep) == 0 for bt in batches)      # every lane on lane 0 only
    assert {max(1, len(S.build_case(c)[2]["blocks"])) > 1 for c in A} == {False, True}


def test_family_b_holds_its_offsets_and_lengths(oracle_ref):
    B = S.family("B")
    for o in S.OFFSETS:
        S.spread(S.lanes_where(B, lambda l: l.off == o), ("offset", o))
    for m in S.MATCHES:
        S.spread(S.lanes_where(B, lambda l: l.ml == m), ("match length", m))
    S.spread(S.lanes_where(B, lambda l: l.ml > 64 and l.off >= l.ml), "wave-wide, off >= ml")
    S.spread(S.lanes_where(B, lambda l: l.ml > 64 and 64 <= l.off < l.ml), "wave-wide, 64 <= off < ml")
    S.spread(S.lanes_where(B, lambda l: l.ml > 64 and l.off < 64), "wave-wide, off < 64")
    S.spread(S.lanes_where(B, lambda l: l.ml <= 64 and l.off < 8 and l.ml > l.off), "byte path, overlapping")
    S.spread(S.lanes_where(B, lambda l: 8 < l.ml <= 64 and 8 <= l.off < l.ml), "8-byte path, overlapping")
    assert all(S.simple(S.build_case(c)[2]) for c in B if len(c.blocks) == 1)


def test_family_c_holds_its_windows(oracle_ref):
    Cc = S.family("C")
    for t in S.TOTALS:
        for later in (False, True):
            S.spread(S.lanes_where(Cc, lambda l: l.ll > 3000, lambda bt: bt.out_total == t and (bt.index > 0) == later and len(bt.lanes) == 64), ("batch total", t, later))
    for a in S.BEFORE:
        if a < 64:                                            # (a match of at most 64 bytes that starts 70 bytes in front ends in front too)
            S.spread(S.lanes_where(Cc, lambda l: l.before == a and l.ml <= 64 and l.ml > a), ("source starts before the window", a, "ml <= 64"))
        S.spread(S.lanes_where(Cc, lambda l: l.before == a and l.ml > 64), ("source starts before the window", a, "ml > 64"))
    S.spread(S.lanes_where(Cc, lambda l: l.at_start and l.ml <= 64), "source ends at the window start, ml <= 64")
    S.spread(S.lanes_where(Cc, lambda l: l.at_start and l.ml > 64), "source ends at the window start, ml > 64")


def test_family_d_holds_its_literal_runs(oracle_ref):
    D = S.family("D")
    for ll in S.LITS:
        S.spread(S.lanes_where(D, lambda l: l.ll == ll), ("literal run", ll))
    for kind in ("text", "raw"):
        assert S.lanes_where([c for c in D if c.literals == kind and len(c.blocks) == 1], lambda l: l.lit_tail), kind
    tails = {tail for c in D for _, tail in c.blocks}
    assert 0 in tails and len(tails) >= 4
    assert {S.build_case(c)[2]["blocks"][0]["lit_type"] for c in D if len(c.blocks) == 1} >= {0, 1, 2}      # raw, RLE and Huffman literals


def test_family_e_holds_its_repcodes(oracle_ref):
    E = S.family("E")
    mid = [c for c in E if c.name.startswith("lane")]
    for f in S.FORMS:
        S.spread(S.lanes_where(mid, lambda l: l.form == f and not l.first_of_block), ("mid-block", f))
    for run in S.RUNS:                                        # the lane at which a run of exactly `run` starts
        found = set()
        for c in mid:
            flat = [r for bt in S.build_case(c)[3] if bt.block == 0 for r in bt.runs_m1]
            found.update((k - run + 1) % S.BATCH for k, r in enumerate(flat) if r == run and (k + 1 == len(flat) or flat[k + 1] == 0))
        S.spread(found, ("run of rep0-1", run))
    behind = {f: set() for f in S.FORMS}
    first_runs = set()
    for c in E:
        if not c.name.startswith("first/"):
            continue
        _, _, shape, cen = S.build_case(c)
        for bt in cen:
            if bt.block == 0 or bt.index != 0:
                continue
            prev = shape["blocks"][bt.block - 1]
            what = {0: "raw", 1: "rle"}.get(prev["type"], "seq" if prev["nbSeq"] else "noseq")
            behind[bt.lanes[0].form].add((what, bt.block >= 2, c.level))
            if bt.lanes[0].form == "rep0m1_ll0":
                first_runs.add(max(r for k, r in enumerate(bt.runs_m1) if all(bt.runs_m1[j] == j + 1 for j in range(k + 1))))
    for f in S.FORMS:                                         # first sequence of a block, behind every kind of block, at both levels
        assert behind[f] >= {(w, True, lv) for w in ("raw", "rle", "noseq", "seq") for lv in (3, 7)} | {("seq", False, 3)}, (f, behind[f])
    assert first_runs >= {1, 2, 3, 10}
    for f in S.FORMS:                                         # the dictionary's own repcodes, taken by the frame's first sequence
        cen = [S.build_case(c)[3] for c in E if c.name == f"dictrep/{f}"]
        assert len(cen) == 1 and cen[0][0].lanes[0].form == f and cen[0][0].lanes[0].first_of_block


def test_family_f_holds_its_codes_and_counts(oracle_ref):
    F = S.family("F")
    vals = S.code_values()
    assert {(k, c) for k, c, _ in vals} == {("ll", c) for c in range(16, 36)} | {("ml", c) for c in range(32, 53)}
    assert len(vals) == 2 * (20 + 21) - 2                     # only the last values of LL code 35 and ML code 52 do not fit a 128 KiB block
    for kind, code, v in vals:
        S.spread(S.lanes_where(F, (lambda l: l.ll == v) if kind == "ll" else (lambda l: l.ml == v)), (kind, code, v))
    shapes = {c.name: S.build_case(c)[2] for c in F}
    for n in S.COUNTS:
        assert shapes[f"count/{n}"]["blocks"][0]["nbSeq"] == n and S.simple(shapes[f"count/{n}"])
        assert [b["nbSeq"] for b in shapes[f"count/{n}/twice"]["blocks"]] == [n, n]
    modes = {(c.level, t, b["modes"][t]) for c in F for b in S.build_case(c)[2]["blocks"] if b["modes"] for t in range(3)}
    for t in range(3):                                        # LL, OF, ML: predefined, RLE and compressed at level 3, repeat at level 7
        assert {(3, t, 0), (3, t, 1), (3, t, 2), (7, t, 3)} <= modes, (t, sorted(modes))
    frame, content, shape, cen = S.build_case([c for c in F if c.name == "wide"][0])
    assert 1_200_000 < len(content) < 1_500_000 and len(shape["blocks"]) == 11 and all(b["type"] == 2 for b in shape["blocks"])
    wide = [(bt.block, bt.index, l.k) for bt in cen for l in bt.lanes if (l.ll, l.ml, l.off) == S.WIDE_SEQ]
    frame, content, shape, cen = S.build_case([c for c in F if c.name == "widths"][0])
    bits = [tw for rec in S.seq_bits(shape, cen).values() for tw in rec[:-1]]              # (not the blocks' last sequences)
    assert {(t, True) for t in range(57, 67)} <= set(bits), sorted(set(bits), key=str)     # both sides of 64 bits, with 16 bytes of bitstream below
    assert (57, False) in bits                                                             # ... and a long one within 16 bytes of the stream's start
    assert wide == [(9, 0, 0), (10, 0, 40)]                   # a block's first sequence (bits at the stream's end) and a block's last (within 16 bytes of its start)


def test_family_g_holds_its_dictionary_matches(oracle_ref):
    G = S.family("G")
    for dname in ("raw", "full"):
        for big in (False, True):
            sub = [c for c in G if c.name.startswith(f"{dname}/") and ("/big/" in c.name) == big]
            size = (lambda bt: bt.out_total > S.STAGE) if big else (lambda bt: bt.out_total <= S.STAGE)
            for long in (False, True):
                ml = (lambda l: l.ml > 64) if long else (lambda l: l.ml <= 64)
                who = (dname, "big" if big else "small", "ml > 64" if long else "ml <= 64")
                S.spread(S.lanes_where(sub, lambda l: ml(l) and l.dict_n == l.ml and not l.dict_end, size), who + ("inside",))
                S.spread(S.lanes_where(sub, lambda l: ml(l) and l.dict_end, size), who + ("ends on the last byte",))
                S.spread(S.lanes_where(sub, lambda l: ml(l) and l.dict_first, size), who + ("offset = position + dictionary size",))
                for s in S.STRADDLE:
                    if s < 64 or long:                        # (70 bytes into the output takes a match of more than 64)
                        S.spread(S.lanes_where(sub, lambda l: ml(l) and l.dict_n > 0 and l.ml - l.dict_n == s, size), who + ("straddles by", s))
    assert all(S.build_case(c)[2]["dict_id"] == c.name.startswith("full/") for c in G)


def test_family_h_holds_both_kinds_of_batches(oracle_ref):
    H = S.family("H")
    assert sum(c.name.startswith("single/") for c in H) == 400 and sum(c.name.startswith("multi/") for c in H) == 60 and sum(c.name.startswith("dict/") for c in H) == 60
    assert all(len(S.build_case(c)[1]) <= 16384 for c in H if not c.name.startswith("multi/"))
    assert all(2 <= len(c.blocks) <= 6 for c in H if c.name.startswith("multi/"))
    totals = [bt.out_total for c in H for bt in S.build_case(c)[3]]
    assert sum(t <= S.STAGE for t in totals) >= 20 and sum(t > S.STAGE for t in totals) >= 20
