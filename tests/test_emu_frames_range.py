"""CPU (-m "not gpu"): the arithmetic of ranged decompress (zstd-jni_amd/csrc/zj_frames_range.h), built lane-serial from tests/emu_frames_range/emu_frames_range.cpp.

Every buffer of tests/inspect_cases.py plus the crafted ones of tests/test_emu_frames.py, and for each every range whose ends come from {0, every frame boundary
- 1 / + 0 / + 1, T, T + 1, 2^64 - 1}.  PLAN CHECK: status, T, the clamped range, first, last, the edges, every entry array and every copy run against a model
computed here from the reference's ZSTD_findFrameCompressedSize and ZSTD_getFrameContentSize.  PLAN EXECUTION: every planned entry is decoded by the reference
into simulated destination and scratch arrays exactly as planned, the gathers are done in Python, and the result and all bytes of the destination — the 0xCD
fill around and inside the slots included — must be "the reference decodes the buffer, sliced".  The gather's tile and alignment arithmetic runs for every
residue pair.  The -m gpu twin is tests/test_gpu_frames_range.py."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from util import emu_so

import inspect_cases as ic
from test_emu_frames import crafted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU = (1 << 64) - 1
ERROR = MAXU - 1
EDGE_MAX = 128 << 20
FILL = 0xCD
REC_FIELDS = ("total", "lo", "hi", "posF", "endF", "posL", "endL", "preF", "preL", "fcsF", "fcsL")


class Rec(C.Structure):
    """ZRRec (zj_frames_range.h)"""
    _fields_ = [(f, C.c_uint64) for f in REC_FIELDS] + [("status", C.c_uint32), ("frames", C.c_uint32), ("edges", C.c_uint32), ("pad", C.c_uint32)]


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_frames_range", "libzjni_emu_frames_range.so"))
    vp = C.c_void_p
    L.emu_range_count.restype = None
    L.emu_range_count.argtypes = [vp, vp, vp, vp, C.c_uint, vp, vp, vp]
    L.emu_range_emit.restype = None
    L.emu_range_emit.argtypes = [vp, vp, vp, vp, vp, C.c_uint, vp, vp, vp, vp, vp, vp]
    L.emu_range_copy.restype = C.c_uint
    L.emu_range_copy.argtypes = [vp, vp, C.c_ulonglong, vp]
    L.emu_range_gather.restype = C.c_ulonglong
    L.emu_range_gather.argtypes = [vp, C.c_ulonglong, vp, vp, C.c_uint, C.c_ulonglong]
    assert L.emu_range_rec_bytes() == C.sizeof(Rec)
    return L


def arr(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ the model
class Model:
    """what the reference says about a buffer: rule 1's answer, or the frames (position, size, content size) and T"""


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    R = ic.setup_ref(oracle_ref)
    R.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    R.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    cases, _ = ic.build_cases(oracle_ref)
    cases = crafted(oracle_ref) + cases
    dictionary = ic.dictionary(oracle_ref)
    for c in cases:
        c.code, c.frames, pos, total = 0, [], 0, 0
        while pos < len(c.data) and not c.code:
            b = ic.exact(c.data[pos:])
            size = R.ZSTD_findFrameCompressedSize(b, len(c.data) - pos)
            if size > MAXU - 120:
                c.code = MAXU + 1 - size
                break
            fcs = R.ZSTD_getFrameContentSize(b, len(c.data) - pos)
            if fcs == MAXU or total + fcs > MAXU:
                c.code = 14
                break
            assert fcs != ERROR or c.name == "declares_error"
            c.frames.append((pos, size, fcs))
            total += fcs
            pos += size
        c.T = ERROR if c.code else total
        c.decoded = {}

    def frame(c, k):
        """the reference on frame k alone with a capacity of exactly its content size: bytes, or the negative code"""
        if k not in c.decoded:
            pos, size, fcs = c.frames[k]
            z = c.data[pos:pos + size]
            try:
                c.decoded[k] = oracle_ref.decompress_using_dict(z, dictionary, fcs) if c.dict else oracle_ref.decompress(z, fcs)
            except oracle_ref.ZstdRefError as e:
                c.decoded[k] = -e.code
        return c.decoded[k]
    w = Model()
    w.cases, w.frame, w.ref, w.dictionary = cases, frame, oracle_ref, dictionary
    by = {c.name: c for c in cases}
    assert by["forty"].code == 0 and len(by["forty"].frames) == 40 and by["one"].code == 0 and by["skip_alone"].T == 0
    assert by["one_without_size"].code == 14 and by["sum_overflows"].code == 14 and by["truncated_tail"].code == 72 and by["bad_second_magic"].code == 10
    assert by["three_then_stray_byte"].code == 10 and by["declares_2_60"].T == 1 << 60
    assert sum(c.code == 0 and len(c.frames) >= 2 for c in cases) > 10
    return w


def ranges_of(c):
    if c.code:
        return [(0, MAXU), (0, 0), (5, 7), (MAXU, MAXU)]
    ends, run = {0, c.T, c.T + 1, MAXU}, 0
    for _, _, fcs in c.frames:
        run += fcs
        ends |= {max(run - 1, 0), run, run + 1}
    ends = sorted(e for e in ends if e <= MAXU)
    return [(lo, hi - lo) for lo in ends for hi in ends if hi >= lo]


def plan(c, lo, length, slot):
    """rules 1-4 for one buffer: (status, lo', hi', first, last, edges) — edges as the layer counts them: bit 0 first is an entry of set B, bit 1 last is another"""
    if c.code:
        return c.code, 0, 0, 0, 0, 0
    lo2, hi2 = min(lo, c.T), min(lo + length, MAXU, c.T)
    if lo2 == hi2:
        return 1, lo2, hi2, 0, 0, 0
    if slot < hi2 - lo2:
        return 70, lo2, hi2, 0, 0, 0
    run, first, last, pre = 0, None, None, []
    for k, (_, _, fcs) in enumerate(c.frames):
        pre.append(run)
        if fcs and run <= lo2 < run + fcs:
            first = k
        if fcs and run <= hi2 - 1 < run + fcs:
            last = k
        run += fcs
    e_first, e_last = pre[first] < lo2, pre[last] + c.frames[last][2] > hi2
    edges = int(e_first or e_last) if first == last else int(e_first) | int(e_last) << 1
    if (edges & 1 and c.frames[first][2] > EDGE_MAX) or (edges & 2 and c.frames[last][2] > EDGE_MAX):
        return 64, lo2, hi2, 0, 0, 0
    return 0, lo2, hi2, first, last, edges


def expected_arrays(cases, src_off, dst_off, plans):
    """the entry arrays and copy runs of a whole batch from the model: (srcA, dstA, srcB, dstB, in, out, closing entries, first B entry per buffer)"""
    n = len(cases)
    src_a, dst_a, src_b, dst_b, closing, first_b = [], [], [], [], [], []
    in_a, in_b, out = [], [], []
    sel = []
    for i, c in enumerate(cases):
        status, lo2, hi2, first, last, edges = plans[i]
        if status:
            sel.append(None)
            continue
        pre = list(itertools.accumulate([0] + [f[2] for f in c.frames]))
        inter = [k for k in range(first, last + 1) if not (k == first and edges & 1) and not (k == last and edges & 2)]
        sel.append((pre, inter))
    bytes_a = sum(sum(cases[i].frames[k][1] for k in s[1]) for i, s in enumerate(sel) if s)
    at_a, at_b, at_e = 0, bytes_a, 0
    for i, c in enumerate(cases):
        status, lo2, hi2, first, last, edges = plans[i]
        lo, dlo = int(src_off[i]), int(dst_off[i])
        first_b.append(len(src_b))
        if status:
            src_a.append(at_a); dst_a.append(dlo); closing.append(len(src_a) - 1)
            in_a.append((at_a, 0, 0)); in_b += [(at_b, 0, 0)] * 2; out += [(at_e, 0, 0)] * 2
            continue
        pre, inter = sel[i]
        run_bytes = sum(c.frames[k][1] for k in inter)
        run_lo = c.frames[first][0] + (c.frames[first][1] if edges & 1 else 0)
        in_a.append((at_a, lo + run_lo, run_bytes))
        done = 0
        if edges & 1:
            pos, size, fcs = c.frames[first]
            s_lo, s_hi = lo2 - pre[first], min(hi2, pre[first] + fcs) - pre[first]
            src_b.append(at_b); dst_b.append(at_e)
            in_b.append((at_b, lo + pos, size)); out.append((at_e + s_lo, dlo, s_hi - s_lo))
            at_b += size; at_e += fcs
            done = s_hi - s_lo
        else:
            in_b.append((at_b, 0, 0)); out.append((at_e, 0, 0))
        if edges & 2:
            pos, size, fcs = c.frames[last]
            src_b.append(at_b); dst_b.append(at_e)
            in_b.append((at_b, lo + pos, size)); out.append((at_e, dlo + (pre[last] - lo2), hi2 - pre[last]))
            at_b += size; at_e += fcs
        else:
            in_b.append((at_b, 0, 0)); out.append((at_e, 0, 0))
        for k in inter:
            src_a.append(at_a); dst_a.append(dlo + done)
            at_a += c.frames[k][1]; done += c.frames[k][2]
        src_a.append(at_a); dst_a.append(dlo + done); closing.append(len(src_a) - 1)
    src_a.append(at_a); dst_a.append(dst_a[-1]); src_b.append(at_b); dst_b.append(at_e)
    assert at_a == bytes_a
    return src_a, dst_a, src_b, dst_b, in_a + in_b, out, closing, first_b


def run_emu(emu, src, src_off, dst_off, ranges):
    n = len(src_off) - 1
    rec = (Rec * n)()
    scan, total = np.zeros(5 * (n + 1), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    off, doff, rng = arr(src_off), arr(dst_off), arr([v for r in ranges for v in r])
    emu.emu_range_count(ptr(src), ptr(off), ptr(doff), ptr(rng), n, C.byref(rec), ptr(scan), ptr(total))
    tot = [int(scan[k * (n + 1) + n]) for k in range(5)]
    ea, eb = tot[0], tot[1]
    src_a, dst_a = np.full(ea + 1, 0xDEAD, dtype=np.uint64), np.full(ea + 1, 0xDEAD, dtype=np.uint64)
    src_b, dst_b = np.full(eb + 1, 0xDEAD, dtype=np.uint64), np.full(eb + 1, 0xDEAD, dtype=np.uint64)
    cin, cout = np.full(9 * n, 0xDEAD, dtype=np.uint64), np.full(6 * n, 0xDEAD, dtype=np.uint64)
    emu.emu_range_emit(ptr(src), ptr(off), ptr(doff), C.byref(rec), ptr(scan), n, ptr(src_a), ptr(dst_a), ptr(src_b), ptr(dst_b), ptr(cin), ptr(cout))
    triples = lambda a: [tuple(int(x) for x in a[3 * k:3 * k + 3]) for k in range(len(a) // 3)]      # noqa: E731
    lst = lambda a: [int(x) for x in a]      # noqa: E731
    return rec, [int(x) for x in total], tot, lst(src_a), lst(dst_a), lst(src_b), lst(dst_b), triples(cin), triples(cout)


def check_batch(emu, w, cases, ranges, slots, lead=1, execute=True):
    """plan check and plan execution of one batch; returns the results"""
    n = len(cases)
    blob = b"\xAA" * lead + b"".join(c.data for c in cases)
    src = np.frombuffer(blob, dtype=np.uint8)
    src_off = np.cumsum([lead] + [len(c.data) for c in cases]).tolist()
    dst_off = list(itertools.accumulate([7 if sum(slots) < 1 << 62 else 0] + list(slots)))
    rec, total, tot, src_a, dst_a, src_b, dst_b, cin, cout = run_emu(emu, src, src_off, dst_off, ranges)
    plans = [plan(c, ranges[i][0], ranges[i][1], slots[i]) for i, c in enumerate(cases)]
    # ---- plan check
    for i, c in enumerate(cases):
        status, lo2, hi2, first, last, edges = plans[i]
        what = (c.name, ranges[i], slots[i])
        assert rec[i].status == status and total[i] == c.T, what
        if c.code:
            continue
        assert (rec[i].lo, rec[i].hi) == (lo2, hi2), what
        if status == 0:
            pre = [0]
            for f in c.frames:
                pre.append(pre[-1] + f[2])
            assert (rec[i].frames, rec[i].edges) == (last - first + 1, edges), what
            assert (rec[i].posF, rec[i].endF, rec[i].preF, rec[i].fcsF) == (c.frames[first][0], c.frames[first][0] + c.frames[first][1], pre[first], c.frames[first][2]), what
            assert (rec[i].posL, rec[i].endL, rec[i].preL, rec[i].fcsL) == (c.frames[last][0], c.frames[last][0] + c.frames[last][1], pre[last], c.frames[last][2]), what
    want = expected_arrays(cases, src_off, dst_off, plans)
    names = [c.name for c in cases] if n < 4 else n
    assert src_a == want[0] and dst_a == want[1], (names, ranges[:3])
    assert src_b == want[2] and dst_b == want[3], (names, ranges[:3])
    assert cin == want[4] and cout == want[5], (names, ranges[:3])
    closing, first_b = want[6], want[7]
    assert tot == [len(src_a) - 1, len(src_b) - 1, src_a[-1], src_b[-1] - src_a[-1], dst_b[-1]]
    if not execute:
        return None
    # ---- plan execution: source -> compact bytes, the two entry sets by the reference, the finish rule, edge scratch -> the slots
    compact, scratch = bytearray(b"\xEE" * src_b[-1]), bytearray(b"\xEE" * dst_b[-1])
    dst = bytearray(bytes([FILL]) * (dst_off[-1] + 64))
    for key, other, length in cin:
        compact[key:key + length] = blob[other:other + length]
    owner = {}
    for i, c in enumerate(cases):
        if plans[i][0] == 0:
            _, _, _, first, last, edges = plans[i]
            inter = [k for k in range(first, last + 1) if not (k == first and edges & 1) and not (k == last and edges & 2)]
            a0 = (closing[i - 1] + 1) if i else 0
            for j, k in enumerate(inter):
                owner[("A", a0 + j)] = (c, k)
            b = first_b[i]
            if edges & 1:
                owner[("B", b)] = (c, first); b += 1
            if edges & 2:
                owner[("B", b)] = (c, last)
    res = {}
    for tag, s_off, d_off, base in (("A", src_a, dst_a, dst), ("B", src_b, dst_b, scratch)):
        for e in range(len(s_off) - 1):
            z, cap = bytes(compact[s_off[e]:s_off[e + 1]]), max(d_off[e + 1] - d_off[e], 0)
            if (tag, e) not in owner:
                assert tag == "A" and e in closing and z == b""                     # a closing entry: no source byte; it writes nothing
                continue
            c, k = owner[(tag, e)]
            assert z == c.data[c.frames[k][0]:c.frames[k][0] + c.frames[k][1]] and cap == c.frames[k][2], (c.name, k)      # exactly the frame, a slot of exactly its content
            got = w.frame(c, k)
            res[(tag, e)] = got if isinstance(got, int) else len(got)
            if not isinstance(got, int):
                base[d_off[e]:d_off[e] + len(got)] = got
    results = []
    for i, c in enumerate(cases):
        status, lo2, hi2, first, last, edges = plans[i]
        if status:
            results.append(0 if status == 1 else -status)
            continue
        a0, a1, b = (closing[i - 1] + 1) if i else 0, closing[i], first_b[i]
        order = ([("B", b)] if edges & 1 else []) + [("A", e) for e in range(a0, a1)] + ([("B", b + (edges & 1))] if edges & 2 else [])
        assert len(order) == last - first + 1
        bad = [res[o] for o in order if res[o] < 0]
        results.append(bad[0] if bad else hi2 - lo2)
        if bad:
            cout[2 * i], cout[2 * i + 1] = (0, 0, 0), (0, 0, 0)
    for key, other, length in cout:
        dst[other:other + length] = scratch[key:key + length]
    # ---- against the reference's decode of the buffer, sliced
    for i, c in enumerate(cases):
        status, lo2, hi2, first, last, edges = plans[i]
        slot = bytes(dst[dst_off[i]:dst_off[i + 1]])
        if status or results[i] < 0:
            if status:
                assert slot == bytes([FILL]) * len(slot), c.name
            else:
                assert slot[hi2 - lo2:] == bytes([FILL]) * (len(slot) - (hi2 - lo2)), c.name
                codes = [w.frame(c, k) for k in range(first, last + 1)]
                assert results[i] == [x for x in codes if isinstance(x, int)][0], c.name
            continue
        parts = [w.frame(c, k) for k in range(len(c.frames))]
        if all(not isinstance(p, int) for p in parts):
            whole = b"".join(parts)
            if c.name not in c.whole_checked:
                ref_whole = w.ref.decompress_using_dict(c.data, w.dictionary, c.T) if c.dict else w.ref.decompress(c.data, c.T)
                assert ref_whole == whole
                c.whole_checked.add(c.name)
        else:
            pre = 0
            whole = b""
            for k, p in enumerate(parts):
                whole += p if not isinstance(p, int) else b"?" * c.frames[k][2]
        assert results[i] == hi2 - lo2 and slot[:hi2 - lo2] == whole[lo2:hi2], (c.name, ranges[i])
        assert slot[hi2 - lo2:] == bytes([FILL]) * (len(slot) - (hi2 - lo2)), (c.name, ranges[i])
    assert bytes(dst[:dst_off[0]]) == bytes([FILL]) * dst_off[0] and bytes(dst[dst_off[-1]:]) == bytes([FILL]) * 64
    return results


def test_every_buffer_every_range(emu, world):
    w = world
    selected = edges = errors = 0
    for c in w.cases:
        c.whole_checked = set()
        small = c.T != ERROR and c.T <= 1 << 22
        for j, (lo, length) in enumerate(ranges_of(c)):
            want = 0 if c.code else min(lo + length, c.T) - min(lo, c.T)
            execute = small or want == 0
            slot = (want + (j % 3) * 5) if execute else want
            check_batch(emu, w, [c], [(lo, length)], [slot], lead=j % 16, execute=execute)
            p = plan(c, lo, length, slot)
            selected += p[0] == 0
            edges += bin(p[5]).count("1")
            errors += p[0] > 1
            if want and small and j % 4 == 0:
                assert check_batch(emu, w, [c], [(lo, length)], [want - 1]) == [-70]
    assert selected > 5000 and edges > 5000 and errors > 3000


def test_batches_of_every_kind(emu, world):
    """many buffers in one call, a different range each: the scans, the closing entries between the buffers, set B behind set A"""
    w = world
    pool = [c for c in w.cases if c.code == 0 and c.T <= 1 << 22 and not c.name.startswith("random")]
    pool += [c for c in w.cases if c.code and not c.name.startswith(("random", "xmlsmall", "stream^", "dict^"))][:12]
    assert len(pool) > 40
    for c in pool:
        c.whole_checked = set()
    for rnd in range(12):
        ranges, slots = [], []
        for i, c in enumerate(pool):
            rs = ranges_of(c)
            lo, length = rs[(rnd * 131 + i * 17) % len(rs)]
            want = 0 if c.code else min(lo + length, c.T) - min(lo, c.T)
            ranges.append((lo, length))
            slots.append(max(want - 1, 0) if (i + rnd) % 11 == 0 else want + (i % 4) * 3)
        res = check_batch(emu, w, pool, ranges, slots, lead=rnd)
        assert sum(r > 0 for r in res) >= 5                      # (the batch is not all empty ranges and refusals)


def test_oversized_edge_and_beyond_32_bits(emu, world):
    by = {c.name: c for c in world.cases}
    big = by["declares_2_60"]                       # one frame that declares 2^60 bytes
    rec = run_emu(emu, np.frombuffer(big.data, dtype=np.uint8), [0, len(big.data)], [0, 1 << 61], [(0, MAXU)])[0]
    assert (rec[0].status, rec[0].frames, rec[0].edges) == (0, 1, 0)          # whole: an interior frame, straight into the slot
    for rng in ((1, MAXU), (0, (1 << 60) - 1), (5, 10)):
        rec = run_emu(emu, np.frombuffer(big.data, dtype=np.uint8), [0, len(big.data)], [0, 1 << 61], [rng])[0]
        assert rec[0].status == 64, rng
    # an edge of exactly the maximum passes rule 4, one byte more does not
    import struct
    for fcs, status in ((EDGE_MAX, 0), (EDGE_MAX + 1, 64)):
        z = struct.pack("<IBQ", 0xFD2FB528, 0xE0, fcs) + b"\x01\x00\x00"
        rec = run_emu(emu, np.frombuffer(z, dtype=np.uint8), [0, len(z)], [0, 100], [(3, 50)])[0]
        assert rec[0].status == status
    # above 2^32 - 1 source bytes the walk is not started: the source is never read
    n = 1
    recs = (Rec * n)()
    scan, total = np.zeros(10, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    emu.emu_range_count(None, ptr(arr([0, 1 << 32])), ptr(arr([0, 10])), ptr(arr([0, 10])), 1, C.byref(recs), ptr(scan), ptr(total))
    assert recs[0].status == 14 and int(total[0]) == ERROR and [int(scan[2 * k + 1]) for k in range(5)] == [1, 0, 0, 0, 0]


LENGTHS = (0, 1, 15, 16, 17, 4095, 4097)


def test_copy_plan_every_residue_pair(emu):
    """zj_range_copy_plan as a workgroup of the gather uses it: the right bytes arrive, nothing else is written, and 16-byte pieces are used exactly where the
    residues of source and destination agree (the emulation aborts on a misaligned wide piece)"""
    raw_s, raw_d = np.arange(8192, dtype=np.uint32).astype(np.uint8), np.zeros(8192, dtype=np.uint8)
    base_s, base_d = (-raw_s.ctypes.data) % 16, (-raw_d.ctypes.data) % 16
    body = C.c_ulonglong()
    for rs in range(16):
        for rd in range(16):
            for n in LENGTHS:
                raw_d[:] = FILL
                s, d = base_s + 32 + rs, base_d + 48 + rd
                word = emu.emu_range_copy(raw_s.ctypes.data + s, raw_d.ctypes.data + d, n, C.byref(body))
                head, tail, wide = word & 0xFF, (word >> 8) & 0xFF, word >> 16
                assert bytes(raw_d[d:d + n]) == bytes(raw_s[s:s + n]), (rs, rd, n)
                assert (raw_d[:d] == FILL).all() and (raw_d[d + n:] == FILL).all(), (rs, rd, n)
                assert wide == (rs == rd) and head + 16 * body.value + tail == n and tail < 16
                assert head == (min((16 - rd) % 16, n) if wide else 0), (rs, rd, n)


def test_gather_tiles(emu):
    """runs of every length laid end to end in the key space, cut into tiles: both directions, runs of no byte among them, a run that spans several tiles"""
    tile = emu.emu_range_tile()
    rnd = np.random.RandomState(4)
    lengths = list(LENGTHS) * 3 + [tile - 1, tile, tile + 1, 3 * tile + 5, 0, 0, 7]
    rnd.shuffle(lengths)
    far = rnd.randint(0, 256, size=sum(lengths) + 16 * len(lengths) + 64).astype(np.uint8)
    runs, key, other = [], 0, 5
    for k, n in enumerate(lengths):
        runs.append((key, other, n))
        key += n
        other += n + (k % 16)                       # every residue pair between the two sides
    flat = arr([v for r in runs for v in r])
    for key_is_dst in (1, 0):
        near = np.full(key + 32, FILL, dtype=np.uint8)
        if key_is_dst:
            busy = emu.emu_range_gather(ptr(flat), len(runs), ptr(far), ptr(near), 1, key)
            want = bytearray(bytes([FILL]) * len(near))
            for k0, o, n in runs:
                want[k0:k0 + n] = bytes(far[o:o + n])
            assert bytes(near) == bytes(want)
        else:
            near[:key] = rnd.randint(0, 256, size=key).astype(np.uint8)
            out = np.full(len(far), FILL, dtype=np.uint8)
            busy = emu.emu_range_gather(ptr(flat), len(runs), ptr(near), ptr(out), 0, key)
            want = bytearray(bytes([FILL]) * len(out))
            for k0, o, n in runs:
                want[o:o + n] = bytes(near[k0:k0 + n])
            assert bytes(out) == bytes(want)
        assert busy == (key + tile - 1) // tile
    # dead runs (the finish kernel empties them) keep their keys: nothing moves for them
    dead = arr([v for k0, o, n in runs for v in (k0, o, 0)])
    near = np.full(key + 32, FILL, dtype=np.uint8)
    assert emu.emu_range_gather(ptr(dead), len(runs), ptr(far), ptr(near), 1, key) == 0 and (near == FILL).all()


def test_entries_fail_loudly_without_gpu(zj):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = zj.lib()
    out4 = (C.c_uint * 4)()
    buf, dst = C.create_string_buffer(b"x" * 64, 64), C.create_string_buffer(64)
    total = C.c_ulonglong(0)
    r = L.zjni_decompress_frames_range_batch_device(None, None, None, None, None, None, None, 0, None, None)
    assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 200
    r = L.zjni_decompress_frames_range(dst, 64, buf, 64, 0, 10, C.byref(total))
    assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 200
    assert L.zjni_last_frames_range(out4) == -200
