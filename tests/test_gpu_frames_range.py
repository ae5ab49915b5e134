"""GPU (-m gpu): ranged decompress.  zjni_decompress_frames_range_batch_device against "the reference decodes the whole buffer, sliced" — exact results and exact
bytes, the destination filled with 0xCD and checked everywhere — or, where a selected frame is damaged, against the reference on that frame alone.
zjni_last_frames_range is pinned in every valid case: frames handed to the decoder = the frames the range touches, so no other frame was decoded.  The CPU
twin of the arithmetic is tests/test_emu_frames_range.py."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import inspect_cases as ic
from util import json_records

pytestmark = pytest.mark.gpu

FILL = 0xCD
MAXU = (1 << 64) - 1
EDGE_MAX = 128 << 20


class World:
    pass


class Buf:
    """a buffer of frames: pieces = [(decoded bytes, frame bytes)], a skippable frame decodes to nothing; tail: bytes behind them that end the walk with `code`"""

    def __init__(self, pieces, tail=b"", code=0, dict=False):
        self.pieces, self.tail, self.code, self.dict = list(pieces), tail, code, dict
        self.data = b"".join(p[1] for p in pieces) + tail
        self.whole = b"".join(p[0] for p in pieces)
        self.T = len(self.whole)


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    import torch
    zj.batch.init(0)
    w = World()
    w.torch, w.zj, w.ref = torch, zj, oracle_ref
    w.R = ic.setup_ref(oracle_ref)
    rnd = random.Random(12)
    text = b",".join(json_records(3000, seed=9))
    noise = zj.synth_host(65536, 5, 1)
    w.pool = []                                          # (original, frame, checksum): 256 B - 4 KiB payloads, levels 1 and 3, every third with a checksum
    for k in range(97):
        size = rnd.choice((256, 300, 511, 700, 1024, 1500, 4096)) if k % 5 else rnd.randrange(256, 4097)
        at = rnd.randrange(0, len(text) - size)
        orig = text[at:at + size] if k % 4 else noise[at % 60000:at % 60000 + size]
        w.pool.append((orig, oracle_ref.compress(orig, 1 if k & 1 else 3, checksum=(k % 3 == 0)), k % 3 == 0))
    w.dict_bytes = ic.dictionary(oracle_ref)
    w.ddict = zj.ZstdDictDecompress(w.dict_bytes)
    w.other_dict = oracle_ref.train_dict(json_records(1500, seed=77), 4096)
    w.other_ddict = zj.ZstdDictDecompress(w.other_dict)
    w.checked = set()
    yield w
    w.ddict.close()
    w.other_ddict.close()


def many(w, count, start):
    return Buf([w.pool[(start + j) % len(w.pool)][:2] for j in range(count)])


def skip(payload, variant=3):
    return (b"", ic.skippable(payload, variant))


def expect(w, b, lo, length, slot):
    """(result, bytes at the slot's start, frames decoded, edge frames) by rules 1-5 from what the reference says about the buffer"""
    if b.code:
        return -b.code, b"", 0, 0
    if b.data not in w.checked:                          # the oracle: the reference decodes the whole buffer
        got = w.ref.decompress_using_dict(b.data, w.dict_bytes, b.T) if b.dict else w.ref.decompress(b.data, b.T)
        assert got == b.whole
        w.checked.add(b.data)
    lo2, hi2 = min(lo, b.T), min(lo + length, b.T)
    if lo2 == hi2:
        return 0, b"", 0, 0
    if slot < hi2 - lo2:
        return -70, b"", 0, 0
    run, first, last, pre = 0, None, None, []
    for k, (orig, _) in enumerate(b.pieces):
        pre.append(run)
        if orig and run <= lo2 < run + len(orig):
            first = k
        if orig and run <= hi2 - 1 < run + len(orig):
            last = k
        run += len(orig)
    e_first, e_last = pre[first] < lo2, pre[last] + len(b.pieces[last][0]) > hi2
    edges = int(e_first or e_last) if first == last else int(e_first) + int(e_last)
    return hi2 - lo2, b.whole[lo2:hi2], last - first + 1, edges


def call(w, bufs, ranges, slots, dictionary=None, lead=1, totals=True):
    """one call -> (results, destination bytes, totals, last_frames_range, slot offsets)"""
    t, zj = w.torch, w.zj
    blob = b"\xAA" * lead + b"".join(b.data for b in bufs)
    src = t.frombuffer(bytearray(blob), dtype=t.uint8).cuda()
    off = t.from_numpy(np.cumsum([lead] + [len(b.data) for b in bufs]).astype(np.int64)).cuda()
    at = np.cumsum([3] + list(slots)).tolist()
    dst_off = t.tensor(at, dtype=t.int64, device="cuda")
    dst = t.full((at[-1] + 64,), FILL, dtype=t.uint8, device="cuda")
    rng = t.from_numpy(np.array([int(v) for r in ranges for v in r], dtype=np.uint64).view(np.int64)).cuda()
    if totals:
        res, tot = zj.batch.decompress_frames_range(src, off, dst, dst_off, rng, dictionary=dictionary)
    else:
        res, tot = t.empty(len(bufs), dtype=t.int64, device="cuda"), None
        dd = dictionary._ptr if dictionary is not None else None
        r = zj.lib().zjni_decompress_frames_range_batch_device(src.data_ptr(), off.data_ptr(), dst.data_ptr(), dst_off.data_ptr(), rng.data_ptr(), res.data_ptr(), None,
                                                               len(bufs), dd, t.cuda.current_stream().cuda_stream)
        assert r == 0
    stats = zj.batch.last_frames_range()
    return res.cpu().tolist(), dst.cpu().numpy().tobytes(), None if tot is None else tot.cpu().tolist(), stats, at


def check(w, bufs, ranges, slack=0, dictionary=None, lead=1, totals=True, slots=None):
    """the call against the model, every byte of the destination included"""
    wants = [min(lo + ln, b.T) - min(lo, b.T) if not b.code else 0 for b, (lo, ln) in zip(bufs, ranges)]
    if slots is None:
        slots = [x + (slack if i & 1 else 0) for i, x in enumerate(wants)]
    exp = [expect(w, b, lo, ln, slots[i]) for i, (b, (lo, ln)) in enumerate(zip(bufs, ranges))]
    r, out, tot, stats, at = call(w, bufs, ranges, slots, dictionary=dictionary, lead=lead, totals=totals)
    assert r == [e[0] for e in exp], (r, [e[0] for e in exp])
    if totals:
        assert tot == [b.T if not b.code else -2 for b in bufs]
    image = bytearray(bytes([FILL]) * len(out))
    for i, e in enumerate(exp):
        image[at[i]:at[i] + len(e[1])] = e[1]
    assert out == bytes(image)
    assert stats == {"served": sum(e[0] >= 0 for e in exp), "frames": sum(e[2] for e in exp), "edges": sum(e[3] for e in exp), "errors": sum(e[0] < 0 for e in exp)}
    return r, out, at


def shapes(b):
    """the range shapes of one buffer: whole, empty, lo == T, lo > T, an endless length, ends on frame boundaries, inside one frame, two edges"""
    sizes = [len(p[0]) for p in b.pieces]
    cuts = np.cumsum([0] + sizes).tolist()
    T = b.T
    out = [(0, T), (0, MAXU), (5, 0), (T, 10), (T + 7, 10), (MAXU, MAXU), (1, MAXU), (0, T - 1), (1, T - 2)]
    big = max(range(len(sizes)), key=lambda k: sizes[k])
    out += [(cuts[big] + 3, 40), (cuts[big], sizes[big]), (cuts[big] + 1, sizes[big] - 1), (cuts[big], sizes[big] - 1)]
    if len(sizes) >= 2:
        out += [(cuts[1], T - cuts[1]), (cuts[1] - 1, 2), (0, cuts[1])]
    if len(sizes) >= 3:
        out += [(cuts[1], cuts[2] - cuts[1]), (cuts[1] - 1, cuts[2] - cuts[1] + 2), (cuts[1], cuts[-2] - cuts[1])]
    if len(sizes) >= 40:
        out += [(cuts[3] + 5, cuts[30] - cuts[3]), (cuts[7], cuts[19] - cuts[7]), (cuts[7], cuts[19] - cuts[7] + 1), (cuts[20] - 1, 1)]
    return out


@pytest.mark.parametrize("count", (1, 2, 3, 40))
def test_range_shapes(world, count):
    w = world
    b = many(w, count, 3 * count)
    rs = shapes(b)
    check(w, [b] * len(rs), rs, slack=9)
    check(w, [b] * len(rs), rs, slack=0, totals=False, lead=6)


def test_skippable_and_empty_frames(world):
    w, ref = world, world.ref
    empty, empty_ck = (b"", ref.compress(b"", 3)), (b"", ref.compress(b"", 1, checksum=True))
    f = [w.pool[k][:2] for k in range(8)]
    n = [len(x[0]) for x in f]
    bufs = [Buf([skip(b"index"), f[0], f[1]]), Buf([f[0], skip(b""), f[1], skip(b"xy", 7), f[2]]), Buf([f[3], f[4], skip(b"trailer", 15)]),
            Buf([empty, f[5], empty_ck, empty, f[6], empty]), Buf([empty, empty]), Buf([skip(b"alone")])]
    for rs in ([(0, MAXU)] * 6,
               [(1, MAXU), (n[0] - 1, n[1] + 2), (n[3], MAXU), (n[5] - 1, 2), (0, 5), (0, 5)],           # skippable and empty frames between the selected ones
               [(0, n[0]), (0, n[0]), (0, n[3] + n[4]), (0, n[5]), (1, 1), (3, 0)],                       # ... and left out at either end
               [(n[0], n[1]), (n[0], n[1]), (n[3] + 1, n[4] - 1), (n[5], n[6]), (0, 0), (0, 1)]):
        check(w, bufs, rs, slack=5)
    # a range that touches frames of no content only: nothing to decode
    r, _, _, stats, _ = call(w, [bufs[4], bufs[5]], [(0, MAXU), (0, 1)], [16, 16])
    assert r == [0, 0] and stats == {"served": 2, "frames": 0, "edges": 0, "errors": 0}


def test_checksum_frames(world):
    w = world
    ck = [p[:2] for p in w.pool if p[2]][:9]
    b = Buf(ck)
    n0 = len(ck[0][0])
    check(w, [b, b, b, b], [(0, MAXU), (n0 - 1, 2), (n0, b.T - n0), (5, b.T - 10)], slack=3)


def test_dictionary_frames(world):
    w, ref = world, world.ref
    recs = json_records(60, seed=21)
    origs = [b",".join(recs[k:k + 3]) for k in range(0, 60, 3)]
    pieces = [(o, ref.compress_using_dict(o, w.dict_bytes, 3)) for o in origs]
    b = Buf(pieces, dict=True)
    mixed = Buf(pieces[:2] + [w.pool[0][:2]], dict=True)
    n0, n1 = len(origs[0]), len(origs[1])
    rs = [(0, MAXU), (n0 + 4, n1 + 50), (n0, n1), (n0 + n1, MAXU)]
    check(w, [b, b, b, mixed], rs, slack=4, dictionary=w.ddict)
    # the other dictionary, and none: dictionary_wrong (32) from the first selected frame; a range of plain frames only does not notice
    for dd in (w.other_ddict, None):
        slots = [b.T, n1 + 50, n1, len(w.pool[0][0])]
        r, out, _, stats, at = call(w, [b, b, b, mixed], rs, slots, dictionary=dd)
        assert r == [-32, -32, -32, len(w.pool[0][0])]
        assert out[at[3]:at[4]] == w.pool[0][0] and out[at[4]:] == bytes([FILL]) * 64 and out[:3] == bytes([FILL]) * 3
        assert stats == {"served": 1, "frames": 20 + 2 + 1 + 1, "edges": 2, "errors": 3}


def flipped(frame):
    z = bytearray(frame)
    z[len(z) // 2] ^= 0x10                                   # inside the block content
    return bytes(z)


def test_damage(world):
    w, ref = world, world.ref
    ck = [p[:2] for p in w.pool if p[2]]
    pieces = ck[:7]
    good = Buf(pieces)
    cuts = np.cumsum([0] + [len(p[0]) for p in pieces]).tolist()
    bad3 = Buf(pieces[:3] + [(pieces[3][0], flipped(pieces[3][1]))] + pieces[4:])
    try:
        ref.decompress(bad3.pieces[3][1], len(pieces[3][0]))
        code = 0
    except ref.ZstdRefError as e:
        code = e.code                                        # the reference on the damaged frame alone
    assert code in (20, 22)
    # outside the selection: not seen.  (the model's whole-buffer oracle does not apply to a damaged buffer: the undamaged twin is the oracle)
    w.checked.add(bad3.data)
    check(w, [good, bad3, bad3, bad3, good], [(0, MAXU), (0, cuts[3]), (cuts[4], MAXU), (cuts[1] + 1, cuts[3] - cuts[1] - 1), (3, 50)], slack=6)
    # inside: as an interior frame, as the first edge, as the last edge, as the one frame of the range — the neighbours' slots stay whole
    rs = [(0, MAXU), (cuts[1] + 1, cuts[5] - cuts[1] - 2), (cuts[3] + 5, MAXU), (0, cuts[4] - 5), (cuts[3] + 1, 9), (cuts[3], cuts[4] - cuts[3]), (2, 70)]
    bufs = [good, bad3, bad3, bad3, bad3, bad3, good]
    slots = [min(lo + ln, good.T) - lo + 8 for lo, ln in rs]
    r, out, _, stats, at = call(w, bufs, rs, slots)
    assert r == [good.T, -code, -code, -code, -code, -code, 70]
    assert out[at[0]:at[0] + good.T] == good.whole and out[at[6]:at[6] + 70] == good.whole[2:72]
    for i in range(7):
        assert out[at[i + 1] - 8:at[i + 1]] == bytes([FILL]) * 8, i           # nothing behind the first hi' - lo' bytes of any slot
    assert out[:3] == bytes([FILL]) * 3 and out[at[7]:] == bytes([FILL]) * 64
    assert stats == {"served": 2, "frames": 7 + 4 + 4 + 4 + 1 + 1 + 1, "edges": 0 + 2 + 1 + 1 + 1 + 0 + 1, "errors": 5}


def test_short_slot(world):
    w = world
    a, b = many(w, 5, 2), many(w, 3, 40)
    rs = [(3, a.T - 5), (0, MAXU), (1, 600)]
    slots = [a.T - 5, b.T - 1, 599]
    r, out, _, stats, at = call(w, [a, b, a], rs, slots)
    assert r == [a.T - 5, -70, -70]
    assert out[at[0]:at[1]] == a.whole[3:a.T - 2] and out[at[1]:] == bytes([FILL]) * (len(out) - at[1])
    assert stats == {"served": 1, "frames": 5, "edges": 2, "errors": 2}


def test_not_indexable(world):
    w, ref, R = world, world.ref, world.R
    f = [w.pool[k][:2] for k in range(6)]
    text = w.pool[1][0]
    nosize = ref.compress(text, 3, content_size=False)

    def code_at(tail):
        size = R.ZSTD_findFrameCompressedSize(ic.exact(tail), len(tail))
        assert size > MAXU - 120
        return MAXU + 1 - size
    tails = [f[2][1][:-5], b"\x29\xB5\x2F\xFD" + f[3][1][4:], b"\x00"]
    bufs = [Buf(f[:2], tail=t, code=code_at(t)) for t in tails]
    bufs.append(Buf([f[0]], tail=nosize + f[1][1], code=14))
    bufs.append(Buf([], tail=nosize, code=14))
    assert [b.code for b in bufs] == [72, 10, 10, 14, 14]
    good = many(w, 2, 0)
    check(w, bufs + [good], [(0, 10)] * 5 + [(1, 10)], slots=[32] * 6)
    check(w, bufs + [good], [(0, MAXU), (5, 0), (MAXU, 1), (0, 1), (7, 7), (0, MAXU)], slots=[0, 0, 8, 8, 8, good.T])


def test_oversized_edge(world):
    w = world
    for fcs, want in ((EDGE_MAX + 1, -64), (1 << 60, -64)):
        z = struct.pack("<IBQ", 0xFD2FB528, 0xE0, fcs) + b"\x01\x00\x00"            # a hand-written header: one frame that declares fcs bytes, one empty raw block
        b = Buf([], tail=z)
        r, out, tot, stats, at = call(w, [b, many(w, 2, 5)], [(3, 50), (3, 50)], [100, 50])
        assert r == [want, 50] and tot[0] == fcs and out[at[0]:at[1]] == bytes([FILL]) * 100
        assert stats == {"served": 1, "frames": 1, "edges": 1, "errors": 1}


@pytest.mark.parametrize("lead", range(16))
def test_seventy_buffers(world, lead):
    """two waves of lanes, a different range each; with the leads every residue between the source and the compact bytes occurs"""
    w = world
    rnd = random.Random(lead)
    bufs, rs = [], []
    for i in range(70):
        b = many(w, (1, 2, 3, 5, 9, 17)[i % 6], 7 * i + lead)
        lo = rnd.randrange(0, b.T)
        bufs.append(b)
        rs.append((lo, rnd.randrange(1, b.T - lo + 40)) if i % 7 else (0, MAXU))
    check(w, bufs, rs, slack=lead)


def test_pipeline_route(world):
    """4 buffers x 1 100 frames, the whole range minus a byte at each end: 4 392 interior entries (at or above ZJNI_DSPLIT_MIN: the three-stage pipeline) and 8 edges"""
    w = world
    bufs = [many(w, 1100, 11 * i) for i in range(4)]
    check(w, bufs, [(1, b.T - 2) for b in bufs])
    stats = w.zj.batch.last_frames_range()
    assert stats["frames"] == 4400 and stats["edges"] == 8


def test_no_buffers(world):
    t, zj = world.torch, world.zj
    z = t.zeros(1, dtype=t.int64, device="cuda")
    e = t.empty(8, dtype=t.uint8, device="cuda")
    res, tot = zj.batch.decompress_frames_range(e, z, e, z, t.empty(0, dtype=t.int64, device="cuda"))
    assert res.numel() == 0 and tot.numel() == 0
    assert zj.batch.last_frames_range() == {"served": 0, "frames": 0, "edges": 0, "errors": 0}


def test_host_form(world):
    w, L = world, world.zj.lib()
    b = many(w, 12, 4)
    assert b.T > 3700
    dst = C.create_string_buffer(b.T + 16)
    total = C.c_ulonglong(0)
    for lo, ln in ((0, MAXU), (700, 3000), (b.T - 5, 100), (b.T, 5), (0, 0)):
        C.memset(dst, FILL, b.T + 16)
        r = L.zjni_decompress_frames_range(dst, b.T, b.data, len(b.data), lo, ln, C.byref(total))
        want = b.whole[lo:lo + ln]
        assert r == len(want) and total.value == b.T
        assert dst.raw[:r] == want and dst.raw[r:] == bytes([FILL]) * (b.T + 16 - r)
    assert L.zjni_getErrorCode(L.zjni_decompress_frames_range(dst, 2999, b.data, len(b.data), 700, 3000, None)) == 70
    assert L.zjni_decompress_frames_range(dst, 10, b.data, len(b.data), 700, 10, None) == 10 and dst.raw[:10] == b.whole[700:710]
    cut = b.data[:-3]
    assert L.zjni_getErrorCode(L.zjni_decompress_frames_range(dst, b.T, cut, len(cut), 0, 10, C.byref(total))) == 72 and total.value == MAXU - 1


def test_interplay_on_one_stream(world):
    """two ranged calls back to back on one stream (the second needs more scratch than the first), and one behind zjni_decompress_frames_batch_device"""
    w, t, zj = world, world.torch, world.zj
    small, large = many(w, 3, 1), many(w, 300, 2)

    def enqueue(b, lo, ln):
        src = t.frombuffer(bytearray(b.data), dtype=t.uint8).cuda()
        off = t.tensor([0, len(b.data)], dtype=t.int64, device="cuda")
        dst_off = t.tensor([0, ln], dtype=t.int64, device="cuda")
        dst = t.full((ln + 32,), FILL, dtype=t.uint8, device="cuda")
        rng = t.tensor([lo, ln], dtype=t.int64, device="cuda")
        return zj.batch.decompress_frames_range(src, off, dst, dst_off, rng)[0], dst, src, off, dst_off, rng
    a = enqueue(small, 5, small.T - 9)
    b = enqueue(large, 7, large.T - 20)
    c = enqueue(small, 300, 100)
    t.cuda.synchronize()
    for (res, dst, *_), buf, lo, ln in ((a, small, 5, small.T - 9), (b, large, 7, large.T - 20), (c, small, 300, 100)):
        assert res.cpu().tolist() == [ln]
        assert dst.cpu().numpy().tobytes() == buf.whole[lo:lo + ln] + bytes([FILL]) * 32
    # behind the whole-buffer entry, which keeps its own arrays in the same scratch
    src = t.frombuffer(bytearray(large.data), dtype=t.uint8).cuda()
    off = t.tensor([0, len(large.data)], dtype=t.int64, device="cuda")
    full_off = t.tensor([0, large.T], dtype=t.int64, device="cuda")
    full = t.full((large.T,), FILL, dtype=t.uint8, device="cuda")
    r1 = zj.batch.decompress_frames(src, off, full, full_off)
    d = enqueue(large, 1000, 5000)
    r2 = zj.batch.decompress_frames(src, off, full, full_off)
    t.cuda.synchronize()
    assert r1.cpu().tolist() == r2.cpu().tolist() == [large.T] and full.cpu().numpy().tobytes() == large.whole
    assert d[0].cpu().tolist() == [5000] and d[1].cpu().numpy().tobytes() == large.whole[1000:6000] + bytes([FILL]) * 32
