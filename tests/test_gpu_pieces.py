"""GPU (-m gpu): zjni_compress_pieces_batch_device — chunked compress with a dictionary, the caller's cuts and the frame sizes out.  Without any of the three it is
held against zjni_compress_chunked_batch_device on the same tensors (results and every destination byte); with them every frame is held against the reference's
frame for its piece (ZSTD_compress2 with or without ZSTD_CCtx_refCDict, same checksum and dictID flags), the index against the frames' sizes, and the output is read
back through decompress_frames, decompress_frames_range and, frame by frame from the index alone, the plain decompress.  The CPU twin of the arithmetic is
tests/test_emu_pieces.py."""
import ctypes as C
import random

import numpy as np
import pytest

import dictutil as du
from pieces_cases import illegal, lay_out
from util import json_records

pytestmark = pytest.mark.gpu

FILL = 0xCD
RES_FILL = -777
CD_LEVELS = (1, 3, -3)


class World:
    pass


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    import torch
    zj.batch.init(0)
    w = World()
    w.torch, w.zj, w.ref = torch, zj, oracle_ref
    recs = json_records(9000, seed=31)
    content = b",".join(recs[:150])
    hist = [0] * 256
    for b in content:
        hist[b] += 1
    w.dict_bytes = du.build(content, 4242, hist, du.normalise([1, 0, 1, 1, 0] + [2] * 12, 7), 7, du.normalise([3 if i < 20 else 1 for i in range(40)], 8), 8,
                            du.normalise([4 if i < 10 else 1 for i in range(36)], 8), 8)
    w.cd = {lv: zj.ZstdDictCompress(w.dict_bytes, lv) for lv in CD_LEVELS}
    w.ref_cd = {lv: oracle_ref.CDict(w.dict_bytes, lv) for lv in CD_LEVELS}
    w.dd = zj.ZstdDictDecompress(w.dict_bytes)
    text = b",".join(recs[200:])
    w.body = (text[:300000] + zj.synth_host(65536, 3, 1) + text[300000:])            # compressible bytes with an incompressible stretch
    assert len(w.body) > 700000
    w.frames = {}
    yield w
    for cd in w.cd.values():
        cd.close()
    w.dd.close()


def payload(w, size, at=0):
    """`size` bytes of the body from `at` on, going round"""
    return (w.body[at:] + w.body * (size // len(w.body) + 1))[:size]


def ref_frame(w, piece, level, ck, cd_level=None, dict_id=True):
    """the reference's frame for one piece, computed once"""
    key = (piece, level, ck, cd_level, dict_id)
    if key not in w.frames:
        w.frames[key] = (w.ref.compress(piece, level, checksum=ck) if cd_level is None else w.ref_cd[cd_level].compress(piece, checksum=ck, dict_id=dict_id))
    return w.frames[key]


def pieces_of(data, cuts, chunk):
    if cuts is None:
        return [data[k:k + chunk] for k in range(0, len(data), chunk)] or [b""]
    edges = [0] + [int(c) for c in cuts] + [len(data)]
    return [data[a:b] for a, b in zip(edges[:-1], edges[1:])]


def tensors(w, bufs, caps, lead=5):
    t = w.torch
    blob = b"\xAA" * lead + b"".join(bufs)
    assert len(blob) < 16 << 20 and sum(caps) < 48 << 20
    src = t.frombuffer(bytearray(blob), dtype=t.uint8).cuda()
    off = t.from_numpy(np.cumsum([lead] + [len(b) for b in bufs]).astype(np.int64)).cuda()
    dst_off = t.from_numpy(np.cumsum([3] + list(caps)).astype(np.int64)).cuda()
    return src, off, dst_off, 3 + sum(caps) + 64


class Out:
    pass


def run(w, datas, chunk, level=3, ck=False, cuts=None, cd=None, dict_id=True, sizes=False, caps=None, raw=None, piece_cap=None, chunked=False):
    """one call on FILLed tensors.  cuts: a list of cut lists (one per buffer), or None for the fixed grid; raw: (d_cut, d_cut_off) as they are;
    chunked: the existing zjni_compress_chunked_batch_device instead"""
    t, zj = w.torch, w.zj
    if caps is None:
        counts = [len(c) + 1 for c in cuts] if cuts is not None else [max(1, -(-len(d) // chunk)) for d in datas]
        caps = [zj.batch.compress_bound_pieces(len(d), k) for d, k in zip(datas, counts)]
    src, off, dst_off, total = tensors(w, datas, caps)
    dst = t.full((total,), FILL, dtype=t.uint8, device="cuda")
    res = t.full((len(datas),), RES_FILL, dtype=t.int64, device="cuda")
    o = Out()
    o.src, o.off, o.dst, o.dst_off, o.res = src, off, dst, dst_off, res
    if chunked:
        zj.batch.compress_chunked(src, off, dst, dst_off, level=level, checksum=ck, chunk=chunk, results=res)
    else:
        cut_t = off_t = None
        if raw is None and cuts is not None:
            raw = lay_out([(c, True) for c in cuts])
        if raw is not None:
            cut_t = t.tensor(raw[0], dtype=t.int64, device="cuda")
            off_t = t.tensor(raw[1], dtype=t.int64, device="cuda")
        got = zj.batch.compress_pieces(src, off, dst, dst_off, level=level, checksum=ck, chunk=chunk, cuts=cut_t, cut_off=off_t, dictionary=cd, dict_id=dict_id,
                                       sizes=sizes, piece_cap=piece_cap, results=res)
        if sizes:
            o.first, o.size = got[3].cpu().tolist(), got[4].cpu().tolist()
    t.cuda.synchronize()
    o.r, o.out, o.at = res.cpu().tolist(), dst.cpu().numpy().tobytes(), np.cumsum([3] + list(caps)).tolist()
    return o


def check_frames(w, o, datas, cuts, chunk, level, ck, cd_level=None, dict_id=True, skip=()):
    """every buffer's slot holds the reference's frames for its pieces, end to end, and FILL behind them"""
    for i, d in enumerate(datas):
        if i in skip:
            continue
        want = b"".join(ref_frame(w, p, level, ck, cd_level, dict_id) for p in pieces_of(d, None if cuts is None else cuts[i], chunk))
        assert o.r[i] == len(want), (i, len(d))
        assert o.out[o.at[i]:o.at[i] + len(want)] == want, (i, len(d))
        assert o.out[o.at[i] + len(want):o.at[i + 1]] == bytes([FILL]) * (o.at[i + 1] - o.at[i] - len(want)), i


# ---------------------------------------------------------------------------------------------- 1. parity with the existing entry
@pytest.mark.parametrize("ck", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("level", (3, 1, -3, 5))
@pytest.mark.parametrize("chunk", (256, 4096, 131072))
def test_parity_with_chunked(world, chunk, level, ck):
    w = world
    datas = [payload(w, s, 11 * k) for k, s in enumerate((0, 1, 255, 256, 257, 65536, 200000))]
    caps = [w.zj.batch.compress_bound_chunked(len(d), chunk) for d in datas]
    a = run(w, datas, chunk, level, ck, caps=caps)
    b = run(w, datas, chunk, level, ck, caps=caps, chunked=True)
    assert a.r == b.r and RES_FILL not in a.r
    assert a.out == b.out
    if level != 5:
        assert all(x > 0 for x in a.r)


# ---------------------------------------------------------------------------------------------- 2. dictionary
def round_trip(w, o, datas, dictionary):
    """the output through decompress_frames, and a range of every buffer that starts inside a piece through decompress_frames_range"""
    t, zj = w.torch, w.zj
    sizes = [len(d) for d in datas]
    packed, packed_off = zj.batch.pack(o.res, o.dst, o.dst_off)          # (generous slots: the frames of buffer i end before the next slot begins)
    back_off = t.from_numpy(np.cumsum([0] + sizes).astype(np.int64)).cuda()
    back = t.full((sum(sizes) + 64,), FILL, dtype=t.uint8, device="cuda")
    r = zj.batch.decompress_frames(packed, packed_off, back, back_off, dictionary=dictionary).cpu().tolist()
    stats = zj.batch.last_frames()
    assert r == sizes
    assert back.cpu().numpy().tobytes() == b"".join(datas) + bytes([FILL]) * 64
    ranges = [(s // 3 + 1, min(s, 9000)) for s in sizes]
    want = [d[lo:lo + ln] for d, (lo, ln) in zip(datas, ranges)]
    r_off = t.from_numpy(np.cumsum([0] + [len(x) for x in want]).astype(np.int64)).cuda()
    part = t.full((sum(len(x) for x in want) + 64,), FILL, dtype=t.uint8, device="cuda")
    rr, totals = zj.batch.decompress_frames_range(packed, packed_off, part, r_off, t.tensor(ranges, dtype=t.int64, device="cuda"), dictionary=dictionary)
    assert rr.cpu().tolist() == [len(x) for x in want] and totals.cpu().tolist() == sizes
    assert part.cpu().numpy().tobytes() == b"".join(want) + bytes([FILL]) * 64
    return stats


@pytest.mark.parametrize("ck,dict_id", ((False, True), (True, False), (True, True)), ids=("plain", "checksum-noid", "checksum"))
@pytest.mark.parametrize("chunk", (4096, 20000), ids=("attach", "copy"))
@pytest.mark.parametrize("cd_level", CD_LEVELS)
def test_dictionary_on_the_fixed_grid(world, cd_level, chunk, ck, dict_id):
    w = world
    datas = [payload(w, s, 5 * k) for k, s in enumerate((0, 1, 4095, 4096, 4097, 50000, 300000))]
    o = run(w, datas, chunk, level=9, ck=ck, cd=w.cd[cd_level], dict_id=dict_id)            # (the level argument is ignored with a dictionary)
    check_frames(w, o, datas, None, chunk, None, ck, cd_level, dict_id)
    if ck:
        stats = round_trip(w, o, datas, w.dd)
        assert stats["entries"] == sum(max(1, -(-len(d) // chunk)) for d in datas) and stats["redo"] == 0


# ---------------------------------------------------------------------------------------------- 3. cuts
def records(rnd, count, chunk, must=()):
    sizes = list(must) + [rnd.choice((1, 7, 255, chunk, rnd.randrange(1, chunk + 1), rnd.randrange(1, 600))) for _ in range(count - len(must))]
    rnd.shuffle(sizes)
    return sizes


def cut_buffers(w, rnd, chunk, counts, at=0):
    datas, cuts = [], []
    for k, c in enumerate(counts):
        sizes = records(rnd, c, chunk, must=(1, 7, 255, chunk) if c >= 4 else ())
        datas.append(payload(w, sum(sizes), at + 13 * k))
        cuts.append([int(x) for x in np.cumsum(sizes)[:-1]])
    return datas, cuts


@pytest.mark.parametrize("cd_level", (None, 3, -3), ids=("nodict", "cdict3", "cdict-3"))
def test_cuts_at_record_boundaries(world, cd_level):
    w = world
    chunk = 4096
    datas, cuts = cut_buffers(w, random.Random(41), chunk, (1, 2, 4, 30, 65, 130, 9))
    datas += [b"", payload(w, chunk, 77)]                                                   # an empty buffer and a buffer of one full piece, both without a cut
    cuts += [[], []]
    o = run(w, datas, chunk, level=1, ck=True, cuts=cuts, cd=None if cd_level is None else w.cd[cd_level], sizes=True)
    check_frames(w, o, datas, cuts, chunk, 1, True, cd_level)
    stats = round_trip(w, o, datas, None if cd_level is None else w.dd)
    assert stats["entries"] == sum(len(c) + 1 for c in cuts) == o.first[-1] and stats["redo"] == 0


@pytest.mark.parametrize("with_dict", (False, True), ids=("nodict", "cdict"))
def test_illegal_lists_among_legal_ones(world, with_dict):
    w = world
    chunk = 1000
    rnd = random.Random(7)
    bad = illegal(chunk)
    good, good_cuts = cut_buffers(w, rnd, chunk, (5, 70, 3, 12, 1, 8, 2, 6, 40, 3, 5, 4, 2, 9), at=500)
    datas, lists = [], []
    for k, name in enumerate(sorted(bad)):
        size, c, asc = bad[name]
        datas += [good[k], payload(w, size, 900 + k)]
        lists += [(good_cuts[k], True), (c, asc)]
    datas.append(good[len(bad)])
    lists.append((good_cuts[len(bad)], True))
    bad_at = set(range(1, len(datas), 2))
    caps = [len(d) + (len(d) >> 8) + 64 * (len(c) + 1) for d, (c, _) in zip(datas, lists)]
    o = run(w, datas, chunk, level=3, ck=False, raw=lay_out(lists), cd=w.cd[3] if with_dict else None, sizes=True, caps=caps)
    for i in bad_at:
        assert o.r[i] == -42, (i, sorted(bad)[i // 2])
        assert o.out[o.at[i]:o.at[i + 1]] == bytes([FILL]) * caps[i], (i, sorted(bad)[i // 2])
    cuts = [c for c, _ in lists]
    check_frames(w, o, datas, cuts, chunk, 3, False, 3 if with_dict else None, skip=bad_at)
    assert o.out[:3] == bytes([FILL]) * 3 and o.out[o.at[-1]:] == bytes([FILL]) * 64
    # the index: illegal buffers own no entry
    run_count = [0]
    for i, c in enumerate(cuts):
        run_count.append(run_count[-1] + (0 if i in bad_at else len(c) + 1))
    assert o.first == run_count and len(o.size) == run_count[-1]
    for i in range(len(datas)):
        if i not in bad_at:
            assert sum(o.size[o.first[i]:o.first[i + 1]]) == o.r[i], i


# ---------------------------------------------------------------------------------------------- 4. the index
def test_index_reads_single_records(world):
    w, t, zj = world, world.torch, world.zj
    chunk = 4096
    datas, cuts = cut_buffers(w, random.Random(3), chunk, (40, 1, 90, 7, 200))
    o = run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], sizes=True)
    counts = [len(c) + 1 for c in cuts]
    assert o.first == np.cumsum([0] + counts).tolist()
    E = o.first[-1]
    assert len(o.size) == E and all(s > 0 for s in o.size)
    starts, recs = [], []
    for i, d in enumerate(datas):
        assert sum(o.size[o.first[i]:o.first[i + 1]]) == o.r[i]
        at = o.at[i]
        for k, p in enumerate(pieces_of(d, cuts[i], chunk)):
            starts.append(at)
            recs.append(p)
            at += o.size[o.first[i] + k]
    # every third frame, by the index alone, through the plain batch decompress: frames out of order and not adjacent, so they are gathered first
    pick = list(range(0, E, 3))
    sel_off = np.cumsum([0] + [o.size[e] for e in pick]).astype(np.int64)
    sel = t.cat([o.dst[starts[e]:starts[e] + o.size[e]] for e in pick])
    want = [recs[e] for e in pick]
    out_off = t.from_numpy(np.cumsum([0] + [len(x) for x in want]).astype(np.int64)).cuda()
    out = t.full((sum(len(x) for x in want) + 64,), FILL, dtype=t.uint8, device="cuda")
    r = zj.batch.decompress(sel, t.from_numpy(sel_off).cuda(), out, out_off, dictionary=w.dd).cpu().tolist()
    assert r == [len(x) for x in want]
    assert out.cpu().numpy().tobytes() == b"".join(want) + bytes([FILL]) * 64
    # a piece_size array one entry short: 70 before any compress work, results and destination untouched
    with pytest.raises(zj.ZstdException) as e:
        run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], sizes=True, piece_cap=E - 1)
    assert e.value.getErrorCode() == 70
    src, off, dst_off, total = tensors(w, datas, [o.at[i + 1] - o.at[i] for i in range(len(datas))])
    dst = t.full((total,), FILL, dtype=t.uint8, device="cuda")
    res = t.full((len(datas),), RES_FILL, dtype=t.int64, device="cuda")
    flat, coff = lay_out([(c, True) for c in cuts])
    with pytest.raises(zj.ZstdException):
        zj.batch.compress_pieces(src, off, dst, dst_off, chunk=chunk, cuts=t.tensor(flat, dtype=t.int64, device="cuda"), cut_off=t.tensor(coff, dtype=t.int64, device="cuda"),
                                 dictionary=w.cd[3], sizes=True, piece_cap=E - 1, results=res)
    t.cuda.synchronize()
    assert bool((res == RES_FILL).all()) and bool((dst == FILL).all())
    # exactly E entries fit
    o2 = run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], sizes=True, piece_cap=E)
    assert o2.size == o.size and o2.out == o.out


# ---------------------------------------------------------------------------------------------- 5. slices and tight slots
@pytest.mark.parametrize("with_dict", (False, True), ids=("nodict", "cdict"))
def test_slices_under_a_scratch_limit(world, with_dict):
    """chunk 128 KiB: 128.5 KiB of scratch per piece, 8 157 pieces per slice under the smallest limit (4 GiB, a quarter of it for this layer): 21 000 records are three slices"""
    w, zj = world, world.zj
    L = zj.lib()
    chunk = 131072
    rnd = random.Random(19)
    datas, cuts = [], []
    for k, c in enumerate((9000, 1, 7000, 4999, 0)):
        sizes = [rnd.randrange(1, 900) for _ in range(c + 1)]
        datas.append(payload(w, sum(sizes), 1000 * k) if k != 1 else (payload(w, 600000) * 5)[:sum(sizes)])
        cuts.append([int(x) for x in np.cumsum(sizes)[:-1]])
    kw = dict(level=1, ck=False, cuts=cuts, cd=w.cd[1] if with_dict else None, sizes=True)
    whole = run(w, datas, chunk, **kw)
    assert all(x > 0 for x in whole.r) and whole.first[-1] == 21005
    assert (4 << 30) // 4 // (chunk + 512 + 48) * 2 < 21005                                # at least three slices
    try:
        assert L.zjni_set_scratch_limit(1) == (4 << 30)
        L.zjni_release_scratch()
        sliced = run(w, datas, chunk, **kw)
    finally:
        L.zjni_set_scratch_limit(0)
        L.zjni_release_scratch()
    assert sliced.r == whole.r and sliced.first == whole.first and sliced.size == whole.size
    assert sliced.out == whole.out
    for i in (1, 4):                                                                         # and the frames are the reference's (the two small buffers; the large ones by sample)
        check_frames(w, whole, datas, cuts, chunk, 1, False, 1 if with_dict else None, skip=set(range(5)) - {i})
    i, at = 2, whole.at[2]
    for k, p in enumerate(pieces_of(datas[i], cuts[i], chunk)):
        size = whole.size[whole.first[i] + k]
        if k % 97 == 0 or k == len(cuts[i]):
            assert whole.out[at:at + size] == ref_frame(w, p, 1, False, 1 if with_dict else None), k
        at += size


def test_tight_slots(world):
    w = world
    chunk = 4096
    datas, cuts = cut_buffers(w, random.Random(23), chunk, (12, 30, 5, 9))
    o = run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], sizes=True)
    totals = list(o.r)
    assert all(x > 0 for x in totals)
    exact = run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], caps=totals)
    assert exact.r == totals
    assert exact.out[3:3 + sum(totals)] == b"".join(o.out[o.at[i]:o.at[i] + totals[i]] for i in range(4)) and exact.out[3 + sum(totals):] == bytes([FILL]) * 64
    caps = [totals[0], totals[1] - 1, totals[2], totals[3]]
    short = run(w, datas, chunk, ck=True, cuts=cuts, cd=w.cd[3], caps=caps)
    assert short.r == [totals[0], -70, totals[2], totals[3]]
    for i in (0, 2, 3):
        assert short.out[short.at[i]:short.at[i + 1]] == o.out[o.at[i]:o.at[i] + totals[i]], i
    assert short.out[short.at[4]:] == bytes([FILL]) * 64 and short.out[:3] == bytes([FILL]) * 3
    # what did fit of the short buffer lies at its slot's beginning, frame by frame; nothing else of the slot was written
    whole = o.out[o.at[1]:o.at[1] + totals[1]]
    sizes = o.size[o.first[1]:o.first[2]]
    fit = sum(sizes[:-1])
    assert short.out[short.at[1]:short.at[1] + fit] == whole[:fit] and short.out[short.at[1] + fit:short.at[2]] == bytes([FILL]) * (caps[1] - fit)


# ---------------------------------------------------------------------------------------------- 6. refusals, no buffers, the host form
def test_refusals(world):
    w, zj = world, world.zj
    data = [payload(w, 1000)]
    for bad in (255, 131073):
        with pytest.raises(zj.ZstdException) as e:
            run(w, data, bad, caps=[4096])
        assert e.value.getErrorCode() == 42
    t = w.torch
    src, off, dst_off, total = tensors(w, data, [4096])
    dst = t.full((total,), FILL, dtype=t.uint8, device="cuda")
    res = t.full((1,), RES_FILL, dtype=t.int64, device="cuda")
    L = zj.lib()
    for flags, cd in ((2, None), (3, None), (2, w.cd[3]._ptr)):                              # ZJNI_FRAME_NO_CONTENTSIZE
        r = L.zjni_compress_pieces_batch_device(src.data_ptr(), off.data_ptr(), dst.data_ptr(), dst_off.data_ptr(), res.data_ptr(), 1, 3, flags, 4096, None, None, cd,
                                                None, None, 0, t.cuda.current_stream().cuda_stream)
        assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 42
    with pytest.raises(zj.ZstdException) as e:
        run(w, data, 4096, level=9, caps=[4096])                                            # a level that is not served
    assert e.value.getErrorCode() == 42
    t.cuda.synchronize()
    assert bool((res == RES_FILL).all()) and bool((dst == FILL).all())
    z = t.zeros(1, dtype=t.int64, device="cuda")
    e8 = t.empty(8, dtype=t.uint8, device="cuda")
    got = zj.batch.compress_pieces(e8, z, e8, z, sizes=True)
    assert got[2].numel() == 0 and got[3].cpu().tolist() == [0] and got[4].numel() == 0


def test_host_forms(world):
    w, zj = world, world.zj
    L = zj.lib()
    chunk = 4096
    (data,), (cuts,) = cut_buffers(w, random.Random(5), chunk, (25,))
    want = [ref_frame(w, p, None, True, 3) for p in pieces_of(data, cuts, chunk)]
    cap = L.zjni_compressBound_pieces(len(data), len(cuts) + 1)
    assert cap == len(data) + (len(data) >> 8) + 64 * 25
    dst = C.create_string_buffer(cap)
    sizes = (C.c_uint64 * 25)()
    count = C.c_size_t(0)
    cut_arr = (C.c_uint64 * len(cuts))(*cuts)
    n = L.zjni_compress_pieces(dst, cap, data, len(data), 0, 1, chunk, cut_arr, len(cuts), w.cd[3]._ptr, sizes, 25, C.byref(count))
    assert not L.zjni_isError(n) and count.value == 25 and list(sizes) == [len(x) for x in want] and dst.raw[:n] == b"".join(want)
    assert L.zjni_getErrorCode(L.zjni_compress_pieces(dst, cap, data, len(data), 0, 1, chunk, cut_arr, len(cuts), w.cd[3]._ptr, sizes, 24, None)) == 70
    assert L.zjni_getErrorCode(L.zjni_compress_pieces(dst, n - 1, data, len(data), 0, 1, chunk, cut_arr, len(cuts), w.cd[3]._ptr, None, 0, None)) == 70
    frames = dst.raw[:n]
    plain = C.create_string_buffer(len(data))
    assert L.zjni_decompress_frames_usingDDict(plain, len(data), frames, n, w.dd._ptr) == len(data) and plain.raw == data
    total = C.c_ulonglong(0)
    lo = cuts[3] + 1
    ln = min(5000, len(data) - lo)
    part = C.create_string_buffer(ln)
    assert L.zjni_decompress_frames_range_usingDDict(part, ln, frames, n, lo, ln, C.byref(total), w.dd._ptr) == ln
    assert part.raw == data[lo:lo + ln] and total.value == len(data)
    # without cuts and without a dictionary: zjni_compress_chunked's bytes
    grid = C.create_string_buffer(cap)
    m = L.zjni_compress_pieces(grid, cap, data, len(data), 3, 0, chunk, None, 0, None, None, 0, C.byref(count))
    old = C.create_string_buffer(cap)
    assert m == L.zjni_compress_chunked(old, cap, data, len(data), 3, 0, chunk) and grid.raw[:m] == old.raw[:m] and count.value == -(-len(data) // chunk)
