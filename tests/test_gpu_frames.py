"""GPU (-m gpu): large buffers as many frames.  zjni_decompress_frames_batch_device against zjni_decompress_batch_device[_usingDDict] on the same tensors (the
existing entry is the yardstick: same results, same bytes) and against the original data, with zjni_last_frames saying that the buffers were really split and
none was decoded twice; zjni_compress_chunked_batch_device against the reference's frame for every piece, byte for byte; the round trip of the two and the
blocking host forms.  The CPU twin of the arithmetic is tests/test_emu_frames.py."""
import ctypes as C
import random

import numpy as np
import pytest

import inspect_cases as ic
from util import json_records

pytestmark = pytest.mark.gpu

FILL = 0xCD


class World:
    pass


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    import torch
    zj.batch.init(0)
    w = World()
    w.torch, w.zj, w.ref = torch, zj, oracle_ref
    rnd = random.Random(12)
    text = b",".join(json_records(3000, seed=9))
    noise = zj.synth_host(65536, 5, 1)
    w.pool = []                                          # (original, frame): 256 B - 4 KiB payloads, levels 1 and 3, every third with a checksum
    for k in range(97):
        size = rnd.choice((256, 300, 511, 700, 1024, 1500, 4096)) if k % 5 else rnd.randrange(256, 4097)
        at = rnd.randrange(0, len(text) - size)
        orig = text[at:at + size] if k % 4 else noise[at % 60000:at % 60000 + size]
        w.pool.append((orig, oracle_ref.compress(orig, 1 if k & 1 else 3, checksum=(k % 3 == 0)), k % 3 == 0))
    w.dict_bytes = ic.dictionary(oracle_ref)
    w.ddict = zj.ZstdDictDecompress(w.dict_bytes)
    w.other_dict = oracle_ref.train_dict(json_records(1500, seed=77), 4096)
    w.other_ddict = zj.ZstdDictDecompress(w.other_dict)
    yield w
    w.ddict.close()
    w.other_ddict.close()


def many(w, count, start):
    """(buffer, original) of `count` frames of the pool, from `start` on"""
    pieces = [w.pool[(start + j) % len(w.pool)] for j in range(count)]
    return b"".join(p[1] for p in pieces), b"".join(p[0] for p in pieces)


def tensors(w, bufs, caps, lead=1):
    t = w.torch
    blob = b"\xAA" * lead + b"".join(bufs)
    assert len(blob) < 16 << 20 and sum(caps) < 48 << 20
    src = t.frombuffer(bytearray(blob), dtype=t.uint8).cuda()
    off = t.from_numpy(np.cumsum([lead] + [len(b) for b in bufs]).astype(np.int64)).cuda()
    dst_off = t.from_numpy(np.cumsum([3] + list(caps)).astype(np.int64)).cuda()
    return src, off, dst_off, 3 + sum(caps) + 64


def both(w, bufs, caps, dictionary=None):
    """the new entry and the existing one on the same tensors -> (results, bytes, results of the existing entry, bytes, last_frames, dst offsets)"""
    t, zj = w.torch, w.zj
    src, off, dst_off, total = tensors(w, bufs, caps)
    dst = t.full((total,), FILL, dtype=t.uint8, device="cuda")
    res = zj.batch.decompress_frames(src, off, dst, dst_off, dictionary=dictionary)
    stats = zj.batch.last_frames()
    dst2 = t.full((total,), FILL, dtype=t.uint8, device="cuda")
    res2 = zj.batch.decompress(src, off, dst2, dst_off, dictionary=dictionary)
    t.cuda.synchronize()
    return res.cpu().tolist(), dst.cpu().numpy().tobytes(), res2.cpu().tolist(), dst2.cpu().numpy().tobytes(), stats, np.cumsum([3] + list(caps)).tolist()


def check_parity(w, counts, start=0):
    made = [many(w, c, start + 13 * i) for i, c in enumerate(counts)]
    bufs, origs = [m[0] for m in made], [m[1] for m in made]
    r, out, r2, out2, stats, at = both(w, bufs, [len(o) for o in origs])
    assert r == r2 == [len(o) for o in origs]
    assert out == out2
    for i, o in enumerate(origs):
        assert out[at[i]:at[i + 1]] == o, i
    split = sum(c >= 2 for c in counts)
    assert stats == {"split": split, "entries": sum(counts), "unsplit": len(counts) - split, "redo": 0}


@pytest.mark.parametrize("count", (1, 2, 63, 64, 65, 257, 1025))
def test_one_buffer_of_many_frames(world, count):
    check_parity(world, [count], start=count)


@pytest.mark.parametrize("counts", ([2, 65, 1], [1025, 1, 257], [64, 63, 2]), ids=("2-65-1", "1025-1-257", "64-63-2"))
def test_three_buffers(world, counts):
    check_parity(world, counts)


def test_seventy_buffers(world):
    check_parity(world, [1, 2, 63, 64, 65, 257] * 11 + [1025] * 4, start=5)


def test_more_than_4096_entries_take_the_inner_pipeline(world):
    check_parity(world, [1025] * 5, start=1)
    lists = (C.c_uint * 4)()
    assert world.zj.lib().zjni_last_decode_lists(lists) == 0
    assert lists[0] + lists[1] + lists[2] > 0                     # the three-stage pipeline's lists were filled by this call's 5 125 entries


def test_mixed_call(world):
    w, ref = world, world.ref
    a, ao = many(w, 65, 3)
    b, bo = many(w, 2, 9)
    single, so = many(w, 1, 4)
    sdata = ic.stream_data(70000)
    stream = ref.compress_stream(sdata, 3, chunk=20000, flush_every=1)          # no content size
    cut = a[:len(a) - 9]
    garbage = bytes(random.Random(3).getrandbits(8) for _ in range(500))
    bufs = [a, single, b"", stream, b, cut, garbage, a + stream, a]
    caps = [len(ao), len(so), 16, len(sdata), len(bo), len(ao), 4096, len(ao) + len(sdata), len(ao)]
    r, out, r2, out2, stats, at = both(w, bufs, caps)
    assert r == r2
    assert r[0] == len(ao) and r[1] == len(so) and r[3] == len(sdata) and r[4] == len(bo) and r[5] < 0 and r[6] < 0 and r[7] == len(ao) + len(sdata)
    for i, o in ((0, ao), (1, so), (3, sdata), (4, bo), (7, ao + sdata), (8, ao)):
        assert out[at[i]:at[i] + len(o)] == o == out2[at[i]:at[i] + len(o)], i
    assert stats == {"split": 3, "entries": 65 + 2 + 65 + 6, "unsplit": 6, "redo": 0}


def test_skippable_and_empty_frames(world):
    w, ref = world, world.ref
    S = ic.skippable
    empty, empty_ck = ref.compress(b"", 3), ref.compress(b"", 1, checksum=True)
    f = [w.pool[k] for k in range(6)]
    bufs = [S(b"index") + f[0][1] + f[1][1],
            f[0][1] + S(b"") + f[1][1] + S(b"xy", 7) + f[2][1],
            f[3][1] + f[4][1] + S(b"trailer", 15),
            empty + f[5][1] + empty_ck + empty,
            empty + empty,
            S(b"alone")]
    origs = [f[0][0] + f[1][0], f[0][0] + f[1][0] + f[2][0], f[3][0] + f[4][0], f[5][0], b"", b""]
    r, out, r2, out2, stats, at = both(w, bufs, [len(o) + (7 if i & 1 else 0) for i, o in enumerate(origs)])
    assert r == r2 == [len(o) for o in origs] and out == out2
    for i, o in enumerate(origs):
        assert out[at[i]:at[i] + len(o)] == o, i
    assert stats == {"split": 5, "entries": 3 + 5 + 3 + 4 + 2 + 1, "unsplit": 1, "redo": 0}


def test_dictionary_frames(world):
    w, ref = world, world.ref
    recs = json_records(60, seed=21)
    origs = [b",".join(recs[k:k + 3]) for k in range(0, 60, 3)]
    frames = [ref.compress_using_dict(o, w.dict_bytes, 3) for o in origs]
    bufs = [b"".join(frames), frames[0], b"".join(frames[:2]) + w.pool[0][1]]
    want = [b"".join(origs), origs[0], origs[0] + origs[1] + w.pool[0][0]]
    caps = [len(x) for x in want]
    r, out, r2, out2, stats, at = both(w, bufs, caps, dictionary=w.ddict)
    assert r == r2 == caps and out == out2
    for i, o in enumerate(want):
        assert out[at[i]:at[i + 1]] == o, i
    assert stats == {"split": 2, "entries": 20 + 1 + 3, "unsplit": 1, "redo": 0}
    # the wrong dictionary, and none: the existing entry's dictionary_wrong (32), reached through the redo list
    for dd in (w.other_ddict, None):
        r, out, r2, out2, stats, at = both(w, bufs, caps, dictionary=dd)
        assert r == r2 and r[0] == -32 and r[1] == -32 and r[2] == -32
        assert stats["split"] == 2 and stats["redo"] == 2


def test_damage_the_walk_cannot_see(world):
    w = world
    pieces = [w.pool[(3 * j) % len(w.pool)] if j == 32 else w.pool[(j + 1) % len(w.pool)] for j in range(65)]      # the middle frame carries a checksum
    assert pieces[32][2]
    good, orig = b"".join(p[1] for p in pieces), b"".join(p[0] for p in pieces)
    start = sum(len(p[1]) for p in pieces[:32])
    flipped = bytearray(good)
    flipped[start + len(pieces[32][1]) // 2] ^= 0x10                # inside the middle frame's block content
    sums = bytearray(good)
    last_ck = max(j for j in range(65) if pieces[j][2])
    sums[sum(len(p[1]) for p in pieces[:last_ck + 1]) - 2] ^= 0xFF    # inside a frame's checksum
    bufs = [good, bytes(flipped), good, bytes(sums), good]
    r, out, r2, out2, stats, at = both(w, bufs, [len(orig)] * 5)
    assert r == r2
    assert r[1] < 0 and r[3] == -22 and r[0] == r[2] == r[4] == len(orig)
    for i in (0, 2, 4):
        assert out[at[i]:at[i + 1]] == orig, i
    assert stats["split"] == 5 and stats["entries"] == 5 * 65 and stats["redo"] == 2


def test_capacity(world):
    w = world
    a, ao = many(w, 65, 2)
    b, bo = many(w, 64, 40)
    garbage = b"\x00" * 100
    # exact and generous slots pass
    r, out, r2, out2, stats, at = both(w, [a, b], [len(ao), len(bo) + 1000])
    assert r == r2 == [len(ao), len(bo)] and stats["redo"] == 0
    assert out[at[0]:at[1]] == ao and out[at[1]:at[1] + len(bo)] == bo and out[at[1] + len(bo):at[2]] == bytes([FILL]) * 1000
    # one byte short: 70 like the existing entry, and nothing behind the slot is touched (a buffer nobody writes lies there)
    r, out, r2, out2, stats, at = both(w, [a, garbage, b], [len(ao) - 1, 64, len(bo)])
    assert r == r2 and r[0] == -70 and r[1] < 0 and r[2] == len(bo)
    assert out[at[1]:at[2]] == bytes([FILL]) * 64 == out2[at[1]:at[2]]
    assert out[at[2]:at[3]] == bo and out[at[3]:] == bytes([FILL]) * 64
    assert stats["redo"] == 1
    # far too short, and no slot at all
    r, out, r2, out2, stats, at = both(w, [a, b, a], [100, len(bo), 0])
    assert r == r2 and r[0] == -70 and r[1] == len(bo) and r[2] == -70
    assert out[at[1]:at[2]] == bo and out[at[3]:] == bytes([FILL]) * 64


def test_no_buffers(world):
    t, zj = world.torch, world.zj
    z = t.zeros(1, dtype=t.int64, device="cuda")
    e = t.empty(8, dtype=t.uint8, device="cuda")
    assert zj.batch.decompress_frames(e, z, e, z).numel() == 0
    assert zj.batch.last_frames() == {"split": 0, "entries": 0, "unsplit": 0, "redo": 0}
    _, _, res = zj.batch.compress_chunked(e, z, e, z)
    assert res.numel() == 0


# ---------------------------------------------------------------------------------------------- chunked compress
CHUNKS = (256, 1000, 4096, 65536, 131072)
_payload = {}


def payload(w, size):
    """compressible bytes with an incompressible stretch, the same for every test"""
    if size not in _payload:
        text = b",".join(json_records(1200, seed=4))
        body = (text + w.zj.synth_host(65536, 3, 1)) * (size // (len(text) + 65536) + 1)
        _payload[size] = body[:size]
    return _payload[size]


_ref_frames = {}


def ref_chunked(w, data, chunk, level, ck):
    key = (len(data), chunk, level, ck)
    if key not in _ref_frames:
        pieces = [data[k:k + chunk] for k in range(0, len(data), chunk)] or [b""]
        _ref_frames[key] = b"".join(w.ref.compress(p, level, checksum=ck) for p in pieces)
    return _ref_frames[key]


def run_chunked(w, datas, chunk, level, ck, caps=None, tail=64):
    t, zj = w.torch, w.zj
    L = zj.lib()
    if caps is None:
        caps = [L.zjni_compressBound_chunked(len(d), chunk) for d in datas]
    src, off, dst_off, total = tensors(w, datas, caps, lead=5)
    dst = t.full((total - 64 + tail,), FILL, dtype=t.uint8, device="cuda")
    _, _, res = zj.batch.compress_chunked(src, off, dst, dst_off, level=level, checksum=ck, chunk=chunk)
    t.cuda.synchronize()
    return res.cpu().tolist(), dst.cpu().numpy().tobytes(), np.cumsum([3] + list(caps)).tolist()


def sizes_of(chunk):
    return [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_chunked_one_buffer(world, chunk):
    w = world
    for size in sizes_of(chunk):
        data = payload(w, size)
        want = ref_chunked(w, data, chunk, 3, False)
        r, out, at = run_chunked(w, [data], chunk, 3, False)
        assert r == [len(want)] and out[at[0]:at[0] + r[0]] == want, size
        assert w.ref.decompress(want, size) == data                     # every zstd decoder reads the pieces as one buffer
        # a slot of exactly the total passes; one byte less answers 70 and leaves what lies behind the slot alone
        r, out, at = run_chunked(w, [data], chunk, 3, False, caps=[len(want)])
        assert r == [len(want)] and out[at[0]:at[1]] == want and out[at[1]:] == bytes([FILL]) * 64
        r, out, at = run_chunked(w, [data], chunk, 3, False, caps=[len(want) - 1])
        assert r == [-70] and out[at[1]:] == bytes([FILL]) * 64, size


# level 5 above 16 KiB parses with one lane per frame (exact, not fast): its large chunks run in test_chunked_level5_large_chunks with a few buffers
GRID = [(chunk, level) for chunk in CHUNKS for level in (1, 3, -3, 5) if not (level == 5 and chunk > 4096)]


@pytest.mark.parametrize("ck", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("chunk,level", GRID)
def test_chunked_sixty_five_buffers(world, chunk, level, ck):
    w = world
    sizes = sizes_of(chunk)
    datas = [payload(w, sizes[(i * 5 + i // 6) % 6]) for i in range(65)]
    wants = [ref_chunked(w, d, chunk, level, ck) for d in datas]
    caps = [len(x) if i % 3 == 0 else len(x) + 40 for i, x in enumerate(wants)]      # exact slots among generous ones: a frame placed wrongly shows in a neighbour
    r, out, at = run_chunked(w, datas, chunk, level, ck, caps=caps)
    assert r == [len(x) for x in wants]
    for i, x in enumerate(wants):
        assert out[at[i]:at[i] + len(x)] == x, (i, len(datas[i]))
        assert out[at[i] + len(x):at[i + 1]] == bytes([FILL]) * (caps[i] - len(x)), i
    assert w.ref.decompress(wants[5], len(datas[5])) == datas[5]


@pytest.mark.parametrize("ck", (False, True), ids=("plain", "checksum"))
@pytest.mark.parametrize("chunk", (65536, 131072))
def test_chunked_level5_large_chunks(world, chunk, ck):
    """whatever the plain entry answers for such a piece: its frame, which is the reference's, or its refusal"""
    w, t, zj = world, world.torch, world.zj
    L = zj.lib()
    datas = [payload(w, s) for s in (chunk, chunk + 1, 3 * chunk + 5)]
    r, out, at = run_chunked(w, datas, chunk, 5, ck)
    for i, d in enumerate(datas):
        pieces = [d[k:k + chunk] for k in range(0, len(d), chunk)]
        src, off, dst_off, total = tensors(w, pieces, [L.zjni_compressBound(len(p)) for p in pieces])
        dst = t.full((total,), FILL, dtype=t.uint8, device="cuda")
        plain = zj.batch.compress(src, off, dst, dst_off, level=5, checksum=ck).cpu().tolist()
        po, pat = dst.cpu().numpy().tobytes(), dst_off.cpu().tolist()
        errors = [x for x in plain if x < 0]
        if errors:
            assert r[i] == errors[0], (i, plain)
        else:
            want = b"".join(po[pat[k]:pat[k] + plain[k]] for k in range(len(pieces)))
            assert r[i] == len(want) and out[at[i]:at[i] + r[i]] == want, i
            assert want == ref_chunked(w, d, chunk, 5, ck), i


def test_chunked_more_than_4096_entries(world):
    w = world
    datas = [payload(w, s) for s in (400000, 256 * 1500, 410001)]
    for level, ck in ((3, True), (1, False)):
        wants = [ref_chunked(w, d, 256, level, ck) for d in datas]
        r, out, at = run_chunked(w, datas, 256, level, ck)
        assert r == [len(x) for x in wants]
        for i, x in enumerate(wants):
            assert out[at[i]:at[i] + len(x)] == x, i


def test_chunked_short_slot_between_neighbours(world):
    """the total decides: a buffer one byte short answers 70, its neighbours are whole, and nothing lies outside any slot"""
    w = world
    chunk = 1000
    datas = [payload(w, s) for s in (3 * chunk + 5, 10 * chunk + 1, chunk, 7 * chunk)]
    wants = [ref_chunked(w, d, chunk, 3, False) for d in datas]
    caps = [len(wants[0]), len(wants[1]) - 1, len(wants[2]), 10]
    r, out, at = run_chunked(w, datas, chunk, 3, False, caps=caps)
    assert r == [len(wants[0]), -70, len(wants[2]), -70]
    assert out[:3] == bytes([FILL]) * 3 and out[at[0]:at[1]] == wants[0] and out[at[2]:at[3]] == wants[2] and out[at[4]:] == bytes([FILL]) * 64


def test_chunk_size_out_of_range(world):
    w, zj = world, world.zj
    for bad in (255, 131073):
        with pytest.raises(zj.ZstdException) as e:
            run_chunked(w, [payload(w, 1000)], bad, 3, False, caps=[4096])
        assert e.value.getErrorCode() == 42
    with pytest.raises(zj.ZstdException) as e:
        run_chunked(w, [payload(w, 1000)], 1000, 9, False, caps=[4096])
    assert e.value.getErrorCode() == 42


# ---------------------------------------------------------------------------------------------- round trip, host forms
def test_round_trip_of_large_buffers(world):
    w, t, zj = world, world.torch, world.zj
    mib = 1 << 20
    src = zj.batch.synth(9, mib)
    off = t.tensor([0, mib, 4 * mib + 17, 9 * mib], dtype=t.int64, device="cuda")
    comp, comp_off, res = zj.batch.compress_chunked(src, off, level=3, checksum=True, chunk=65536)
    sizes = res.cpu().tolist()
    assert all(0 < s < mib * 6 for s in sizes)
    packed, packed_off = zj.batch.pack(res, comp, comp_off)
    back = t.full((9 * mib + 64,), FILL, dtype=t.uint8, device="cuda")
    r = zj.batch.decompress_frames(packed, packed_off, back, off).cpu().tolist()
    assert r == [mib, 3 * mib + 17, 5 * mib - 17]
    assert t.equal(back[:9 * mib], src) and bool((back[9 * mib:] == FILL).all())
    assert zj.batch.last_frames() == {"split": 3, "entries": 16 + 49 + 80, "unsplit": 0, "redo": 0}
    # the first buffer through the reference, and through the blocking host forms
    host_src = src[:mib].cpu().numpy().tobytes()
    frames0 = packed[:sizes[0]].cpu().numpy().tobytes()
    assert w.ref.decompress(frames0, mib) == host_src
    L = zj.lib()
    cap = L.zjni_compressBound_chunked(mib, 65536)
    dst = C.create_string_buffer(cap)
    n = L.zjni_compress_chunked(dst, cap, host_src, mib, 3, 1, 65536)
    assert n == sizes[0] and dst.raw[:n] == frames0
    assert L.zjni_getErrorCode(L.zjni_compress_chunked(dst, n - 1, host_src, mib, 3, 1, 65536)) == 70
    plain = C.create_string_buffer(mib)
    assert L.zjni_decompress_frames(plain, mib, frames0, n) == mib and plain.raw == host_src
    assert L.zjni_getErrorCode(L.zjni_decompress_frames(plain, mib - 1, frames0, n)) == 70
    assert L.zjni_decompress_frames(plain, mib, frames0, n) == L.zjni_decompress(plain, mib, frames0, n)
