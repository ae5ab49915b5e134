"""GPU (-m gpu): range reads by a caller-held index.  zjni_decompress_index_range_batch_device against zjni_decompress_frames_range_batch_device on the same buffers
(results, totals and the whole 0xCD-filled destination) and against the source bytes sliced; the builders against a model on the host; the edges of the scan
workgroup and of the lane-per-entry grid; many requests per buffer; false indexes and the codes the header names for them, with the neighbours of the same call
unaffected and nothing written outside the slots; the host form against zjni_decompress_frames_range.  Buffers are made by batch.compress_pieces at chunk 256 ..
4096.  The CPU twin of the arithmetic is tests/test_emu_index.py."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import inspect_cases as ic
from util import json_records

pytestmark = pytest.mark.gpu

FILL = 0xCD
MAXU = (1 << 64) - 1
SIZE_MAX = (1 << 32) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class World:
    pass


class Store:
    """n buffers compressed piece by piece and packed end to end, with everything the compress call took and gave"""


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    import torch
    zj.batch.init(0)
    w = World()
    w.torch, w.zj, w.ref = torch, zj, oracle_ref
    w.text = b",".join(json_records(6000, seed=21))
    w.noise = zj.synth_host(65536, 5, 1)
    w.dict_bytes = ic.dictionary(oracle_ref)
    w.ddict = zj.ZstdDictDecompress(w.dict_bytes)
    w.cdict = zj.ZstdDictCompress(w.dict_bytes, 3)
    w.stores = {}
    yield w
    w.ddict.close()
    w.cdict.close()


def dev(w, values):
    return w.torch.from_numpy(np.array([int(v) & MAXU for v in values], dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def store(w, sizes, chunk, checksum=False, dictionary=False, cuts=None, seed=0):
    key = (tuple(sizes), chunk, checksum, dictionary, None if cuts is None else tuple(map(tuple, cuts)), seed)
    if key in w.stores:
        return w.stores[key]
    t, zj = w.torch, w.zj
    s = Store()
    rnd = random.Random(seed)
    s.whole = []
    for k, size in enumerate(sizes):
        at = rnd.randrange(0, len(w.text) - size)
        s.whole.append(w.text[at:at + size] if k % 3 != 2 else (w.noise * (size // len(w.noise) + 1))[:size])
    s.n, s.chunk = len(sizes), chunk
    s.usrc = t.frombuffer(bytearray(b"".join(s.whole) + b"\0"), dtype=t.uint8).cuda()
    s.usrc_off = dev(w, np.cumsum([0] + list(sizes)))
    s.cuts = s.cut_off = None
    if cuts is not None:
        s.cuts, s.cut_off = dev(w, [c for cs in cuts for c in cs] + [0]), dev(w, np.cumsum([0] + [len(cs) for cs in cuts]))
    blob, off, s.results, s.first, s.psize = zj.batch.compress_pieces(s.usrc, s.usrc_off, chunk=chunk, checksum=checksum, cuts=s.cuts, cut_off=s.cut_off, sizes=True,
                                                                      dictionary=w.cdict if dictionary else None)
    s.src, s.off = zj.batch.pack(s.results, blob, off)
    s.E = s.psize.numel()
    s.index = zj.batch.index_from_pieces(s.usrc_off, s.results, s.first, s.psize, chunk=chunk, cuts=s.cuts, cut_off=s.cut_off)
    s.h_first, s.h_psize, s.h_results = host(s.first), host(s.psize), host(s.results)
    s.contents = []                                     # per buffer: the entries' content sizes, from the cuts or the grid
    for i, size in enumerate(sizes):
        edges = [0] + list(cuts[i]) + [size] if cuts is not None else list(range(0, size, chunk)) + [size] if size else [0, 0]
        s.contents.append([b - a for a, b in zip(edges[:-1], edges[1:])])
    s.ddict = w.ddict if dictionary else None
    w.stores[key] = s
    return s


def model_index(first, sizes, contents, results=None):
    n, E = len(first) - 1, len(sizes)
    valid = []
    for i in range(n):
        ok = first[i] <= first[i + 1] <= E and all(sizes[e] <= SIZE_MAX and contents[e] <= SIZE_MAX for e in range(first[i], first[i + 1]))
        valid.append((1 << 64) - results[i] if results is not None and results[i] > 1 << 40 else 0 if ok else 42)
    c, u = [0], [0]
    for a, b in zip(sizes, contents):
        c.append(c[-1] + (a if a <= SIZE_MAX else 0))
        u.append(u[-1] + (b if b <= SIZE_MAX else 0))
    return list(first) + valid + c + u


def expect(s, b, lo, length, slot, contents=None):
    """(result, bytes, entries decoded, edges) of one request by rules 2-5 from the source bytes"""
    whole, sizes = s.whole[b], (contents or s.contents)[b]
    T = len(whole)
    lo2, hi2 = min(lo, T), min(lo + length, T)
    if lo2 == hi2:
        return 0, b"", 0, 0
    if slot < hi2 - lo2:
        return -70, b"", 0, 0
    pre = np.cumsum([0] + sizes).tolist()
    first = max(k for k in range(len(sizes)) if sizes[k] and pre[k] <= lo2)
    last = max(k for k in range(len(sizes)) if sizes[k] and pre[k] <= hi2 - 1)
    e_first, e_last = pre[first] < lo2, pre[last + 1] > hi2
    edges = int(e_first or e_last) if first == last else int(e_first) + int(e_last)
    return hi2 - lo2, whole[lo2:hi2], last - first + 1, edges


def read(w, s, requests, slots, index=None, entries=None, totals=True, n=None, src=None):
    """one indexed call -> (results, destination bytes, totals, last_index_range, slot offsets)"""
    t, zj = w.torch, w.zj
    at = np.cumsum([3] + list(slots)).tolist()
    dst_off = t.tensor(at, dtype=t.int64, device="cuda")
    dst = t.full((at[-1] + 64,), FILL, dtype=t.uint8, device="cuda")
    req = dev(w, [v for r in requests for v in r])
    off = s.off if n is None else s.off[:n + 1]
    res, tot = zj.batch.decompress_index_range(s.src if src is None else src, off, s.index if index is None else index, s.E if entries is None else entries, req, dst, dst_off,
                                               dictionary=s.ddict)
    stats = zj.batch.last_index_range()
    signed = lambda xs: [int(x) for x in xs.cpu().tolist()]      # noqa: E731
    return signed(res), dst.cpu().numpy().tobytes(), signed(tot), stats, at


def check(w, s, requests, slack=2, slots=None, **kw):
    """the call against the source bytes sliced, every byte of the destination included; and the diagnostics"""
    wants = [min(lo + ln, len(s.whole[b])) - min(lo, len(s.whole[b])) for b, lo, ln in requests]
    if slots is None:
        slots = [x + (slack if i & 1 else 0) for i, x in enumerate(wants)]
    exp = [expect(s, b, lo, ln, slots[i]) for i, (b, lo, ln) in enumerate(requests)]
    r, out, tot, stats, at = read(w, s, requests, slots, **kw)
    assert r == [e[0] for e in exp]
    assert tot == [len(s.whole[b]) for b, _, _ in requests]
    image = bytearray(bytes([FILL]) * len(out))
    for i, e in enumerate(exp):
        image[at[i]:at[i] + len(e[1])] = e[1]
    assert out == bytes(image)
    assert stats == {"served": sum(e[0] >= 0 for e in exp), "entries": sum(e[2] for e in exp), "edges": sum(e[3] for e in exp), "errors": sum(e[0] < 0 for e in exp)}
    return r, out, at


def boundary_ranges(contents, T, count, rnd):
    ends = {0, T, T + 1, MAXU}
    run = 0
    for c in contents:
        run += c
        ends |= {max(run - 1, 0), run, run + 1}
    ends = sorted(ends)
    pairs = [(lo, hi - lo) for lo in ends for hi in ends if hi >= lo]
    must = [(0, MAXU), (0, T), (T, 5), (T + 1, MAXU), (0, 0), (1, max(T - 2, 0))]
    return must + (pairs if len(pairs) <= count else rnd.sample(pairs, count))


# ------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("variant", ["plain", "dictionary", "checksum"])
def test_one_request_per_buffer_equals_the_walked_entry(world, variant):
    """n = 5 buffers of 1 .. 40 entries, a request each over the boundary set: results, totals and the whole destination equal decompress_frames_range's on the
    same buffers, and the source bytes sliced"""
    w, t = world, world.torch
    chunk = {"plain": 512, "dictionary": 1024, "checksum": 256}[variant]
    sizes = [chunk - 212, 2 * chunk - 5, 7 * chunk, 23 * chunk - 100, 40 * chunk]
    s = store(w, sizes, chunk, checksum=variant == "checksum", dictionary=variant == "dictionary", seed=3)
    assert [len(c) for c in s.contents] == [1, 2, 7, 23, 40] and s.h_first == [0, 1, 3, 10, 33, 73] and all(r < 1 << 40 for r in s.h_results)
    rnd = random.Random(8)
    per = [boundary_ranges(s.contents[b], sizes[b], 50, rnd) for b in range(5)]
    for k in range(max(len(p) for p in per)):
        ranges = [per[b][k % len(per[b])] for b in range(5)]
        requests = [(b, lo, ln) for b, (lo, ln) in enumerate(ranges)]
        wants = [min(lo + ln, sizes[b]) - min(lo, sizes[b]) for b, lo, ln in requests]
        slots = [max(x - 1, 0) if (k + i) % 9 == 0 else x + (i % 3) for i, x in enumerate(wants)]
        r, out, tot, stats, at = read(w, s, requests, slots)
        dst_off = t.tensor(at, dtype=t.int64, device="cuda")
        dst2 = t.full((at[-1] + 64,), FILL, dtype=t.uint8, device="cuda")
        res2, tot2 = w.zj.batch.decompress_frames_range(s.src, s.off, dst2, dst_off, dev(w, [v for rg in ranges for v in rg]), dictionary=s.ddict)
        walked = w.zj.batch.last_frames_range()
        assert r == res2.cpu().tolist() and tot == tot2.cpu().tolist(), (k, ranges)
        assert out == dst2.cpu().numpy().tobytes(), (k, ranges)
        assert stats == {"served": walked["served"], "entries": walked["frames"], "edges": walked["edges"], "errors": walked["errors"]}
        exp = [expect(s, b, lo, ln, slots[i]) for i, (b, lo, ln) in enumerate(requests)]
        assert r == [e[0] for e in exp]
        for i, e in enumerate(exp):
            assert out[at[i]:at[i] + len(e[1])] == e[1]


# ------------------------------------------------------------------------------------------------ the builders and the scan workgroup's tile
@pytest.mark.parametrize("E", [1023, 1024, 1025, 2049, 2500])
def test_scan_boundary(world, E):
    """E one below, at and one above the scan workgroup's tile, above twice the tile; three buffers, so the bases in C and U are not 0; pieces of 256 bytes"""
    w = world
    header = open(os.path.join(ROOT, "zstd-jni_amd", "csrc", "zj_index.h")).read()
    assert int(re.search(r"#define ZJ_INDEX_SCAN_WG (\d+)u", header).group(1)) == 1024
    counts = [E // 3, E // 3 + 1, E - 2 * (E // 3) - 1]
    sizes = [256 * c - (7 if k == 1 else 0) for k, c in enumerate(counts)]
    s = store(w, sizes, 256, seed=E)
    assert s.E == E and s.h_first == np.cumsum([0] + counts).tolist()
    flat = [c for cs in s.contents for c in cs]
    want = model_index(s.h_first, s.h_psize, flat, s.h_results)
    got = host(s.index)
    assert got[:len(want)] == want and len(got) * 8 == w.zj.batch.index_bytes(3, E)
    again = w.zj.batch.index_from_sizes(s.first, s.psize, dev(w, flat))
    assert host(again)[:len(want)] == want
    T = sizes
    requests = [(2, T[2] - 300, 300), (1, 0, MAXU), (0, T[0] - 1, 1), (2, 0, 257), (1, 256 * 100 + 5, 256 * 3), (0, 0, MAXU), (2, 255, 2)]
    check(w, s, requests)


def test_builders_legality_and_codes(world):
    w, zj = world, world.zj
    E = 30
    sizes, contents = [20 + e for e in range(E)], [100 * e for e in range(E)]
    first = [0, 5, 4, 12, 40, 25, 30]
    sizes[27], contents[13], contents[2] = SIZE_MAX + 1, 1 << 40, SIZE_MAX
    got = host(zj.batch.index_from_sizes(dev(w, first), dev(w, sizes), dev(w, contents)))
    want = model_index(first, sizes, contents)
    assert got[:len(want)] == want and want[7:13] == [0, 42, 0, 42, 42, 42]
    # n == 0 and E == 0
    assert host(zj.batch.index_from_sizes(dev(w, [0]), dev(w, []), dev(w, [])))[:3] == [0, 0, 0]
    assert host(zj.batch.index_from_sizes(dev(w, [0, 0, 0]), dev(w, []), dev(w, [])))[:7] == [0, 0, 0, 0, 0, 0, 0]
    # a compress call with an illegal cut list: that buffer owns no entry and carries 42; its neighbours read as ever
    s = store(w, [900, 900, 700], 512, cuts=[[300, 600], [300, 200, 600], [512]], seed=5)
    assert s.h_results[1] == MAXU + 1 - 42 and s.h_first == [0, 3, 3, 5]
    idx = host(s.index)
    assert idx[4:7] == [0, 42, 0]
    s.contents[1] = [900]
    r, out, tot, stats, at = read(w, s, [(0, 100, 700), (1, 0, 10), (2, 500, 100)], [700, 10, 100])
    assert r == [700, -42, 100] and tot == [900, -2, 700] and stats == {"served": 2, "entries": 5, "edges": 4, "errors": 1}
    assert out[at[0]:at[1]] == s.whole[0][100:800] and out[at[1]:at[2]] == bytes([FILL]) * 10 and out[at[2]:at[3]] == s.whole[2][500:600]


# ------------------------------------------------------------------------------------------------ the lane-per-entry grid
def test_emit_boundary(world):
    """requests with 0, 1, 63, 64, 65 and 255, 256, 257 interior entries — the edges of the kernels that take one entry of set A per lane (workgroups of
    ZJ_INDEX_EMIT_WG lanes, waves of 64) — with and without edge entries around them, in one call and alone"""
    w = world
    header = open(os.path.join(ROOT, "zstd-jni_amd", "csrc", "zj_index.h")).read()
    wg = int(re.search(r"#define ZJ_INDEX_EMIT_WG (\d+)u", header).group(1))
    assert wg == 256
    s = store(w, [256 * 300, 256 * 420 - 9, 256 * 305], 256, seed=77)
    counts = (0, 1, 63, 64, 65, wg - 1, wg, wg + 1)
    requests = []
    for k, m in enumerate(counts):
        b = k % 3
        requests.append((b, 256 * (k + 2), 256 * m))                        # no edge
        requests.append((b, 256 * (k + 2) - 7, 256 * m + 7 + 100))          # an edge on either side
        requests.append((b, 256 * (k + 2) - 1, 256 * m + 1))               # an edge in front only
    check(w, s, requests)
    for q in requests[::4]:
        check(w, s, [q])
    r, out, tot, stats, at = read(w, s, [(1, 512, 256 * 256)], [256 * 256])
    assert stats == {"served": 1, "entries": 256, "edges": 0, "errors": 0}


# ------------------------------------------------------------------------------------------------ batching
def test_many_requests_any_order_and_empty_calls(world):
    w, t, zj = world, world.torch, world.zj
    s = store(w, [4096 * 9 + 17, 4096 * 2, 100, 4096 * 30], 4096, seed=13)
    rnd = random.Random(2)
    requests = []
    for _ in range(300):
        b = rnd.randrange(4)
        T = len(s.whole[b])
        requests.append((b, rnd.randrange(T + 2), rnd.choice((1, 50, 4096, 4097, 20000, MAXU))))
    requests += [(3, 0, MAXU)] * 3 + [(0, 5000, 9000), (0, 6000, 9000), (0, 5000, 9000)]
    big = check(w, s, requests)
    # back to back with another R: nothing of the larger call's scratch shows in the smaller one's answers
    check(w, s, requests[:7])
    check(w, s, [(2, 0, MAXU)])
    assert check(w, s, requests)[1] == big[1]
    # R == 0
    e = t.empty(0, dtype=t.int64, device="cuda")
    dst = t.full((64,), FILL, dtype=t.uint8, device="cuda")
    zj.batch.decompress_index_range(s.src, s.off, s.index, s.E, e, dst, t.zeros(1, dtype=t.int64, device="cuda"))
    assert zj.batch.last_index_range() == {"served": 0, "entries": 0, "edges": 0, "errors": 0} and bool((dst == FILL).all())
    # n == 0: every request names a buffer that is not there
    idx0 = zj.batch.index_from_sizes(dev(w, [0]), dev(w, []), dev(w, []))
    res, tot = zj.batch.decompress_index_range(s.src, t.zeros(1, dtype=t.int64, device="cuda"), idx0, 0, dev(w, [0, 0, 5, 1, 0, 5]), dst, dev(w, [0, 8, 16]))
    assert res.cpu().tolist() == [-42, -42] and tot.cpu().tolist() == [-2, -2] and bool((dst == FILL).all())
    # E == 0: buffers without entries hold no byte
    idx1 = zj.batch.index_from_sizes(dev(w, [0, 0, 0]), dev(w, []), dev(w, []))
    res, tot = zj.batch.decompress_index_range(s.src, dev(w, [5, 5, 5]), idx1, 0, dev(w, [0, 0, 5, 1, 3, MAXU]), dst, dev(w, [0, 8, 16]))
    assert res.cpu().tolist() == [0, 0] and tot.cpu().tolist() == [0, 0] and bool((dst == FILL).all())


def test_coarse_index_and_entries_without_content(world):
    """an index of two and three frames an entry; buffers with empty pieces (an empty buffer is one frame of no content) between the others"""
    w, zj = world, world.zj
    s = store(w, [1024 * 11 + 3, 0, 1024 * 4, 0], 1024, seed=31)
    assert [len(c) for c in s.contents] == [12, 1, 4, 1]
    check(w, s, [(1, 0, MAXU), (0, 1000, 5000), (3, 0, 1), (2, 1023, 2050)])
    for group in (2, 3):
        first, sizes, contents, per = [0], [], [], []
        for b in range(4):
            cs = s.contents[b]
            ps = s.h_psize[s.h_first[b]:s.h_first[b] + len(cs)]
            per.append([sum(cs[k:k + group]) for k in range(0, len(cs), group)])
            sizes += [sum(ps[k:k + group]) for k in range(0, len(cs), group)]
            contents += per[-1]
            first.append(len(sizes))
        idx = zj.batch.index_from_sizes(dev(w, first), dev(w, sizes), dev(w, contents))
        requests = [(0, 0, MAXU), (0, 1024 * group, 1024 * group), (0, 1024 * group - 1, 2), (2, 5, 4000), (1, 0, 9), (0, 11000, 5000)]
        slots = [min(lo + ln, len(s.whole[b])) - min(lo, len(s.whole[b])) for b, lo, ln in requests]
        exp = [expect(s, b, lo, ln, slots[i], contents=per) for i, (b, lo, ln) in enumerate(requests)]
        r, out, tot, stats, at = read(w, s, requests, slots, index=idx, entries=len(sizes))
        assert r == [e[0] for e in exp] and stats["entries"] == sum(e[2] for e in exp) and stats["edges"] == sum(e[3] for e in exp)
        image = bytearray(bytes([FILL]) * len(out))
        for i, e in enumerate(exp):
            image[at[i]:at[i] + len(e[1])] = e[1]
        assert out == bytes(image)


def test_entries_outside_the_selection_are_not_read(world):
    """the frames in front of and behind the selection overwritten with 0xFF: the indexed read answers as before, the walked entry refuses the buffer"""
    w, t = world, world.torch
    s = store(w, [512 * 12, 512 * 3], 512, seed=61)
    pre = np.cumsum([0] + s.h_psize).tolist()
    src = s.src.clone()
    src[:pre[3]] = 0xFF                                  # entries 0-2 of buffer 0
    src[pre[8]:pre[12]] = 0xFF                           # entries 8-11 of buffer 0
    requests, slots = [(0, 512 * 3, 512 * 5), (1, 0, MAXU), (0, 512 * 3 + 9, 512 * 4)], [512 * 5, 512 * 3, 512 * 4]
    r, out, tot, stats, at = read(w, s, requests, slots, src=src)
    assert r == slots and tot == [512 * 12, 512 * 3, 512 * 12] and stats == {"served": 3, "entries": 13, "edges": 2, "errors": 0}
    assert out[at[0]:at[1]] == s.whole[0][512 * 3:512 * 8] and out[at[1]:at[2]] == s.whole[1] and out[at[2]:at[3]] == s.whole[0][512 * 3 + 9:512 * 7 + 9]
    dst = t.full((at[-1],), FILL, dtype=t.uint8, device="cuda")
    res, _ = w.zj.batch.decompress_frames_range(src, s.off, dst, t.tensor([0, 512 * 5, 512 * 8], dtype=t.int64, device="cuda"), dev(w, [512 * 3, 512 * 5, 0, MAXU]))
    assert res.cpu().tolist()[0] < 0 and res.cpu().tolist()[1] == 512 * 3
    r, _, _, _, _ = read(w, s, [(0, 512 * 2, 512 * 2)], [1024], src=src)        # a selection that does hold a destroyed frame answers its error
    assert r[0] < 0


# ------------------------------------------------------------------------------------------------ false indexes
def test_false_indexes_answer_their_codes(world):
    """wrong answers, each with the code the header names; the neighbours in the same call read as ever and nothing is written outside the slots.  Every index
    here is one for which the header promises in-bounds access."""
    w, zj = world, world.zj
    s = store(w, [512 * 6, 512 * 20 + 9, 512 * 5], 512, seed=41)
    flat = [c for cs in s.contents for c in cs]
    T = [len(x) for x in s.whole]
    requests = [(0, 10, 2000), (1, 0, MAXU), (2, 0, MAXU), (1, 700, 3000), (0, 0, MAXU)]
    k = s.h_first[1] + 7                                 # an interior entry of both requests for buffer 1
    cases = []
    sizes = list(s.h_psize); sizes[k] += 1
    cases.append(("sizes do not sum to the extent", s.h_first, sizes, flat, -72, -2, 0))
    first = list(s.h_first); first[2] = first[1] - 1      # buffer 1 descends; buffer 2 then begins one entry early, so its sizes miss its extent
    cases.append(("first does not ascend", first, s.h_psize, flat, -42, -2, None))
    contents = list(flat); contents[k] += 1
    cases.append(("a content size one above the truth", s.h_first, s.h_psize, contents, -20, T[1] + 1, 1))
    sizes = list(s.h_psize); sizes[k] = SIZE_MAX + 1
    cases.append(("a size above 2^32 - 1", s.h_first, sizes, flat, -42, -2, 0))
    for name, first, sizes, contents, code, total, delta in cases:
        idx = zj.batch.index_from_sizes(dev(w, first), dev(w, sizes), dev(w, contents))
        slots = [2000, T[1] + 1, T[2], 3000, T[0]]
        r, out, tot, stats, at = read(w, s, requests, slots, index=idx)
        if name == "first does not ascend":               # 42 for that buffer only: its neighbours are not marked
            assert host(idx)[4:7] == [0, 42, 0] and r == [2000, -42, -72, -42, T[0]] and tot == [T[0], -2, -2, -2, T[0]], (name, r, tot)
            assert out[at[0]:at[0] + 2000] == s.whole[0][10:2010] and out[at[4]:at[4] + T[0]] == s.whole[0] and out[at[1]:at[4]] == bytes([FILL]) * (at[4] - at[1])
            continue
        assert r == [2000, code, T[2], code, T[0]] and tot == [T[0], total, T[2], total, T[0]], (name, r, tot)
        image = bytearray(out)                            # (the first hi' - lo' bytes of a slot that answered an entry's error are unspecified)
        for i in (1, 3):
            want = min(slots[i], (T[1] + 1 if i == 1 else 3000)) if code == -20 else 0
            image[at[i]:at[i] + want] = bytes([FILL]) * want
        model = bytearray(bytes([FILL]) * len(out))
        model[at[0]:at[0] + 2000] = s.whole[0][10:2010]
        model[at[2]:at[2] + T[2]] = s.whole[2]
        model[at[4]:at[4] + T[0]] = s.whole[0]
        assert bytes(image) == bytes(model), name
        assert stats["errors"] == 2 and stats["served"] == 3, name


def test_descending_sums_mark_the_request_and_spare_its_neighbours(world):
    """an interior C[k] raised above C[k + 1]: the request answers 20 with none of its entries written, and the requests in front of it — one with slack behind its
    range, one of an empty range — keep every byte of theirs 0xCD: the marked request's gathered run lies in its own entries, never in a neighbour's closing entry"""
    w, zj = world, world.zj
    s = store(w, [512 * 6, 512 * 20 + 9, 512 * 5], 512, seed=41)
    T = [len(x) for x in s.whole]
    words = host(s.index)
    k = 2 * 3 + 1 + s.h_first[1] + 7
    words[k] = words[k + 1] + 5
    idx = dev(w, words)
    requests = [(0, 10, 2000), (2, T[2], 5), (1, 0, MAXU), (2, 0, MAXU), (1, 512 * 3, 512 * 9), (0, 0, MAXU)]
    slots = [2011, 16, T[1], T[2] + 3, 512 * 9, T[0]]
    r, out, tot, stats, at = read(w, s, requests, slots, index=idx)
    assert r == [2000, 0, -20, T[2], -20, T[0]] and tot == [T[0], T[2], T[1], T[2], T[1], T[0]]
    model = bytearray(bytes([FILL]) * len(out))
    model[at[0]:at[0] + 2000] = s.whole[0][10:2010]
    model[at[3]:at[3] + T[2]] = s.whole[2]
    model[at[5]:at[5] + T[0]] = s.whole[0]
    assert out == bytes(model)
    assert stats["served"] == 4 and stats["errors"] == 2


# ------------------------------------------------------------------------------------------------ the host form
def test_host_form_against_the_walked_host_form(world):
    w, zj = world, world.zj
    L = zj.lib()
    for dictionary in (False, True):
        s = store(w, [2048 * 25 + 100], 2048, dictionary=dictionary, seed=51)
        data = s.src.cpu().numpy().tobytes()
        T = len(s.whole[0])
        dd = s.ddict._ptr if dictionary else None
        rnd = random.Random(4)
        for lo, ln in boundary_ranges(s.contents[0], T, 25, rnd):
            cap = min(ln, T + 5)
            dst = C.create_string_buffer(bytes([FILL]) * (cap + 16), cap + 16)
            total = C.c_ulonglong(0)
            want_r = L.zjni_decompress_frames_range_usingDDict(dst, cap, data, len(data), lo, ln, C.byref(total), dd)
            want = (want_r, total.value, dst.raw)
            got, tot = zj.decompress_index_range(data, lo, ln, s.h_psize, s.contents[0], dictionary=s.ddict, capacity=cap)
            assert (len(got), tot) == (want_r, T) and total.value == T, (lo, ln)
            assert got == s.whole[0][min(lo, T):min(lo + ln, T)] == want[2][:want_r]
        stats = zj.batch.last_index_range()
        assert stats["errors"] == 0
        # a slot too small, sizes that do not sum to the buffer, an oversized entry
        sizes = (C.c_uint64 * s.E)(*s.h_psize)
        contents = (C.c_uint64 * s.E)(*s.contents[0])
        dst = C.create_string_buffer(64)
        code = lambda r: L.zjni_getErrorCode(r) if L.zjni_isError(r) else 0      # noqa: E731
        assert code(L.zjni_decompress_index_range(dst, 10, data, len(data), 0, 11, sizes, contents, s.E, None, dd)) == 70
        assert code(L.zjni_decompress_index_range(dst, 10, data, len(data) - 1, 0, 10, sizes, contents, s.E, None, dd)) == 72
        sizes[3] = SIZE_MAX + 1
        assert code(L.zjni_decompress_index_range(dst, 10, data, len(data), 0, 10, sizes, contents, s.E, None, dd)) == 42
