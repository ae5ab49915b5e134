"""GPU (-m gpu): the range-read index built from the frames alone (zjni_index_count_frames_device, zjni_index_from_frames_device, zjni_index_from_frames).
The walk-built index against zjni_index_from_pieces_device's word for word — plain, with a dictionary, with a checksum, n across the edges of the 64-lane
workgroup, 0 .. 1100 frames a buffer — the buffers of tests/inspect_cases.py read by the indexed entry over the walk-built index against
zjni_decompress_frames_range_batch_device (results, totals, the whole 0xCD-filled destination), the compact form fed back to zjni_index_from_sizes_device, a false
d_piece_first with guard words around every array, empty calls, and the host form.  Stores are made by batch.compress_pieces at chunk 256 .. 4096, as in
tests/test_gpu_index.py, whose helpers these tests use.  The CPU twin of the arithmetic is tests/test_emu_index_walk.py."""
import ctypes as C
import random

import numpy as np
import pytest

import inspect_cases as ic
import test_gpu_index as gi
from test_gpu_index import dev, host, store, FILL, MAXU, SIZE_MAX

pytestmark = pytest.mark.gpu
world = gi.world
GUARD = 0x7EEDFACECAFEBEEF
PAD = 4


def words_of(n, E):
    return 2 * n + 1 + 2 * (E + 1)


# ------------------------------------------------------------------------------------------------ 1. builders agree
@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("variant", ["plain", "dictionary", "checksum"])
def test_walk_built_index_equals_the_one_from_pieces(world, variant, n):
    """frame counts 1, 2, 3, 65 and 1100 a buffer (E above the scan workgroup's 1024 lanes: a share above 1), then buffers of 0 frames laid between them.
    Every legal buffer of a compress call owns at least one entry, so the layout with empty buffers is compared with zjni_index_from_sizes_device, the builder
    zjni_index_from_pieces_device ends in, on the same sizes with repeated entries in first[]."""
    w, zj = world, world.zj
    chunk = {"plain": 256, "dictionary": 512, "checksum": 256}[variant]
    counts = [1100 if i == n // 2 else (1, 2, 65, 3)[i % 4] for i in range(n)]
    sizes = [chunk * c - (i % 5) for i, c in enumerate(counts)]
    s = store(w, sizes, chunk, checksum=variant == "checksum", dictionary=variant == "dictionary", seed=n)
    assert s.h_first == np.cumsum([0] + counts).tolist() and s.E > 1024 and all(r < 1 << 40 for r in s.h_results)
    index, E, first = zj.batch.index_from_frames(s.src, s.off)
    assert E == s.E and host(first) == s.h_first
    got, want = host(index), host(s.index)
    assert len(got) == len(want) and got[:words_of(n, E)] == want[:words_of(n, E)]
    # buffers of no frame: in front, in the middle (twice running), at the end
    h_off = host(s.off)
    at = sorted({0, n // 2, n})
    off2, first2 = [], []
    for i in range(n + 1):
        rep = 1 + (2 if i == n // 2 and i in at else 1 if i in at else 0)
        off2 += [h_off[i]] * rep
        first2 += [s.h_first[i]] * rep
    n2 = len(off2) - 1
    assert n2 > n
    index2, E2, first_t = zj.batch.index_from_frames(s.src, dev(w, off2))
    flat = [c for cs in s.contents for c in cs]
    want2 = host(zj.batch.index_from_sizes(dev(w, first2), s.psize, dev(w, flat)))
    assert E2 == s.E and host(first_t) == first2 and host(index2)[:words_of(n2, E)] == want2[:words_of(n2, E)]
    assert want2[n2 + 1:2 * n2 + 1] == [0] * n2


# ------------------------------------------------------------------------------------------------ 2. the corpus on the device
def test_corpus_reads_equal_the_walked_entry(world):
    """every buffer of tests/inspect_cases.py, indexable or not, a request each: the indexed entry over the walk-built index against the walked entry.  A buffer
    with a frame that records more than 2^32 - 1 bytes answers 14 by the index (its entry format) whatever the walked entry says: the one documented difference."""
    w, t, zj = world, world.torch, world.zj
    cases, _ = ic.build_cases(w.ref)
    n = len(cases)
    assert n > 3000
    blob = b"\xAA" * 5 + b"".join(c.data for c in cases) + b"\0" * 8
    src = t.frombuffer(bytearray(blob), dtype=t.uint8).cuda()
    h_off = np.cumsum([5] + [len(c.data) for c in cases]).tolist()
    off = dev(w, h_off)
    index, E, first = zj.batch.index_from_frames(src, off, sizes=False)
    idx = host(index)
    valid, h_first = idx[n + 1:2 * n + 1], idx[:n + 1]
    U = idx[2 * n + 2 + E:2 * n + 3 + 2 * E]
    T = [U[h_first[i + 1]] - U[h_first[i]] for i in range(n)]
    oversize = []
    for i, c in enumerate(cases):                               # the host form says the same of every buffer
        r = zj.lib().zjni_index_from_frames(c.data, len(c.data), None, None, 0, C.byref(C.c_size_t(0)))
        code = (1 << 64) - r if r > MAXU - 120 else 0
        assert (code if code != 70 else 0) == valid[i], c.name
        if valid[i] == 14 and c.name in ("declares_2_60", "declares_error"):
            oversize.append(i)
    assert len(oversize) == 2 and sum(v == 0 for v in valid) > 500 and sum(v != 0 for v in valid) > 500 and E > sum(v == 0 for v in valid)
    for rnd in range(2):
        ranges = [(0, min(T[i], 1 << 15)) if rnd == 0 else (T[i] // 2 - min(T[i] // 2, 7), 3001) for i in range(n)]
        slots = [min(max(T[i] - lo, 0), ln) + (i % 3) for i, (lo, ln) in enumerate(ranges)]
        at = np.cumsum([3] + slots).tolist()
        dst_off = dev(w, at)
        dst_x = t.full((at[-1] + 64,), FILL, dtype=t.uint8, device="cuda")
        dst_w = t.full((at[-1] + 64,), FILL, dtype=t.uint8, device="cuda")
        req = dev(w, [v for i, (lo, ln) in enumerate(ranges) for v in (i, lo, ln)])
        res_x, tot_x = zj.batch.decompress_index_range(src, off, index, E, req, dst_x, dst_off, dictionary=w.ddict)
        stats = zj.batch.last_index_range()
        res_w, tot_w = zj.batch.decompress_frames_range(src, off, dst_w, dst_off, dev(w, [v for r in ranges for v in r]), dictionary=w.ddict)
        rx, tx, rw, tw = res_x.cpu().tolist(), tot_x.cpu().tolist(), res_w.cpu().tolist(), tot_w.cpu().tolist()
        for i in oversize:
            assert (rx[i], tx[i]) == (-14, -2)
            rw[i], tw[i] = -14, -2
        assert rx == rw and tx == tw, rnd
        assert dst_x.cpu().numpy().tobytes() == dst_w.cpu().numpy().tobytes(), rnd
        assert stats["served"] + stats["errors"] == n and stats["served"] > 300


# ------------------------------------------------------------------------------------------------ 3. the compact form
def test_compact_form_rebuilds_the_index(world):
    w, zj = world, world.zj
    s = store(w, [1024 * 11 + 3, 0, 1024 * 4, 0, 700], 1024, seed=31)
    index, E, first, psize, pcontent = zj.batch.index_from_frames(s.src, s.off, sizes=True)
    assert E == s.E == 19 and host(psize) == s.h_psize and host(pcontent) == [c for cs in s.contents for c in cs]
    again = zj.batch.index_from_sizes(first, psize, pcontent)
    assert host(again)[:words_of(5, E)] == host(index)[:words_of(5, E)] == host(s.index)[:words_of(5, E)]
    gi.check(w, s, [(0, 1000, 5000), (2, 1023, 2050), (4, 0, MAXU), (1, 0, 5)], index=again)


# ------------------------------------------------------------------------------------------------ 4. a false first array
def test_false_first_marks_its_buffer_alone(world):
    """the second walk trusts nothing of the first: d_piece_first too small, too large, descending, past E — 42 for that buffer alone, its entries 0, the others'
    words exact, and the guard words around the index and both arrays unchanged"""
    w, t, zj = world, world.torch, world.zj
    L = zj.lib()
    s = store(w, [512 * 40, 512 * 2 - 9, 512 * 3], 512, seed=9)
    assert s.h_first == [0, 40, 42, 45]
    per = [(s.h_psize[s.h_first[b]:s.h_first[b + 1]], s.contents[b]) for b in range(3)]
    cases = {"honest": ([0, 40, 42, 45], 45, [0, 0, 0]), "too small": ([0, 40, 41, 44], 44, [0, 42, 0]), "too large": ([0, 40, 50, 53], 60, [0, 42, 0]),
             "descending": ([50, 90, 0, 3], 90, [0, 42, 0]), "past E": ([0, 40, 42, 45], 44, [0, 0, 42]), "the first too small": ([0, 39, 41, 44], 44, [42, 0, 0])}
    for name, (first, E, verdicts) in cases.items():
        words = words_of(3, E)
        idx = dev(w, [GUARD] * (words + 2 * PAD))
        size, content, d_first = dev(w, [GUARD] * (E + 2 * PAD)), dev(w, [GUARD] * (E + 2 * PAD)), dev(w, first)
        r = L.zjni_index_from_frames_device(s.src.data_ptr(), s.off.data_ptr(), 3, d_first.data_ptr(), E, idx.data_ptr() + 8 * PAD, size.data_ptr() + 8 * PAD,
                                            content.data_ptr() + 8 * PAD, t.cuda.current_stream().cuda_stream)
        assert r == 0, name
        t.cuda.synchronize()
        h_idx, h_size, h_content = host(idx), host(size), host(content)
        for a, used in ((h_idx, words), (h_size, E), (h_content, E)):
            assert a[:PAD] == [GUARD] * PAD and a[PAD + used:] == [GUARD] * PAD, name
        want_size, want_content = [0] * E, [0] * E
        for b in range(3):
            if verdicts[b] == 0:
                want_size[first[b]:first[b + 1]], want_content[first[b]:first[b + 1]] = per[b]
        got = h_idx[PAD:PAD + words]
        assert got[:4] == first and got[4:7] == verdicts, name
        assert h_size[PAD:PAD + E] == want_size and h_content[PAD:PAD + E] == want_content, name
        assert got[7:8 + E] == np.cumsum([0] + want_size).tolist() and got[8 + E:] == np.cumsum([0] + want_content).tolist(), name
    # the index of the last case reads: the marked buffer answers 42, the others as ever
    first, E, _ = cases["too small"]
    index, d_first = dev(w, [0] * (zj.batch.index_bytes(3, E) // 8)), dev(w, first)
    assert L.zjni_index_from_frames_device(s.src.data_ptr(), s.off.data_ptr(), 3, d_first.data_ptr(), E, index.data_ptr(), None, None, t.cuda.current_stream().cuda_stream) == 0
    r, out, tot, stats, at = gi.read(w, s, [(0, 100, 700), (1, 0, 10), (2, 500, 100)], [700, 10, 100], index=index, entries=E)
    assert r == [700, -42, 100] and tot == [512 * 40, -2, 512 * 3]
    assert out[at[0]:at[1]] == s.whole[0][100:800] and out[at[1]:at[2]] == bytes([FILL]) * 10 and out[at[2]:at[3]] == s.whole[2][500:600]


# ------------------------------------------------------------------------------------------------ 5. empty calls
def test_empty_calls(world):
    w, t, zj = world, world.torch, world.zj
    src = t.zeros(16, dtype=t.uint8, device="cuda")
    index, E, first = zj.batch.index_from_frames(src, dev(w, [0]))                   # n == 0
    assert E == 0 and host(first) == [0] and host(index)[:3] == [0, 0, 0]
    index, E, first, psize, pcontent = zj.batch.index_from_frames(src, dev(w, [5, 5, 5, 5]), sizes=True)      # E == 0: buffers of no byte
    assert E == 0 and host(first) == [0, 0, 0, 0] and host(index)[:9] == [0] * 9 and psize.numel() == 0 and pcontent.numel() == 0
    dst = t.full((64,), FILL, dtype=t.uint8, device="cuda")
    res, tot = zj.batch.decompress_index_range(src, dev(w, [5, 5, 5, 5]), index, 0, dev(w, [0, 0, 5, 2, 3, MAXU]), dst, dev(w, [0, 8, 16]))
    assert res.cpu().tolist() == [0, 0] and tot.cpu().tolist() == [0, 0] and bool((dst == FILL).all())
    # n or E above 2^32 - 1: 72, before anything is touched
    L = zj.lib()
    for r in (L.zjni_index_count_frames_device(src.data_ptr(), first.data_ptr(), 1 << 32, first.data_ptr(), None),
              L.zjni_index_from_frames_device(src.data_ptr(), first.data_ptr(), 1, first.data_ptr(), 1 << 32, index.data_ptr(), None, None, None)):
        assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 72


# ------------------------------------------------------------------------------------------------ 6. the host form
def test_host_form_then_the_indexed_host_read(world):
    w, zj = world, world.zj
    L = zj.lib()
    s = store(w, [2048 * 25 + 100], 2048, seed=51)
    data = s.src.cpu().numpy().tobytes()
    T = len(s.whole[0])
    sizes, contents = zj.index_from_frames(data)
    assert sizes == s.h_psize and contents == s.contents[0]
    n = C.c_size_t(0)
    r = L.zjni_index_from_frames(data, len(data), None, None, 0, C.byref(n))
    assert L.zjni_getErrorCode(r) == 70 and n.value == 26
    rnd = random.Random(4)
    for lo, ln in gi.boundary_ranges(contents, T, 25, rnd):
        cap = min(ln, T + 5)
        dst = C.create_string_buffer(bytes([FILL]) * (cap + 16), cap + 16)
        total = C.c_ulonglong(0)
        want_r = L.zjni_decompress_frames_range(dst, cap, data, len(data), lo, ln, C.byref(total))
        got, tot = zj.decompress_index_range(data, lo, ln, sizes, contents, capacity=cap)
        assert (len(got), tot) == (want_r, T) and total.value == T, (lo, ln)
        assert got == s.whole[0][min(lo, T):min(lo + ln, T)] == dst.raw[:want_r]
    with pytest.raises(zj.ZstdException) as e:
        zj.index_from_frames(data[:-3])
    assert e.value.getErrorCode() == 72
    assert SIZE_MAX == (1 << 32) - 1
