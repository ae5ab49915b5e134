"""GPU (-m gpu): the blocking forms for one host buffer, alternating over the one staging slot.  In one process and on one thread zjni_compress_chunked,
zjni_compress_pieces, zjni_decompress_frames, zjni_decompress_frames_range and zjni_decompress_index_range are called in turn on sources of 1 KiB, then 300 KiB,
then 1 KiB again, so the slot they share grows once and is then reused larger than needed.  Every answer — result, bytes, piece sizes, total — must be the one
the corresponding *_batch_device entry gives for the same bytes, and each zjni_last_* getter must show the counts the calls imply."""
import ctypes as C

import numpy as np
import pytest

from util import json_records

pytestmark = pytest.mark.gpu

CHUNK = 4096
FILL = 0xCD
SIZES = (1 << 10, 300 << 10, 1 << 10)


def signed(r):
    return r - (1 << 64) if r >= (1 << 63) else r


def dev_bytes(t, data):
    return t.frombuffer(bytearray(data), dtype=t.uint8).cuda() if data else t.empty(0, dtype=t.uint8, device="cuda")


def one(t, size):
    return t.tensor([0, size], dtype=t.int64, device="cuda")


def pieces_both(zj, t, data, chunk, cuts):
    """zjni_compress_pieces with the cut list and a piece-size array against its device entry -> (the frames, or None for a refused list; the pieces)"""
    L, size, cap_p = zj.lib(), len(data), len(cuts) + 1
    dst_blob, dst_off, res, first, psize = zj.batch.compress_pieces(dev_bytes(t, data), one(t, size), level=3, chunk=chunk, cuts=t.tensor(cuts, dtype=t.int64, device="cuda"),
                                                                    cut_off=one(t, len(cuts)), sizes=True, piece_cap=cap_p)
    want, want_n, want_sizes = int(res.item()), int(first[1].item()), psize.cpu().tolist()
    cap = int(dst_off[1].item())
    assert cap == zj.batch.compress_bound_pieces(size, cap_p)
    dst = C.create_string_buffer(bytes([FILL]) * (cap + 16), cap + 16)
    hcut, hsize, hn = (C.c_uint64 * len(cuts))(*cuts), (C.c_uint64 * cap_p)(*([FILL] * cap_p)), C.c_size_t(99)
    r = signed(L.zjni_compress_pieces(dst, cap, data, size, 3, 0, chunk, hcut, len(cuts), None, hsize, cap_p, C.byref(hn)))
    assert (r, hn.value) == (want, want_n)
    if r < 0:
        assert dst.raw == bytes([FILL]) * (cap + 16) and list(hsize) == [FILL] * cap_p
        return None, 0
    assert dst.raw[:r] == dst_blob[:r].cpu().numpy().tobytes() and dst.raw[r:] == bytes([FILL]) * (cap + 16 - r)
    assert list(hsize)[:want_n] == want_sizes and sum(want_sizes) == r and list(hsize)[want_n:] == [FILL] * (cap_p - want_n)
    return dst.raw[:r], want_n


def test_host_forms_alternate_over_one_slot(zj):
    import torch as t
    zj.batch.init(0)
    L, B = zj.lib(), zj.batch
    text = b",".join(json_records(4000, seed=21))
    text = text * (max(SIZES) // len(text) + 1)
    for step, size in enumerate(SIZES):
        data = text[step * 777:step * 777 + size]
        src, off = dev_bytes(t, data), one(t, size)

        # chunked compress: ceil(size / CHUNK) frames
        frames_n = -(-size // CHUNK)
        d_blob, d_off, d_res = B.compress_chunked(src, off, level=3, chunk=CHUNK)
        cap = int(d_off[1].item())
        dst = C.create_string_buffer(bytes([FILL]) * (cap + 16), cap + 16)
        r = signed(L.zjni_compress_chunked(dst, cap, data, size, 3, 0, CHUNK))
        assert r == int(d_res.item()) and r > 0
        frames = dst.raw[:r]
        assert frames == d_blob[:r].cpu().numpy().tobytes() and dst.raw[r:] == bytes([FILL]) * (cap + 16 - r)

        # pieces with a two-cut list and a piece-size array: at CHUNK (a list the 300 KiB source cannot have: three pieces, each above CHUNK) and at the largest chunk
        cuts = [size // 3, 2 * size // 3]
        legal = max(cuts[0], cuts[1] - cuts[0], size - cuts[1]) <= CHUNK
        got, count = pieces_both(zj, t, data, CHUNK, cuts)
        assert (got is not None) == legal and count == (3 if legal else 0)
        got, count = pieces_both(zj, t, data, zj.BLOCKSIZE_MAX, cuts)
        assert got is not None and count == 3

        # whole decompress of the chunked frames
        fsrc, foff = dev_bytes(t, frames), one(t, len(frames))
        out = t.full((size + 16,), FILL, dtype=t.uint8, device="cuda")
        d_res = B.decompress_frames(fsrc, foff, out, one(t, size))
        dst = C.create_string_buffer(bytes([FILL]) * (size + 16), size + 16)
        r = signed(L.zjni_decompress_frames(dst, size, frames, len(frames)))
        assert r == int(d_res.item()) == size
        assert dst.raw == out.cpu().numpy().tobytes() == data + bytes([FILL]) * 16
        assert B.last_frames() == {"split": int(frames_n > 1), "entries": frames_n, "unsplit": int(frames_n == 1), "redo": 0}

        # a range that cuts its first and its last frame
        lo, ln = size // 10 + 1, size // 2
        first, last = lo // CHUNK, (lo + ln - 1) // CHUNK
        e_first, e_last = lo % CHUNK != 0, min((last + 1) * CHUNK, size) > lo + ln
        touched, edges = last - first + 1, int(e_first or e_last) if first == last else int(e_first) + int(e_last)
        assert edges == (1 if frames_n == 1 else 2)
        out = t.full((ln + 16,), FILL, dtype=t.uint8, device="cuda")
        rng = t.tensor([lo, ln], dtype=t.int64, device="cuda")
        d_res, d_tot = B.decompress_frames_range(fsrc, foff, out, one(t, ln), rng)
        dst = C.create_string_buffer(bytes([FILL]) * (ln + 16), ln + 16)
        total = C.c_ulonglong(0)
        r = signed(L.zjni_decompress_frames_range(dst, ln, frames, len(frames), lo, ln, C.byref(total)))
        assert r == int(d_res.item()) == ln and total.value == int(d_tot.item()) == size
        assert dst.raw == out.cpu().numpy().tobytes() == data[lo:lo + ln] + bytes([FILL]) * 16
        assert B.last_frames_range() == {"served": 1, "frames": touched, "edges": edges, "errors": 0}

        # the same range by an index: the host form takes the two arrays, the device entry the index prepared from them
        sizes, contents = zj.index_from_frames(frames)
        assert len(sizes) == frames_n and sum(sizes) == len(frames) and sum(contents) == size
        index = B.index_from_sizes(one(t, frames_n), t.tensor(sizes, dtype=t.int64, device="cuda"), t.tensor(contents, dtype=t.int64, device="cuda"))
        out = t.full((ln + 16,), FILL, dtype=t.uint8, device="cuda")
        d_res, d_tot = B.decompress_index_range(fsrc, foff, index, frames_n, t.tensor([0, lo, ln], dtype=t.int64, device="cuda"), out, one(t, ln))
        assert B.last_index_range() == {"served": 1, "entries": touched, "edges": edges, "errors": 0}
        dst = C.create_string_buffer(bytes([FILL]) * (ln + 16), ln + 16)
        total = C.c_ulonglong(0)
        hs, hc = (C.c_uint64 * frames_n)(*sizes), (C.c_uint64 * frames_n)(*contents)
        r = signed(L.zjni_decompress_index_range(dst, ln, frames, len(frames), lo, ln, hs, hc, frames_n, C.byref(total), None))
        assert r == int(d_res.item()) == ln and total.value == int(d_tot.item()) == size
        assert dst.raw == out.cpu().numpy().tobytes() == data[lo:lo + ln] + bytes([FILL]) * 16
        assert B.last_index_range() == {"served": 1, "entries": touched, "edges": edges, "errors": 0}
