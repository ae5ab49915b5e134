#!/usr/bin/env python3
"""Large buffers as many frames, measured: the benchmark's mixed-entropy data held as a few large buffers.

  C   zjni_compress_chunked_batch_device      n buffers -> ceil(size / chunk) frames each, laid end to end
  B   zjni_decompress_frames_batch_device     the packed output of C, one entry per frame
  A   zjni_decompress_batch_device            the same buffers through the existing entry (unchanged code: one wave per buffer, frame after frame)
  c0  zjni_compress_batch_device2             the same bytes as E separate buffers of `chunk` bytes   (the ceiling of C)
  d0  zjni_decompress_batch_device            the same frames as E separate entries                   (the ceiling of B)

All in one process, after a warm-up of each, every call between two device events and a synchronise (the new entries wait once on the host for their entry
count: inside the window).  A, B and d0 alternate; A takes seconds per call, so it gets fewer calls (--existing-steps).  The outputs are compared: C's frames with
c0's byte for byte (they are packed to the same blob), B's and A's results and decoded bytes with the source.  No torch: HBM through the HIP runtime, so the same
command runs under `rocprofv3 --kernel-trace --stats` for the times of the new kernels (--existing-steps 0 keeps the seconds-long calls out of the trace).

usage: bench_frames.py [--buffers 64] [--buffer-bytes 67108864] [--chunk 65536] [--level 3] [--steps 12] [--existing-steps 3] [--warmup 2] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=64)
    ap.add_argument("--buffer-bytes", type=int, default=64 << 20)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--existing-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def chk(r):
        assert r == 0, r

    def dmalloc(nbytes):
        p = vp()
        chk(hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 8))))
        return p

    def upload(arr):
        p = dmalloc(arr.nbytes)
        chk(hip.hipMemcpy(p, arr.ctypes.data_as(vp), C.c_size_t(arr.nbytes), 1))
        return p

    def download(p, nbytes, dtype=np.uint8, at=0):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        chk(hip.hipMemcpy(out.ctypes.data_as(vp), vp(p.value + at), C.c_size_t(nbytes), 2))
        return out

    assert L.zjni_init(0) == 0, "needs a GPU"
    n, size, chunk, level = a.buffers, a.buffer_bytes, a.chunk, a.level
    assert size % chunk == 0, "the ceiling legs want whole chunks"
    per = size // chunk
    E = n * per
    total = n * size
    slot = L.zjni_compressBound_chunked(size, chunk)
    assert slot == per * L.zjni_compressBound(chunk)
    src, comp, packed, packed0 = dmalloc(total), dmalloc(n * slot), dmalloc(n * slot), dmalloc(n * slot)
    back_a, back_b, back_0 = dmalloc(total), dmalloc(total), dmalloc(total)
    soff, coff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot)
    soff_e, coff_e = upload(np.arange(E + 1, dtype=np.uint64) * chunk), upload(np.arange(E + 1, dtype=np.uint64) * L.zjni_compressBound(chunk))
    res_c, res_a, res_b, poff = dmalloc(n * 8), dmalloc(n * 8), dmalloc(n * 8), dmalloc((n + 1) * 8)
    res_c0, res_d0, poff_e = dmalloc(E * 8), dmalloc(E * 8), dmalloc((E + 1) * 8)
    chk(L.zjni_synth_fill_device(src, chunk, 0, E, None))
    ev = [vp(), vp()]
    for e in ev:
        chk(hip.hipEventCreate(C.byref(e)))

    def timed(call):
        chk(hip.hipEventRecord(ev[0], None))
        chk(call())
        chk(hip.hipEventRecord(ev[1], None))
        chk(hip.hipDeviceSynchronize())
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value

    def call_c():
        return L.zjni_compress_chunked_batch_device(src, soff, comp, coff, res_c, n, level, 0, chunk, None)

    def call_c0():
        return L.zjni_compress_batch_device2(src, soff_e, comp, coff_e, res_c0, E, level, 0, None)

    def call_a():
        return L.zjni_decompress_batch_device(packed, poff, back_a, soff, res_a, n, None)

    def call_b():
        return L.zjni_decompress_frames_batch_device(packed, poff, back_b, soff, res_b, n, None, None)

    def call_d0():
        return L.zjni_decompress_batch_device(packed0, poff_e, back_0, soff_e, res_d0, E, None)

    # ---- compress: the separate buffers first (their packed frames are what the chunked frames must be), then the chunked entry, alternating
    for _ in range(a.warmup):
        timed(call_c0)
    chk(L.zjni_pack_batch_device2(comp, coff_e, res_c0, packed0, poff_e, E, None))
    chk(hip.hipDeviceSynchronize())
    frames_bytes = int(download(poff_e, (E + 1) * 8, np.uint64)[-1])
    for _ in range(a.warmup):
        timed(call_c)
    tc, tc0 = [], []
    for _ in range(a.steps):
        tc0.append(timed(call_c0))
        tc.append(timed(call_c))
    chk(L.zjni_pack_batch_device2(comp, coff, res_c, packed, poff, n, None))
    chk(hip.hipDeviceSynchronize())
    rc = download(res_c, n * 8, np.uint64)
    assert (rc < (1 << 40)).all() and int(rc.sum()) == frames_bytes == int(download(poff, (n + 1) * 8, np.uint64)[-1]), "chunked sizes differ from the separate frames'"
    piece = 256 << 20
    for at in range(0, frames_bytes, piece):
        m = min(piece, frames_bytes - at)
        assert (download(packed, m, at=at) == download(packed0, m, at=at)).all(), "chunked frames differ from the separate frames at %d" % at

    # ---- decompress: the existing entry on the concatenated buffers (A), the new entry (B), the separate frames (d0)
    for _ in range(a.warmup):
        timed(call_b)
        timed(call_d0)
    stats4 = (C.c_uint * 4)()
    chk(L.zjni_last_frames(stats4))
    ta, tb, td0 = [], [], []
    for k in range(a.steps):
        if k < a.existing_steps:
            ta.append(timed(call_a))
        tb.append(timed(call_b))
        td0.append(timed(call_d0))
    rb = download(res_b, n * 8, np.uint64)
    assert (rb == size).all(), "a buffer did not decode through the new entry"
    if ta:
        assert (download(res_a, n * 8, np.uint64) == size).all(), "a buffer did not decode through the existing entry"
    assert (download(res_d0, E * 8, np.uint64) == chunk).all()
    for at in range(0, total, piece):
        m = min(piece, total - at)
        want = download(src, m, at=at)
        assert (download(back_b, m, at=at) == want).all(), "decoded bytes (new entry) differ at %d" % at
        assert (download(back_0, m, at=at) == want).all(), "decoded bytes (separate frames) differ at %d" % at
        if ta:
            assert (download(back_a, m, at=at) == want).all(), "decoded bytes (existing entry) differ at %d" % at

    gib = total / (1 << 30)

    def stats(ts):
        if not ts:
            return None
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        med = statistics.median(ts)
        return {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "calls": len(ts),
                "GiBps_of_source_at_median": round(gib / (med / 1e3), 2)}

    sa, sb = stats(ta), stats(tb)
    line = {"buffers": n, "buffer_bytes": size, "chunk": chunk, "entries": E, "level": level, "source_GiB": round(gib, 3), "frames_bytes": frames_bytes,
            "C_compress_chunked": stats(tc), "c0_compress_separate_buffers": stats(tc0),
            "B_decompress_frames": sb, "A_decompress_existing_entry_same_buffers": sa, "d0_decompress_separate_frames": stats(td0),
            "B_faster_than_A": round(sa["median_ms"] / sb["median_ms"], 1) if sa else None,
            "required": "B at least 2 x faster than A", "met": bool(sa["median_ms"] >= 2 * sb["median_ms"]) if sa else None,
            "last_frames": {"split": stats4[0], "entries": stats4[1], "unsplit": stats4[2], "redo": stats4[3]},
            "outputs_compared": "C's packed frames with c0's byte for byte; results and all decoded bytes of A, B and d0 against the source",
            "build_stamp": zj.build_stamp()}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
