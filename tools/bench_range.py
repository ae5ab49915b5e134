#!/usr/bin/env python3
"""Ranged decompress, measured: the benchmark's mixed-entropy data held as a few large buffers of many frames (zjni_compress_chunked_batch_device's output).

  B       zjni_decompress_frames_batch_device          every buffer whole (existing code: what a ranged reader pays today, before slicing)
  R_full  zjni_decompress_frames_range_batch_device    the range [0, T) of every buffer
  R_1/64  the same entry                               `--range-bytes` (1 MiB) from the middle of every buffer, beginning and ending inside frames
  R_tail  the same entry                               the last `--range-bytes` of every buffer

One process, a warm-up of each leg, then the legs alternating; every call between two device events and a synchronise (the entries wait once on the host for
their entry counts: inside the window).  All outputs are compared with the source.  No torch: HBM through the HIP runtime, so the same command runs under
`rocprofv3 --kernel-trace --stats` for the times of the kernels.

usage: bench_range.py [--buffers 64] [--buffer-bytes 67108864] [--chunk 65536] [--level 3] [--range-bytes 1048576] [--steps 12] [--warmup 2] [--out file.json]"""
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
    ap.add_argument("--range-bytes", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=12)
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
    n, size, chunk, level, part = a.buffers, a.buffer_bytes, a.chunk, a.level, a.range_bytes
    assert size % chunk == 0 and part + chunk < size // 2
    E = n * (size // chunk)
    total = n * size
    slot = L.zjni_compressBound_chunked(size, chunk)
    src, comp, packed = dmalloc(total), dmalloc(n * slot), dmalloc(n * slot)
    back_b, back_r, back_p = dmalloc(total), dmalloc(total), dmalloc(n * part)
    soff, coff, poff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot), dmalloc((n + 1) * 8)
    part_off = upload(np.arange(n + 1, dtype=np.uint64) * part)
    res_c, res_b, res_r, tot_r = dmalloc(n * 8), dmalloc(n * 8), dmalloc(n * 8), dmalloc(n * 8)
    mid = size // 2 + chunk // 3                                        # inside a frame; mid + part ends inside another
    legs = {"R_full": (0, size), "R_1/64": (mid, part), "R_tail": (size - part, part)}
    ranges = {k: upload(np.array([lo, ln] * n, dtype=np.uint64)) for k, (lo, ln) in legs.items()}
    chk(L.zjni_synth_fill_device(src, chunk, 0, E, None))
    chk(L.zjni_compress_chunked_batch_device(src, soff, comp, coff, res_c, n, level, 0, chunk, None))
    chk(L.zjni_pack_batch_device2(comp, coff, res_c, packed, poff, n, None))
    chk(hip.hipDeviceSynchronize())
    frames_bytes = int(download(poff, (n + 1) * 8, np.uint64)[-1])
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

    def call_b():
        return L.zjni_decompress_frames_batch_device(packed, poff, back_b, soff, res_b, n, None, None)

    def ranged(name):
        whole = name == "R_full"
        return lambda: L.zjni_decompress_frames_range_batch_device(packed, poff, back_r if whole else back_p, soff if whole else part_off, ranges[name], res_r, tot_r, n, None, None)

    piece = 256 << 20
    stats4 = (C.c_uint * 4)()
    seen = {}

    def verify(name):
        lo, ln = legs[name]
        assert (download(res_r, n * 8, np.uint64) == ln).all() and (download(tot_r, n * 8, np.uint64) == size).all(), name
        chk(L.zjni_last_frames_range(stats4))
        seen[name] = {"served": stats4[0], "frames": stats4[1], "edges": stats4[2], "errors": stats4[3]}
        if name == "R_full":
            for at in range(0, total, piece):
                m = min(piece, total - at)
                assert (download(back_r, m, at=at) == download(src, m, at=at)).all(), "decoded bytes (R_full) differ at %d" % at
        else:
            got = download(back_p, n * part)
            for i in range(n):
                assert (got[i * part:(i + 1) * part] == download(src, part, at=i * size + lo)).all(), "decoded bytes (%s) differ in buffer %d" % (name, i)

    for _ in range(a.warmup):
        timed(call_b)
        for name in legs:
            timed(ranged(name))
    times = {"B": [], **{k: [] for k in legs}}
    for k in range(a.steps):
        times["B"].append(timed(call_b))
        for name in legs:
            times[name].append(timed(ranged(name)))
            if k == a.steps - 1:
                verify(name)
    assert (download(res_b, n * 8, np.uint64) == size).all()
    for at in range(0, total, piece):
        m = min(piece, total - at)
        assert (download(back_b, m, at=at) == download(src, m, at=at)).all(), "decoded bytes (B) differ at %d" % at

    def stats(ts):
        q = statistics.quantiles(ts, n=4)
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "calls": len(ts)}

    s = {k: stats(v) for k, v in times.items()}
    ratio = s["B"]["median_ms"] / s["R_1/64"]["median_ms"]
    line = {"buffers": n, "buffer_bytes": size, "chunk": chunk, "entries": E, "level": level, "range_bytes": part, "frames_bytes": frames_bytes,
            "B_decompress_frames_whole": s["B"], "R_full": s["R_full"], "R_1/64": s["R_1/64"], "R_tail": s["R_tail"],
            "R_full_minus_B_ms": round(s["R_full"]["median_ms"] - s["B"]["median_ms"], 3),
            "R_1/64_faster_than_B": round(ratio, 1), "required": "R_1/64 at least 2 x faster than B", "met": bool(ratio >= 2.0),
            "last_frames_range": seen, "outputs_compared": "results, totals and all decoded bytes of B and of every ranged leg against the source",
            "build_stamp": zj.build_stamp()}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
