#!/usr/bin/env python3
"""What sizing a decompress batch on the device costs: zjni_decompress_batch_device with host-known offsets (A) against
zjni_decompress_batch_device_sized, which walks the frames, scans the offsets and decodes (B), on the benchmark's batch —
n x 64 KiB mixed-entropy buffers compressed at level 3 by the library and packed tight, as the root of the gather holds them.

Both in one process, alternating A B A B ..., after a warm-up of each; every call between two device events and a synchronise.
The outputs of the last A and B calls are compared with each other and with the source, B's offsets with A's, `needed` with n x size.
No torch (rocprofv3 + torch is unreliable): HBM through the HIP runtime, like tools/prof_driver.py, so the same command also runs under
`rocprofv3 --kernel-trace --stats` (tools/gpu_call.sh's kstats step, with --steps 5) for the times of the four new kernels.

usage: bench_sized_decode.py [--n 65536] [--size 65536] [--steps 24] [--warmup 3] [--out file.json]"""
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
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
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
    n, size = a.n, a.size
    bound = L.zjni_compressBound(size)
    src, comp, packed = dmalloc(n * size), dmalloc(n * bound), dmalloc(n * bound)
    back_a, back_b = dmalloc(n * size), dmalloc(n * size)
    soff = upload(np.arange(n + 1, dtype=np.uint64) * size)
    coff = upload(np.arange(n + 1, dtype=np.uint64) * bound)
    csz, poff = dmalloc(n * 8), dmalloc((n + 1) * 8)
    res_a, res_b, doff, needed, info = dmalloc(n * 8), dmalloc(n * 8), dmalloc((n + 1) * 8), dmalloc(8), dmalloc(n * 40)
    chk(L.zjni_synth_fill_device(src, size, 0, n, None))
    chk(L.zjni_compress_batch_device(src, soff, comp, coff, csz, n, 3, None))
    chk(L.zjni_pack_batch_device2(comp, coff, csz, packed, poff, n, None))
    chk(hip.hipDeviceSynchronize())
    frames_bytes = int(download(poff, (n + 1) * 8, np.uint64)[-1])
    chk(hip.hipFree(comp))
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

    def call_a():
        return L.zjni_decompress_batch_device(packed, poff, back_a, soff, res_a, n, None)

    def call_b():
        return L.zjni_decompress_batch_device_sized(packed, poff, back_b, n * size, 1, 0, info, doff, needed, res_b, n, None, None)

    for _ in range(a.warmup):
        timed(call_a)
        timed(call_b)
    ta, tb = [], []
    for _ in range(a.steps):
        ta.append(timed(call_a))
        tb.append(timed(call_b))

    # outputs: B's offsets are A's, needed is the batch's size, every result is `size`, and the bytes are the source's in both destinations
    assert (download(doff, (n + 1) * 8, np.uint64) == np.arange(n + 1, dtype=np.uint64) * size).all(), "offsets differ"
    assert int(download(needed, 8, np.uint64)[0]) == n * size
    ra, rb = download(res_a, n * 8, np.uint64), download(res_b, n * 8, np.uint64)
    assert (ra == size).all() and (rb == size).all(), "a buffer did not decode"
    piece = 256 << 20
    for at in range(0, n * size, piece):
        m = min(piece, n * size - at)
        want = download(src, m, at=at)
        assert (download(back_a, m, at=at) == want).all() and (download(back_b, m, at=at) == want).all(), "decoded bytes differ at %d" % at

    def stats(ts):
        q = statistics.quantiles(ts, n=4)
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "iqr_ms": round(q[2] - q[0], 4), "calls": len(ts)}

    sa, sb = stats(ta), stats(tb)
    delta = sb["median_ms"] - sa["median_ms"]
    allowed = max(0.05 * sa["median_ms"], sa["iqr_ms"])          # the larger of 5 % of A and A's own spread (its interquartile range) in this run
    line = {"buffers": n, "buffer_bytes": size, "level": 3, "frames_bytes": frames_bytes, "A_host_known_offsets": sa, "B_sized": sb,
            "B_minus_A_ms": round(delta, 4), "allowed_ms": round(allowed, 4), "within_bar": bool(delta <= allowed),
            "outputs_compared": "offsets, needed, results and all decoded bytes of A and B against the source",
            "build_stamp": zj.build_stamp()}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
