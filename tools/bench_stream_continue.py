#!/usr/bin/env python3
"""What a flush costs with and without stream state on the device: n streams of `size` bytes of the benchmark's mixed-entropy buffers, flushed every
`size / k` bytes, then closed.
  A  what there was before: k calls of zjni_compress_stream_batch_device with final = 0 over the growing prefix (each compresses the stream from byte 0 and
     writes the frame's beginning again), then the closing call over the whole stream;
  B  k + 1 calls of zjni_compress_stream_continue_batch_device over the same prefixes (each compresses what was written since the last flush and writes the
     new bytes only), in front of them the memset that makes the states fresh.
Both in one process, alternating A B A B ..., after warm-up pairs; every call between two device events, a synchronise behind it; a set's time is the sum
of its calls.  Before anything is timed B's outputs, concatenated per stream, are compared with the frames of A's closing call, for every stream.
No torch (rocprofv3 + torch is unreliable): HBM through the HIP runtime, so the same command runs under `rocprofv3 --kernel-trace --stats` for the kernels' times.

usage: bench_stream_continue.py [--n 4096] [--size 262144] [--k 16] [--levels 1,3] [--steps 8] [--warmup 3] [--out file.json]"""
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
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--size", type=int, default=262144)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--levels", default="1,3")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    hip = C.CDLL("libamdhip64.so")
    vp, sz = C.c_void_p, C.c_size_t

    def chk(r):
        assert r == 0, r

    def dmalloc(nbytes):
        p = vp()
        chk(hip.hipMalloc(C.byref(p), sz(max(nbytes, 8))))
        return p

    def upload(arr):
        p = dmalloc(arr.nbytes)
        chk(hip.hipMemcpy(p, arr.ctypes.data_as(vp), sz(arr.nbytes), 1))
        return p

    def download(p, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        chk(hip.hipMemcpy(out.ctypes.data_as(vp), p, sz(nbytes), 2))
        return out

    assert L.zjni_init(0) == 0, "needs a GPU"
    n, size, k = a.n, a.size, a.k
    step = size // k
    assert step * k == size
    whole = dmalloc(n * size)
    chk(L.zjni_synth_fill_device(whole, size, 0, n, None))
    # call j (1 .. k) sees the first j * step bytes of every stream, packed; the closing call sees the k-th prefix again
    prefix, poff = [None], [None]
    for j in range(1, k + 1):
        p = whole if j == k else dmalloc(n * j * step)
        if j < k:
            chk(hip.hipMemcpy2D(p, sz(j * step), whole, sz(size), sz(j * step), sz(n), 3))
        prefix.append(p)
        poff.append(upload(np.arange(n + 1, dtype=np.uint64) * (j * step)))
    flush_at = upload(np.tile(np.arange(1, k + 1, dtype=np.uint32) * step, n))                 # every stream: step, 2 step, ... k step
    flush_off = upload(np.arange(n + 1, dtype=np.uint64) * k)                                   # (all k positions every time: those beyond the prefix and those consumed are ignored)
    mode_open, mode_close = upload(np.zeros(n, dtype=np.uint32)), upload(np.ones(n, dtype=np.uint32))
    cap_a = size + (size >> 8) + 4096 + 64 * (k + 2)
    cap_b = step + (step >> 8) + 4096 + 64 * 5
    dst_a, doff_a = dmalloc(n * cap_a), upload(np.arange(n + 1, dtype=np.uint64) * cap_a)
    dst_b, doff_b = dmalloc(n * cap_b), upload(np.arange(n + 1, dtype=np.uint64) * cap_b)
    res = dmalloc(n * 8)
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

    def stats(ts):
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "sets": len(ts)}

    lines = []
    for level in [int(x) for x in a.levels.split(",")]:
        state_bytes = L.zjni_cstream_state_bytes(level)
        states = dmalloc(n * state_bytes)

        def call_a(j):          # j = k + 1: the closing call
            jj = min(j, k)
            return L.zjni_compress_stream_batch_device(prefix[jj], poff[jj], dst_a, doff_a, res, n, level, 0, flush_at, flush_off, mode_close if j > k else mode_open, None)

        def call_b(j):
            jj = min(j, k)
            return L.zjni_compress_stream_continue_batch_device(prefix[jj], poff[jj], dst_b, doff_b, res, n, level, 0, flush_at, flush_off, mode_close if j > k else mode_open, states, None)

        def fresh():
            return hip.hipMemsetAsync(states, 0, sz(n * state_bytes), None)

        # B's outputs, concatenated per stream, against the frames of A's closing call
        chk(fresh())
        parts = [[] for _ in range(n)]
        for j in range(1, k + 2):
            chk(call_b(j))
            chk(hip.hipDeviceSynchronize())
            r = download(res, n * 8, np.uint64)
            assert (r <= cap_b).all(), "a continuation call failed: %s" % r[r > cap_b][:4]
            out = download(dst_b, n * cap_b).reshape(n, cap_b)
            for i in range(n):
                parts[i].append(out[i, :int(r[i])].tobytes())
        for j in range(1, k + 2):
            chk(call_a(j))
        chk(hip.hipDeviceSynchronize())
        r = download(res, n * 8, np.uint64)
        assert (r <= cap_a).all(), "the closing call of A failed"
        out = download(dst_a, n * cap_a).reshape(n, cap_a)
        frame_bytes = 0
        for i in range(n):
            want = out[i, :int(r[i])].tobytes()
            assert b"".join(parts[i]) == want, "stream %d: the continued stream's frame differs" % i
            frame_bytes += len(want)
        del parts, out

        def set_a():
            return [timed(lambda: call_a(j)) for j in range(1, k + 2)]

        def set_b():
            return [timed(fresh)] + [timed(lambda: call_b(j)) for j in range(1, k + 2)]

        for _ in range(a.warmup):
            set_a(); set_b()
        ta, tb = [], []
        for _ in range(a.steps):
            ta.append(set_a()); tb.append(set_b())
        sa, sb = stats([sum(t) for t in ta]), stats([sum(t) for t in tb])
        spread = sa["max_ms"] - sa["min_ms"]
        line = {"streams": n, "stream_bytes": size, "flushes": k, "level": level, "frame_bytes": frame_bytes,
                "A_from_byte_0": sa, "B_continued": sb, "A_over_B": round(sa["median_ms"] / sb["median_ms"], 2),
                "B_below_A_by_more_than_As_spread": bool(sa["median_ms"] - sb["median_ms"] > spread),
                "last_flush_call": {"A": stats([t[k - 1] for t in ta]), "B": stats([t[k] for t in tb])},
                "closing_call": {"A": stats([t[k] for t in ta]), "B": stats([t[k + 1] for t in tb])},
                "first_flush_call": {"A": stats([t[0] for t in ta]), "B": stats([t[1] for t in tb])},
                "B_state_memset": stats([t[0] for t in tb]), "state_bytes_per_stream": state_bytes,
                "outputs_compared": "B's %d outputs concatenated against A's final frame, all %d streams" % (k + 1, n),
                "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        chk(hip.hipFree(states))
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
