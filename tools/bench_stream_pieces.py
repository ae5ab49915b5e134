#!/usr/bin/env python3
"""What the close of an unflushed stream costs with and without the eager mode: one stream written in 32 KiB writes (ZSTD_e_continue), then closed, on
  P  a plain handle (zjni_createCStream): every write buffers, the close compresses the whole stream — what there was before the eager mode;
  E  an eager handle (zjni_createCStream2 with ZJNI_CSTREAM_EAGER): a write that completes a 128 KiB piece launches its compression, later writes
     collect the frame bytes, the close compresses the buffered rest.
Two streams of the benchmark's mixed-entropy buffers: 2 MiB at level 3 and 512 KiB at level 1 (the levels' windows).  Both handles in one process,
alternating P E P E ..., after warm-up rounds; host clock around each call (every call ends in a synchronise of the handle's stream, or launches and
returns); reported are the close call's wall time and the whole stream's (first write to the end of the close).  Every round the two frames are
compared with each other.  The writes follow each other without a pause: a producer that does work between its writes gives the device that time too.

usage: bench_stream_pieces.py [--steps 15] [--warmup 3] [--write 32768] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--write", type=int, default=32768)
    ap.add_argument("--out")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    assert L.zjni_init(0) == 0, "needs a GPU"

    def stats(ts):
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "rounds": len(ts)}

    lines = []
    for level, size in ((3, 2 << 20), (1, 512 << 10)):
        data = b"".join(zj.synth_host(65536, i, 1) for i in range(size // 65536))
        assert len(data) == size
        cap = size + (size >> 8) + 4096 + 64 * 5 + 32 * 4416
        dst = C.create_string_buffer(cap)
        handles = {"P": L.zjni_createCStream2(level, 0, 0), "E": L.zjni_createCStream2(level, 0, 1)}
        assert all(handles.values())

        def stream(h):
            """-> (frame, ms of the close, ms of the whole stream, ms of the slowest write)"""
            out, worst = [], 0.0
            t0 = time.perf_counter()
            for at in range(0, size, a.write):
                t1 = time.perf_counter()
                r = L.zjni_cstream_compress(h, dst, cap, data[at:at + a.write], min(a.write, size - at), 0)
                worst = max(worst, time.perf_counter() - t1)
                assert not L.zjni_isError(r), r
                if r:
                    out.append(dst.raw[:r])
            t2 = time.perf_counter()
            r = L.zjni_cstream_compress(h, dst, cap, None, 0, 2)
            t3 = time.perf_counter()
            assert not L.zjni_isError(r), r
            out.append(dst.raw[:r])
            assert L.zjni_cstream_reset(h) == 0
            return b"".join(out), (t3 - t2) * 1e3, (t3 - t0) * 1e3, worst * 1e3

        times = {k: {"close": [], "whole": [], "worst_write": []} for k in handles}
        frame_bytes = 0
        for rnd in range(a.warmup + a.steps):
            frames = {}
            for k in ("P", "E"):
                frames[k], close_ms, whole_ms, worst_ms = stream(handles[k])
                if rnd >= a.warmup:
                    times[k]["close"].append(close_ms); times[k]["whole"].append(whole_ms); times[k]["worst_write"].append(worst_ms)
            assert frames["P"] == frames["E"], "round %d: the eager handle's frame differs from the plain handle's" % rnd
            frame_bytes = len(frames["P"])
        for h in handles.values():
            L.zjni_freeCStream(h)
        p, e = {k: stats(v) for k, v in times["P"].items()}, {k: stats(v) for k, v in times["E"].items()}
        spread = max(p["whole"]["max_ms"] - p["whole"]["min_ms"], e["whole"]["max_ms"] - e["whole"]["min_ms"])
        line = {"level": level, "stream_bytes": size, "write_bytes": a.write, "pieces": size // 131072, "frame_bytes": frame_bytes,
                "plain": p, "eager": e, "close_plain_over_eager": round(p["close"]["median_ms"] / max(e["close"]["median_ms"], 1e-6), 2),
                "whole_eager_minus_plain_ms": round(e["whole"]["median_ms"] - p["whole"]["median_ms"], 3), "whole_spread_ms": round(spread, 3),
                "whole_eager_worse_by_more_than_the_spread": bool(e["whole"]["median_ms"] - p["whole"]["median_ms"] > spread),
                "frames_compared": "plain against eager, every round (%d)" % (a.warmup + a.steps), "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
