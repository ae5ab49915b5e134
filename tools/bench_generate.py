#!/usr/bin/env python3
"""zjni_generate_sequences_batch_device against the plain compress entry on the same bytes, in one process.

Three lines: `metric`, 65 536 x 64 KiB of the benchmark's mixed-entropy data (zjni_synth_fill_device) at level 3 and at level 1, and `large`, 1 024 x 1 MiB
slices of the xml fixture (config 1's buffers, 8 slices repeated) at level 3.  G: the generate entry (one kernel: parse and export, a wave per frame) into slots
of zjni_sequenceBound rows a frame; P: zjni_compress_batch_device2 (match finders + entropy stage), with its match-kernel time from zjni_last_timing where the
route reports one.  Warm-up calls of each, then G and P alternating, each between two stream events and a synchronise; medians and ranges.  Every result of
both batches is checked and a sample of frames from G is compared with the reference's ZSTD_generateSequences entry for entry, in the run.

usage: bench_generate.py [--shapes metric3,metric1,large3] [--frames N] [--sample 64] [--steps 7] [--warmup 2] [--out file.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="metric3,metric1,large3")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import generate_cases as GC
    from oracle import port
    zj = entry.load_package()
    zj.batch.init(0)
    dev = "cuda"
    lines = []
    for shape in a.shapes.split(","):
        kind, level = shape[:-1], int(shape[-1])
        size, n = (65536, a.frames or 65536) if kind == "metric" else (1 << 20, a.frames or 1024)
        if kind == "metric":
            src = zj.batch.synth(n, size)
        else:
            k = min(8, n)
            xml = port.decompress(open(os.path.join(ROOT, "tests", "golden", "xml-1.zst"), "rb").read(), 6_000_000)
            sample = b"".join(xml[(i * 4099 * 97) % (len(xml) - size):][:size] for i in range(k))
            src = torch.frombuffer(bytearray(sample), dtype=torch.uint8).to(dev).repeat(n // k)
        src_off = zj.batch.uniform_offsets(n, size, dev)
        rows = zj.sequence_bound(size)
        seqs = torch.empty((n * rows, 4), dtype=torch.int32, device=dev)
        seq_off = zj.batch.uniform_offsets(n, rows, dev)
        cap = zj.lib().zjni_compressBound(size) + 64
        dst = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        dst_off = zj.batch.uniform_offsets(n, cap, dev)
        res_p = torch.empty(n, dtype=torch.int64, device=dev)
        res_g = [None]

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if which == "G":
                res_g[0] = zj.batch.generate_sequences(src, src_off, level, seqs=seqs, seq_off=seq_off)[2]
            else:
                zj.batch.compress(src, src_off, dst, dst_off, level, results=res_p)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            call("G"); call("P")
        t = {"G": [], "P": []}
        match_ms = []
        for _ in range(a.steps):
            t["P"].append(call("P")); match_ms.append(zj.batch.last_timing()["match"])
            t["G"].append(call("G"))
        counts = res_g[0]
        assert int((res_p <= 0).sum().item()) == 0 and int((counts <= 0).sum().item()) == 0
        last = zj.batch.last_generate()
        assert last == {"lane": 0, "wave": n, "refused": 0}, last
        picks = sorted(set(int(i) for i in np.linspace(0, n - 1, min(a.sample, n))))
        for i in picks:
            got = seqs[i * rows:i * rows + int(counts[i].item())].cpu().numpy().view(np.uint32)
            want = GC.ref_rows(src[i * size:(i + 1) * size].cpu().numpy().tobytes(), level)
            assert got.shape == want.shape and (got == want).all(), (shape, i)
        total = int(counts.sum().item())
        ms_g, ms_p, ms_m = statistics.median(t["G"]), statistics.median(t["P"]), statistics.median(match_ms)
        gib = n * size / 2.0 ** 30
        line = {"tool": "bench_generate", "shape": f"{kind}_{n}x{size}", "level": level, "route": "wave", "frames_compared_with_reference": len(picks),
                "steps": a.steps, "warmup": a.warmup, "entries_total": total, "entries_per_frame_mean": round(total / n, 1),
                "generate_ms": round(ms_g, 3), "generate_ms_min_max": [round(min(t["G"]), 3), round(max(t["G"]), 3)], "generate_GiBps": round(gib / (ms_g / 1e3), 2),
                "plain_ms": round(ms_p, 3), "plain_ms_min_max": [round(min(t["P"]), 3), round(max(t["P"]), 3)], "plain_GiBps": round(gib / (ms_p / 1e3), 2),
                "plain_match_ms": round(ms_m, 3) if ms_m > 0 else None, "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del src, seqs, dst
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
