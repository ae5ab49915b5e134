#!/usr/bin/env python3
"""zjni_compress_sequences_batch_device against the plain compress entry on the same bytes, in one process.

Two shapes: `metric`, 65 536 x 64 KiB of the benchmark's mixed-entropy data (zjni_synth_fill_device), and `large`, 1 024 x 1 MiB slices of the xml
fixture (config 1's buffers) whose frames have 128 KiB blocks.  The sequences are the reference's own parse (ZSTD_generateSequences at the level, explicit
delimiters) of a SAMPLE of `--sample` frames; sample frame k's bytes and sequences are then REPLICATED to every frame i with i % sample == k, and both
entries compress that replicated batch — the output line says so.  S: the sequence entry (conversion + frame loop, its one host wait included);
P: zjni_compress_batch_device2 (match finders + entropy stage).  Warm-up calls of each, then S and P alternating, each between two stream events and a
synchronise; medians.  The sample's frames from S are compared with the reference's ZSTD_compressSequences byte for byte and decoded, every result of
the batch is checked, in the run.

usage: bench_sequences.py [--shapes metric,large] [--frames N] [--sample 64] [--steps 7] [--warmup 2] [--level 3] [--out file.json]"""
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
    ap.add_argument("--shapes", default="metric,large")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import sequences_cases as SC
    from oracle import port, ref
    zj = entry.load_package()
    zj.batch.init(0)
    dev = "cuda"
    lines = []
    for shape in a.shapes.split(","):
        size, n = (65536, a.frames or 65536) if shape == "metric" else (1 << 20, a.frames or 1024)
        k = min(a.sample if shape == "metric" else max(a.sample // 8, 1), n)
        assert n % k == 0
        if shape == "metric":
            sample = zj.batch.synth(k, size).cpu().numpy().tobytes()
        else:
            xml = port.decompress(open(os.path.join(ROOT, "tests", "golden", "xml-1.zst"), "rb").read(), 6_000_000)
            sample = b"".join(xml[(i * 4099 * 97) % (len(xml) - size):][:size] for i in range(k))
        frames = [sample[i * size:(i + 1) * size] for i in range(k)]
        seqs = [np.array(SC.flat(SC.ref_generate_sequences(f, a.level)), dtype=np.uint32).reshape(-1, 4) for f in frames]
        counts = np.array([len(s) for s in seqs], dtype=np.int64)
        src = torch.frombuffer(bytearray(sample), dtype=torch.uint8).to(dev).repeat(n // k)
        seq_d = torch.from_numpy(np.concatenate(seqs).view(np.int32)).to(dev).repeat(n // k, 1)
        src_off = zj.batch.uniform_offsets(n, size, dev)
        seq_off = torch.zeros(n + 1, dtype=torch.int64)
        seq_off[1:] = torch.from_numpy(np.cumsum(np.tile(counts, n // k)))
        seq_off = seq_off.to(dev)
        cap = zj.lib().zjni_compressBound(size) + 64 + 3 * (size // 1024 + 2)
        dst = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        dst_off = zj.batch.uniform_offsets(n, cap, dev)
        res_s = torch.empty(n, dtype=torch.int64, device=dev)
        res_p = torch.empty(n, dtype=torch.int64, device=dev)

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if which == "S":
                zj.batch.compress_sequences(src, src_off, seq_d, seq_off, a.level, 0, dst=dst, dst_off=dst_off, results=res_s)
            else:
                zj.batch.compress(src, src_off, dst, dst_off, a.level, results=res_p)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            call("S"); call("P")
        t = {"S": [], "P": []}
        match_ms = []
        for _ in range(a.steps):
            t["P"].append(call("P")); match_ms.append(zj.batch.last_timing()["match"])
            t["S"].append(call("S"))
        # the run checks itself: P's results, S's results, the sample's frames from S against the reference
        assert int((res_p <= 0).sum().item()) == 0 and int((res_s <= 0).sum().item()) == 0
        total_p = int(res_p.sum().item())
        call("S")
        sizes = res_s[:k].cpu().tolist()
        back = dst[:k * cap].cpu().numpy()
        for i in range(k):
            want = SC.ref_compress_sequences(frames[i], [tuple(r) for r in seqs[i].tolist()], a.level, False, False)
            assert back[i * cap:i * cap + sizes[i]].tobytes() == want and ref.decompress(want, size) == frames[i], i
        assert res_s.view(n // k, k).eq(res_s[:k]).all().item()
        ms_s, ms_p, ms_m = statistics.median(t["S"]), statistics.median(t["P"]), statistics.median(match_ms)
        gib = n * size / 2.0 ** 30
        line = {"tool": "bench_sequences", "shape": f"{shape}_{n}x{size}", "level": a.level, "sample_frames": k,
                "replicated": f"bytes and sequences of {k} sampled frames repeated {n // k} times", "sequences_per_frame_mean": round(float(counts.mean()), 1),
                "steps": a.steps, "warmup": a.warmup,
                "sequences_ms": round(ms_s, 3), "sequences_ms_min_max": [round(min(t["S"]), 3), round(max(t["S"]), 3)], "sequences_GiBps": round(gib / (ms_s / 1e3), 2),
                "plain_ms": round(ms_p, 3), "plain_ms_min_max": [round(min(t["P"]), 3), round(max(t["P"]), 3)], "plain_GiBps": round(gib / (ms_p / 1e3), 2),
                "plain_match_ms": round(ms_m, 3), "plain_minus_match_ms": round(ms_p - ms_m, 3) if ms_m > 0 else None,
                "bytes_sequences": int(res_s.sum().item()), "bytes_plain": total_p, "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del src, seq_d, dst
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
