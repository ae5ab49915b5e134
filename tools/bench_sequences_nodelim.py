#!/usr/bin/env python3
"""zjni_compress_sequences_batch_device without block delimiters (ZJNI_SEQ_NO_DELIMITERS) against the same entry with them, on the same bytes, in one process.

Two shapes as tools/bench_sequences.py: `metric`, 65 536 x 64 KiB of the benchmark's mixed-entropy data (zjni_synth_fill_device), and `large`, 1 024 x 1 MiB
slices of the xml fixture whose frames have 128 KiB blocks.  The sequences are the reference's own level-3 parse (ZSTD_generateSequences, explicit delimiters) of a
SAMPLE of `--sample` frames, fed twice: E, as they are with flags ZJNI_SEQ_REPCODES (the explicit entry with its repcode walk, what the new mode's frame loop also
runs), and N, after ZSTD_mergeBlockDelimiters with flags ZJNI_SEQ_NO_DELIMITERS (the library cuts the blocks).  Sample frame k's bytes and sequences are REPLICATED
to every frame i with i % sample == k — the output line says so.  Warm-up calls of each, then E and N alternating `--steps` times, each between two stream events
and a synchronise; medians and ranges.  The sample's frames from N are compared with the reference's ZSTD_compressSequences (ZSTD_sf_noBlockDelimiters) byte for
byte and decoded, every result of both batches is checked, in the run.

usage: bench_sequences_nodelim.py [--shapes metric,large] [--frames N] [--sample 64] [--steps 7] [--warmup 2] [--level 3] [--out file.json]"""
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
    import sequences_nodelim_cases as NC
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
        with_d = [SC.ref_generate_sequences(f, a.level) for f in frames]
        merged = [NC.ref_merge(s) for s in with_d]
        src = torch.frombuffer(bytearray(sample), dtype=torch.uint8).to(dev).repeat(n // k)
        src_off = zj.batch.uniform_offsets(n, size, dev)

        def device_array(lists):
            arrs = [np.array(SC.flat(s), dtype=np.uint32).reshape(-1, 4) for s in lists]
            counts = np.array([len(s) for s in arrs], dtype=np.int64)
            seq_d = torch.from_numpy(np.concatenate(arrs).view(np.int32)).to(dev).repeat(n // k, 1)
            off = torch.zeros(n + 1, dtype=torch.int64)
            off[1:] = torch.from_numpy(np.cumsum(np.tile(counts, n // k)))
            return seq_d, off.to(dev), counts
        seq_e, off_e, counts_e = device_array(with_d)
        seq_n, off_n, counts_n = device_array(merged)
        cap = zj.lib().zjni_compressBound(size) + 64 + 3 * (size // 1024 + 2)
        dst = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        dst_off = zj.batch.uniform_offsets(n, cap, dev)
        res = {"E": torch.empty(n, dtype=torch.int64, device=dev), "N": torch.empty(n, dtype=torch.int64, device=dev)}

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if which == "E":
                zj.batch.compress_sequences(src, src_off, seq_e, off_e, a.level, zj.SEQ_REPCODES, dst=dst, dst_off=dst_off, results=res["E"])
            else:
                zj.batch.compress_sequences(src, src_off, seq_n, off_n, a.level, zj.SEQ_NO_DELIMITERS, dst=dst, dst_off=dst_off, results=res["N"])
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            call("E"); call("N")
        t = {"E": [], "N": []}
        for _ in range(a.steps):
            t["E"].append(call("E")); t["N"].append(call("N"))
        # the run checks itself: every result of both, the sample's frames from N against the reference
        assert int((res["E"] <= 0).sum().item()) == 0 and int((res["N"] <= 0).sum().item()) == 0
        call("N")
        sizes = res["N"][:k].cpu().tolist()
        back = dst[:k * cap].cpu().numpy()
        for i in range(k):
            want = NC.ref_compress_nodelim(frames[i], merged[i], a.level, False)
            assert back[i * cap:i * cap + sizes[i]].tobytes() == want and ref.decompress(want, size) == frames[i], i
        assert res["N"].view(n // k, k).eq(res["N"][:k]).all().item()
        ms = {w: statistics.median(t[w]) for w in t}
        gib = n * size / 2.0 ** 30
        line = {"tool": "bench_sequences_nodelim", "shape": f"{shape}_{n}x{size}", "level": a.level, "sample_frames": k,
                "replicated": f"bytes and sequences of {k} sampled frames repeated {n // k} times",
                "sequences_per_frame_mean": {"explicit": round(float(counts_e.mean()), 1), "merged": round(float(counts_n.mean()), 1)},
                "steps": a.steps, "warmup": a.warmup,
                "explicit_repcodes_ms": round(ms["E"], 3), "explicit_repcodes_ms_min_max": [round(min(t["E"]), 3), round(max(t["E"]), 3)], "explicit_repcodes_GiBps": round(gib / (ms["E"] / 1e3), 2),
                "nodelim_ms": round(ms["N"], 3), "nodelim_ms_min_max": [round(min(t["N"]), 3), round(max(t["N"]), 3)], "nodelim_GiBps": round(gib / (ms["N"] / 1e3), 2),
                "nodelim_over_explicit": round(ms["N"] / ms["E"], 4),
                "bytes_explicit": int(res["E"].sum().item()), "bytes_nodelim": int(res["N"].sum().item()), "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del src, seq_e, seq_n, dst
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
