"""GPU (-m gpu): the frames written from hand-chosen sequences (tests/seqframes.py; their conditions are asserted in
tests/test_emu_seqframes.py) through the C-ABI on every route that takes them.  This is where the wave-parallel LZ77 executor
(zd_execute_batch / zd_execute_staged, the #if ZJ_ON_GPU half of zj_decode.h) meets them: 64 chained dependencies in a batch, batches
of 4095 / 4096 / 4097 bytes, sources straddling the staged window or the dictionary's end, every overlap and length class at lane 0, lane 63
and six positions between.  Exact bytes, exact results, a 64-byte guard slot behind every destination (gpu_fuzz_decode.run_cases), and
the route counters after every call that is meant to use a pipeline: a frame that fell back to the fused kernel has tested nothing new.

routes   pipelines  ZJNI_DSPLIT_MIN=1, ZJNI_DEC_MB=1   one-block frames: three stages (staged executor), multi-block frames: block stages
         fused      ZJNI_DSPLIT_MIN=10^9, ZJNI_DEC_MB=0  every frame: the fused kernel (unstaged executor)
         mixed      ZJNI_DSPLIT_MIN=10^9, ZJNI_DEC_MB=1  one-block frames: fused kernel, multi-block frames: block stages"""
import ctypes as C

import numpy as np
import pytest

import gpu_fuzz_decode as F
import seqframes as S

pytestmark = pytest.mark.gpu

ROUTES = {"pipelines": ("1", "1"), "fused": ("1000000000", "0"), "mixed": ("1000000000", "1")}


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def lists(gpu):
    a = (C.c_uint * 5)()
    assert gpu.lib().zjni_last_decode_lists2(a) == 0
    return list(a)                 # [0] three-stage pipeline, [1] fused kernel, [2] block stages, [3] their blocks, [4] frames of one stored block copied by stage 1


def by_dictionary(cases):
    groups = {}
    for c in cases:
        groups.setdefault(id(c.dictionary), (c.dictionary, []))[1].append(c)
    return list(groups.values())


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", "ABCDEFGH")
def test_gpu_family_on_every_route(gpu, oracle_ref, monkeypatch, name, route):
    split_min, dec_mb = ROUTES[route]
    monkeypatch.setenv("ZJNI_DSPLIT_MIN", split_min)
    monkeypatch.setenv("ZJNI_DEC_MB", dec_mb)
    for d, group in by_dictionary(S.family(name)):
        built = [S.build_case(c) for c in group]
        cases = [(frame, len(content), content) for frame, content, _, _ in built]
        one_block = sum(S.simple(shape) for _, _, shape, _ in built)
        several = sum(len(shape["blocks"]) > 1 for _, _, shape, _ in built)
        assert one_block + several == len(built)                     # (no frame of one stored block: every family frame carries sequences)

        def run(dd):
            bad = F.run_cases(gpu, cases, dictionary_obj=dd)
            assert not bad, (name, route, [(group[i].name, what) for i, what in bad[:8]])
            l = lists(gpu)
            print(name, route, "dictionary" if d else "plain", "frames", len(built), "one block", one_block, "several", several, "lists", l)
            if route == "pipelines":
                assert l[0] == one_block, l                          # the staged executor took every one-block frame
                if d is None:
                    assert l[2] == several, l                        # ... and the block stages every multi-block one
                # what is left for the fused kernel: the empty guard entries, and multi-block frames with a dictionary (the block stages take none)
                assert l[1] <= len(cases) + (several if d else 0), l
            elif route == "mixed" and d is None:
                assert l[0] == 0 and l[2] == several and l[1] == one_block + len(cases), l
            elif route == "fused":
                assert l[2] == 0 and l[3] == 0, l                    # no block stages, and below ZJNI_DSPLIT_MIN no three stages: the fused kernel is all there is ([0] and [1] keep the last pipeline call's figures)
        if d is None:
            run(None)
        else:
            with gpu.ZstdDictDecompress(d.raw) as dd:
                run(dd)


@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_damaged_random_programs_answer_as_the_reference(gpu, oracle_ref, monkeypatch, route):
    split_min, dec_mb = ROUTES[route]
    monkeypatch.setenv("ZJNI_DSPLIT_MIN", split_min)
    monkeypatch.setenv("ZJNI_DEC_MB", dec_mb)
    damaged = S.damaged_h(oracle_ref, S.family("H"))
    groups = {}
    for c, z, cap, want in damaged:
        groups.setdefault(id(c.dictionary), (c.dictionary, []))[1].append((z, cap, want))
    for d, cases in groups.values():
        if d is None:
            bad = F.run_cases(gpu, cases)
        else:
            with gpu.ZstdDictDecompress(d.raw) as dd:
                bad = F.run_cases(gpu, cases, dictionary_obj=dd)
        assert not bad, (route, bad[:8])


def small_plain_frames():
    """(frame, content) of the dictionary-free frames of families A .. E, one-block and multi-block ones in turn"""
    out = []
    for name in "ABCDE":
        for c in S.family(name):
            if c.dictionary is None:
                frame, content, _, _ = S.build_case(c)
                out.append((frame, content))
    return out


def to_device(torch, pieces):
    blob = b"".join(pieces)
    off = np.zeros(len(pieces) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    return torch.from_numpy(np.frombuffer(blob + b"\0" * 16, dtype=np.uint8).copy()).cuda(), torch.from_numpy(off).cuda()


def test_gpu_buffers_of_many_family_frames(gpu, oracle_ref):
    """5, 64 and 65 frames per buffer through decompress_frames: one frame per wave slot, the contents back to back"""
    import torch
    pool = small_plain_frames()
    assert len(pool) >= 5 + 64 + 65
    bufs, at = [], 0
    for count in (5, 64, 65):
        bufs.append(pool[at:at + count])
        at += count
    src, src_off = to_device(torch, [b"".join(f for f, _ in b) for b in bufs])
    wholes = [b"".join(c for _, c in b) for b in bufs]
    dst_off = np.zeros(len(bufs) + 1, dtype=np.int64)
    dst_off[1:] = np.cumsum([len(w) + 64 for w in wholes])                   # 64 guard bytes behind every buffer's content
    dst = torch.full((int(dst_off[-1]) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    res = gpu.batch.decompress_frames(src, src_off, dst, torch.from_numpy(dst_off).cuda())
    torch.cuda.synchronize()
    out = dst.cpu().numpy().tobytes()
    assert res.cpu().tolist() == [len(w) for w in wholes]
    for i, w in enumerate(wholes):
        o = int(dst_off[i])
        assert out[o:o + len(w)] == w, i
        assert out[o + len(w):o + len(w) + 64] == b"\xA5" * 64, i
    assert gpu.batch.last_frames()["split"] == len(bufs)


def test_gpu_range_cutting_two_family_frames(gpu, oracle_ref):
    """decompress_frames_range: a range that starts inside one family frame and ends inside another"""
    import torch
    pool = small_plain_frames()
    bufs = [pool[10:15], pool[40:105]]
    src, src_off = to_device(torch, [b"".join(f for f, _ in b) for b in bufs])
    wholes = [b"".join(c for _, c in b) for b in bufs]
    ranges = []
    for b in bufs:
        cuts = np.cumsum([0] + [len(c) for _, c in b]).tolist()
        lo, hi = cuts[1] + len(b[1][1]) // 3, cuts[len(b) - 2] + 2 * len(b[-2][1]) // 3      # inside the second frame .. inside the last but one
        ranges.append((lo, hi - lo))
    dst_off = np.zeros(len(bufs) + 1, dtype=np.int64)
    dst_off[1:] = np.cumsum([ln + 64 for _, ln in ranges])
    dst = torch.full((int(dst_off[-1]) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    rng = torch.tensor([v for r in ranges for v in r], dtype=torch.int64, device="cuda")
    res, tot = gpu.batch.decompress_frames_range(src, src_off, dst, torch.from_numpy(dst_off).cuda(), rng)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().tobytes()
    assert res.cpu().tolist() == [ln for _, ln in ranges] and tot.cpu().tolist() == [len(w) for w in wholes]
    for i, (lo, ln) in enumerate(ranges):
        o = int(dst_off[i])
        assert out[o:o + ln] == wholes[i][lo:lo + ln], i
        assert out[o + ln:o + ln + 64] == b"\xA5" * 64, i
    stats = gpu.batch.last_frames_range()
    assert stats["served"] == 2 and stats["edges"] == 4 and stats["frames"] == (5 - 2) + (65 - 2)
