"""GPU (-m gpu): frames from the caller's sequences WITHOUT block delimiters (ZJNI_SEQ_NO_DELIMITERS) through zjni_compress_sequences_batch_device
(zj_seq_cut_kernel: a wave per frame over the prefix, the cut and the records; zj_encode_sequences_nodelim_kernel: the frame loop over the blocks the library cut)
and the host forms.  The cases are those of tests/test_emu_sequences_nodelim.py (tests/sequences_nodelim_cases.py): every slot must hold what the reference's
ZSTD_compressSequences answers with ZSTD_sf_noBlockDelimiters — the frame byte for byte, or its code — and a decodable frame decodes to its source.  Cases of one
level and flag word share a call.  The destinations of a call are adjacent, each exactly its capacity, between guard bytes; the sequence array sits between guard
rows: the guards come back unchanged, and a frame that wrote past its capacity has damaged its neighbour's."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

import sequences_nodelim_cases as NC

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def roomy(c):
    return len(c.data) + (len(c.data) >> 8) + 128 + 3 * (2 * (len(c.data) >> 17) + 8)


def run_batch(gpu, cases, caps=None, grid=0, flags=None):
    """one call for `cases` (same level and flags): [bytes or -code].  caps: a destination capacity per case (default: roomy)."""
    import torch
    level = cases[0].level
    if flags is None:
        flags = cases[0].flags
        assert all(c.level == level and c.flags == flags for c in cases)
    n = len(cases)
    if caps is None:
        caps = [roomy(c) for c in cases]
    src_off, seq_off, dst_off = [0], [0], [GUARD]
    for c, cap in zip(cases, caps):
        src_off.append(src_off[-1] + len(c.data)); seq_off.append(seq_off[-1] + len(c.seqs)); dst_off.append(dst_off[-1] + cap)
    dev = "cuda"
    rows = seq_off[-1]
    seq_h = np.full((rows + 2 * GUARD, 4), 0xA7A7A7A7, dtype=np.uint32)                  # guard rows on both sides of the array
    if rows:
        seq_h[GUARD:GUARD + rows] = np.array([v for c in cases for v in NC.flat(c.seqs)], dtype=np.uint32).reshape(-1, 4)
    seq_d = torch.from_numpy(seq_h.view(np.int32)).to(dev)
    src = torch.frombuffer(bytearray(b"".join(c.data for c in cases) or b"\0"), dtype=torch.uint8).to(dev)
    dst_h = np.full(dst_off[-1] + GUARD, 0x5C, dtype=np.uint8)
    dst = torch.from_numpy(dst_h.copy()).to(dev)
    tensor = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)                    # noqa: E731
    _, _, results = gpu.batch.compress_sequences(src, tensor(src_off), seq_d[GUARD:], tensor(seq_off), level, flags, dst=dst, dst_off=tensor(dst_off), _grid=grid)
    r = results.cpu().tolist()
    back = dst.cpu().numpy()
    assert (back[:GUARD] == 0x5C).all() and (back[dst_off[-1]:] == 0x5C).all(), "a guard around the destinations was written"
    assert (seq_d.cpu().numpy().view(np.uint32) == seq_h).all(), "the sequence array was written"
    out = []
    for i in range(n):
        assert r[i] < 0 or r[i] <= caps[i], (cases[i].name, r[i], caps[i])
        out.append(r[i] if r[i] < 0 else back[dst_off[i]:dst_off[i] + r[i]].tobytes())
    return out


def by_call(cases):
    groups = defaultdict(list)
    for c in cases:
        groups[(c.level, c.flags)].append(c)
    return list(groups.values())


def check_all(gpu, oracle_ref, cases, grid=0):
    """the case list (cases that are asked of the reference, the wrapping ones that are not, the unserved ones), one call per level and flag word"""
    unserved = {c.name for c, served in NC.level5() if not served}
    wrapping = {c.name for c in NC.wrapping()}
    for group in by_call(cases):
        for c, got in zip(group, run_batch(gpu, group, grid=grid)):
            if c.name in wrapping:
                assert got == -NC.E_SEQUENCES, (c.name, got)
            elif c.name in unserved:
                assert got == -201 and isinstance(NC.expected(c), bytes), (c.name, got)
            else:
                NC.check(c, got, oracle_ref)


def whole_list(level):
    cases = [c for c in NC.every_case() + NC.wrapping() + [c for c, _ in NC.level5()] + NC.batch() if c.level == level]
    assert len(cases) >= 20
    return cases


@pytest.mark.parametrize("level", NC.LEVELS)
def test_gpu_nodelim_every_case_is_the_references_answer(gpu, oracle_ref, level):
    check_all(gpu, oracle_ref, whole_list(level))


def test_gpu_nodelim_level5(gpu, oracle_ref):
    """a frame the library does not serve (no row: the conversion skips it) behind and in front of one it serves, in one call and through one workgroup"""
    cases = [c for c, _ in NC.level5() if c.level == 5]
    for order in (cases, cases[::-1]):
        check_all(gpu, oracle_ref, order)
        check_all(gpu, oracle_ref, order, grid=1)


@pytest.mark.parametrize("level", NC.LEVELS)
def test_gpu_nodelim_one_workgroup_meets_every_frame_in_turn(gpu, oracle_ref, level):
    """a grid of one: the wave's prefix words, and the workgroup's uniforms, LDS, scratch slot and repcode history outlive every frame, refused ones included"""
    check_all(gpu, oracle_ref, whole_list(level), grid=1)


def test_gpu_nodelim_random_arrays(gpu, oracle_ref):
    kinds = set()
    for group in by_call(NC.random_arrays()):
        for c, got in zip(group, run_batch(gpu, group)):
            NC.check(c, got, oracle_ref)
            kinds.add(got if isinstance(got, int) else "frame")
    assert {"frame", -NC.E_SEQUENCES} <= kinds


def test_gpu_nodelim_repcodes_flag_changes_nothing(gpu, oracle_ref):
    cases = [c for c in NC.merged_parse() + NC.runs() + NC.tile_edges() if c.level == 3 and c.flags == NC.NO_DELIMITERS]
    for c, got in zip(cases, run_batch(gpu, cases, flags=NC.NO_DELIMITERS | NC.REPCODES)):
        NC.check(c, got, oracle_ref)


def test_gpu_nodelim_every_capacity(gpu, oracle_ref):
    """every capacity from 0 to the frame's size + 32, all in one call per frame: the reference's size and bytes, or its dstSize_tooSmall"""
    for c in NC.tight():
        full = NC.expected(c)
        caps = list(range(0, len(full) + 33))
        seen = set()
        for cap, got in zip(caps, run_batch(gpu, [c] * len(caps), caps=caps)):
            if cap < NC.HEADER_ROOM:
                assert got == -NC.E_DST, (c.name, cap, got)
            else:
                NC.check(c, got, oracle_ref, cap)
            seen.add(got if isinstance(got, int) else "frame")
        assert seen == {-NC.E_DST, "frame"}, (c.name, seen)


def test_gpu_nodelim_descending_offsets_answer_for_the_whole_call(gpu):
    """the slots of a frame are placed by both offset arrays: one descending pair, and every frame of the call answers srcSize_wrong"""
    import torch
    c = NC.tile_edges()[0]
    seqs = torch.from_numpy(np.array(NC.flat(c.seqs) * 3, dtype=np.uint32).reshape(-1, 4).view(np.int32)).to("cuda")
    src = torch.frombuffer(bytearray(c.data * 3), dtype=torch.uint8).to("cuda")
    n, k = len(c.data), len(c.seqs)
    tensor = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")                 # noqa: E731
    dst = torch.zeros(3 * 256, dtype=torch.uint8, device="cuda")
    _, _, results = gpu.batch.compress_sequences(src, tensor([0, 2 * n, n, 3 * n]), seqs, tensor([0, k, 2 * k, 3 * k]), c.level, c.flags, dst=dst, dst_off=tensor([0, 256, 512, 768]))
    assert results.cpu().tolist() == [-72, -72, -72]


def test_gpu_nodelim_host_forms(gpu, oracle_ref):
    L = gpu.lib()
    names = ("tile/65/L3", "run-400000/L3", "match-131072-straddles/L3", "covers-more/402/L3", "ml2/L3", "stuck/L3", "zero-sequences/7/L3", "merged/131079/L3")
    picks = [c for c in NC.every_case() if c.name in names and c.flags == NC.NO_DELIMITERS]
    assert len(picks) == len(names)
    for c in picks + NC.wrapping()[:1]:                # zjni_compress_sequences, one buffer
        want = -NC.E_SEQUENCES if c.name.startswith("wrapping") else NC.expected(c)
        seqs = np.array(NC.flat(c.seqs), dtype=np.uint32).reshape(-1, 4)
        if isinstance(want, int):
            with pytest.raises(gpu.ZstdException) as e:
                gpu.compress_sequences(c.data, seqs, c.level, c.flags)
            assert e.value.getErrorCode() == -want
        else:
            assert gpu.compress_sequences(c.data, seqs, c.level, c.flags) == want, c.name
            assert gpu.compress_sequences(c.data, seqs, c.level, c.flags | gpu.SEQ_REPCODES) == want, c.name
    # zjni_compress_sequences_batch: host arrays, refusals among frames
    n = len(picks)
    vp, sz = C.c_void_p, C.c_size_t
    srcs = [C.create_string_buffer(c.data, max(len(c.data), 1)) for c in picks]
    arrs = [(C.c_uint32 * max(4 * len(c.seqs), 1))(*NC.flat(c.seqs)) for c in picks]
    dsts = [C.create_string_buffer(roomy(c)) for c in picks]
    res = (sz * n)()
    r = L.zjni_compress_sequences_batch((vp * n)(*[C.addressof(s) for s in srcs]), (sz * n)(*[len(c.data) for c in picks]), (vp * n)(*[C.addressof(a) for a in arrs]),
                                        (sz * n)(*[len(c.seqs) for c in picks]), (vp * n)(*[C.addressof(d) for d in dsts]), (sz * n)(*[roomy(c) for c in picks]), res, n, 3, gpu.SEQ_NO_DELIMITERS)
    assert r == 0
    for i, c in enumerate(picks):
        got = -((1 << 64) - res[i]) if res[i] >= 1 << 63 else dsts[i].raw[:res[i]]
        NC.check(c, got, oracle_ref)


@pytest.mark.parametrize("level", (1, 3))
def test_gpu_nodelim_generate_merge_compress_decompress(gpu, level):
    """the library's own seam end to end: device generate_sequences -> host merge_block_delimiters -> compress_sequences(SEQ_NO_DELIMITERS) -> device decompress"""
    import torch
    for size in (4096, 131079, 400000):
        data = NC.SC.prose(size, seed=size + 9)
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda")
        off = torch.tensor([0, size], dtype=torch.int64, device="cuda")
        seqs, seq_off, res = gpu.batch.generate_sequences(src, off, level)
        rows = int(res.cpu()[0])
        assert rows > 0
        first = int(seq_off.cpu()[0])
        with_delimiters = seqs.cpu().numpy().view(np.uint32).reshape(-1, 4)[first:first + rows]
        merged = gpu.merge_block_delimiters(with_delimiters)
        assert len(merged) < rows and (merged[:, 0] != 0).all()
        m = torch.from_numpy(np.ascontiguousarray(merged).view(np.int32)).to("cuda")
        dst, dst_off, r = gpu.batch.compress_sequences(src, off, m, torch.tensor([0, len(merged)], dtype=torch.int64, device="cuda"), level, gpu.SEQ_NO_DELIMITERS)
        csize = int(r.cpu()[0])
        assert 0 < csize < size
        out = torch.zeros(size, dtype=torch.uint8, device="cuda")
        d0 = int(dst_off.cpu()[0])
        dres = gpu.batch.decompress(dst[d0:d0 + csize].contiguous(), torch.tensor([0, csize], dtype=torch.int64, device="cuda"), out, off)
        assert int(dres.cpu()[0]) == size
        assert out.cpu().numpy().tobytes() == data, (level, size)
