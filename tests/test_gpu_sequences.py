"""GPU (-m gpu): frames from the caller's sequences through zjni_compress_sequences_batch_device (zj_seq_convert_kernel: a wave per frame over the
ZSTD_Sequence array; zj_encode_sequences_kernel: the frame loop over the caller's blocks) and the host forms.  The cases are those of
tests/test_emu_sequences.py (tests/sequences_cases.py): every slot must hold what the reference's ZSTD_compressSequences answers — the frame byte for
byte, or its code — and a decodable frame decodes to its source.  Cases of one level and flag word share a call, so different workgroups meet
different shapes in one launch.  The destinations of a call are adjacent, each exactly its capacity, between guard bytes in front of the first and
behind the last; the sequence array sits between guard rows: the guards come back unchanged, and a frame that wrote past its capacity has damaged
its neighbour's."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

import sequences_cases as SC

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def roomy(c):
    return len(c.data) + (len(c.data) >> 8) + 128 + 3 * (len(c.seqs) + 1)


def run_batch(gpu, cases, caps=None, grid=0, layout=None):
    """one call for `cases` (same level and flags): [bytes or -code].  caps: a destination capacity per case (default: roomy).  layout: (rows, seq_off) where the
    sequence array is not simply the cases' arrays one behind the other"""
    import torch
    level, flags = cases[0].level, cases[0].flags
    assert all(c.level == level and c.flags == flags for c in cases)
    n = len(cases)
    if caps is None:
        caps = [roomy(c) for c in cases]
    src_off, seq_off, dst_off = [0], [0], [GUARD]
    for c, cap in zip(cases, caps):
        src_off.append(src_off[-1] + len(c.data)); seq_off.append(seq_off[-1] + len(c.seqs)); dst_off.append(dst_off[-1] + cap)
    dev = "cuda"
    all_rows = [s for c in cases for s in c.seqs]
    if layout is not None:
        all_rows, seq_off = layout
        assert len(seq_off) == n + 1 and max(seq_off) <= len(all_rows) + 1
    rows = len(all_rows)
    seq_h = np.full((rows + 2 * GUARD, 4), 0xA7A7A7A7, dtype=np.uint32)                  # guard rows on both sides of the array
    if rows:
        seq_h[GUARD:GUARD + rows] = np.array(SC.flat(all_rows), dtype=np.uint32).reshape(-1, 4)
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


@pytest.mark.parametrize("group", ("smallest", "from_generator", "multi_block", "long_codes"))
def test_gpu_sequences_every_case_is_the_references_answer(gpu, oracle_ref, group):
    for cases in by_call(getattr(SC, group)()):
        for c, got in zip(cases, run_batch(gpu, cases)):
            SC.check(c, got, oracle_ref)


def test_gpu_sequences_other_levels(gpu, oracle_ref):
    for c, served in SC.other_levels():
        got = run_batch(gpu, [c])[0]
        if served:
            SC.check(c, got, oracle_ref)
        else:
            assert got == -201, (c.name, got)


def test_gpu_sequences_refusals_stay_in_their_slots(gpu, oracle_ref):
    """200 frames, every tenth damaged: the damaged slots answer 107 and nobody else's frame changes"""
    cases = SC.batch()
    assert len(cases) == 200
    refused = 0
    for group in by_call(cases):
        for c, got in zip(group, run_batch(gpu, group)):
            SC.check(c, got, oracle_ref)
            assert isinstance(got, bytes) == c.decodes, c.name
            refused += got == -SC.E_SEQUENCES
    assert refused == 18                               # every tenth frame, but the two whose damage lies behind the last block


def test_gpu_sequences_one_workgroup_meets_every_frame_in_turn(gpu, oracle_ref):
    """a grid of one: the workgroup's uniforms, LDS, scratch slot and repcode history outlive every frame, refused ones included"""
    for flags in (0, SC.REPCODES):
        cases = [c for c in SC.batch() + SC.multi_block() + SC.smallest() + SC.long_codes() if c.level == 3 and c.flags == flags]
        assert len(cases) >= 60 and sum(not c.decodes for c in cases) >= 6
        for c, got in zip(cases, run_batch(gpu, cases, grid=1)):
            SC.check(c, got, oracle_ref)


def test_gpu_sequences_every_capacity(gpu, oracle_ref):
    """every capacity from 0 to the frame's size + 32, all in one call per frame: the reference's size and bytes, or its dstSize_tooSmall"""
    for c in SC.tight():
        full = SC.expected(c)
        caps = list(range(0, len(full) + 33))
        seen = set()
        for cap, got in zip(caps, run_batch(gpu, [c] * len(caps), caps=caps)):
            if cap < SC.HEADER_ROOM:
                assert got == -SC.E_DST, (c.name, cap, got)
            else:
                SC.check(c, got, oracle_ref, cap)
            seen.add(got if isinstance(got, int) else "frame")
        assert seen == {-SC.E_DST, "frame"}, (c.name, seen)


def test_gpu_sequences_host_forms_and_bound(gpu, oracle_ref):
    L, R = gpu.lib(), SC._lib()
    for n in (0, 1, 1023, 131072, 2 << 20):
        assert gpu.sequence_bound(n) == L.zjni_sequenceBound(n) == R.ZSTD_sequenceBound(n)
    picks = [c for c in SC.smallest() + SC.multi_block() + SC.long_codes() if c.name in ("empty", "lone7", "one-block/65", "raw-second", "rle-second", "ll70000-ml70000", "ml2", "offset-one-too-far")]
    assert len(picks) >= 10
    for c in picks:                                    # zjni_compress_sequences, one buffer
        want = SC.expected(c)
        seqs = np.array(SC.flat(c.seqs), dtype=np.uint32).reshape(-1, 4)
        if isinstance(want, int):
            with pytest.raises(gpu.ZstdException) as e:
                gpu.compress_sequences(c.data, seqs, c.level, c.flags)
            assert e.value.getErrorCode() == -want
        else:
            assert gpu.compress_sequences(c.data, seqs, c.level, c.flags) == want, c.name
    # zjni_compress_sequences_batch: host arrays, a refusal among frames
    group = [c for c in picks if c.level == 3 and c.flags == 0]
    n = len(group)
    assert n >= 4 and any(isinstance(SC.expected(c), int) for c in group)
    vp, sz = C.c_void_p, C.c_size_t
    srcs = [C.create_string_buffer(c.data, max(len(c.data), 1)) for c in group]
    arrs = [(C.c_uint32 * max(4 * len(c.seqs), 1))(*SC.flat(c.seqs)) for c in group]
    dsts = [C.create_string_buffer(roomy(c)) for c in group]
    res = (sz * n)()
    r = L.zjni_compress_sequences_batch((vp * n)(*[C.addressof(s) for s in srcs]), (sz * n)(*[len(c.data) for c in group]), (vp * n)(*[C.addressof(a) for a in arrs]),
                                        (sz * n)(*[len(c.seqs) for c in group]), (vp * n)(*[C.addressof(d) for d in dsts]), (sz * n)(*[roomy(c) for c in group]), res, n, 3, 0)
    assert r == 0
    for i, c in enumerate(group):
        got = -((1 << 64) - res[i]) if res[i] >= 1 << 63 else dsts[i].raw[:res[i]]
        SC.check(c, got, oracle_ref)
    assert L.zjni_isError(L.zjni_compress_sequences_batch(None, None, None, None, None, None, res, 1, 3, 0)) and L.zjni_isError(L.zjni_compress_sequences(None, 0, None, 0, None, 0, 3, 16))


def check_mixed(gpu, oracle_ref, cases, code, grid, layout=None):
    """every served slot the reference's frame, every skipped slot its code (run_batch has looked at the guards)"""
    got = run_batch(gpu, cases, grid=grid, layout=layout)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        if c.name.startswith(SC.SKIPPED):
            assert g == -code, (c.name, grid, g if isinstance(g, int) else len(g))
        else:
            SC.check(c, g, oracle_ref)


@pytest.mark.parametrize("grid", (1, 2, 0))
def test_gpu_sequences_level5_skipped_frames_among_served(gpu, oracle_ref, grid):
    """one call at level 5 in which frames the entry does not serve (just over 128 KiB: 201, the conversion writes block count 0 and moves on) stand at index 0, 1, in
    the middle and last among 36 served ones, in both orders, through one workgroup, two, and the default grid"""
    for cases in SC.mixed_level5():
        assert 2 <= sum(c.name.startswith(SC.SKIPPED) for c in cases) <= 3 and len(cases) >= 38
        for order in (cases, cases[::-1]):
            check_mixed(gpu, oracle_ref, order, 201, grid)


@pytest.mark.parametrize("grid", (1, 2, 0))
@pytest.mark.parametrize("at", (0, 1, 20))
def test_gpu_sequences_one_descending_pair_among_served(gpu, oracle_ref, at, grid):
    """one call at level 3 in which ONE frame's pair of sequence offsets descends: the conversion marks the slot ZS_NO_FRAME, for which the frame loop answers
    externalSequences_invalid (zs_compress_frame), and every other frame of the call is the reference's"""
    cases = SC.mixed_descending(at)
    check_mixed(gpu, oracle_ref, cases, SC.E_SEQUENCES, grid, layout=SC.descending_rows(cases, at))
