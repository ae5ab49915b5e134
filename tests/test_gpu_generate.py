"""GPU (-m gpu): the matchers' sequences out through zjni_generate_sequences_batch_device (zj_generate_kernel: parse and export, a wave per frame) and the host forms.  The cases are those
of tests/test_emu_generate.py (tests/generate_cases.py): every frame's slots must hold what the reference's ZSTD_generateSequences answers, entry for entry, or
its code.  The slots of a call are adjacent, each exactly its capacity, between guard rows in front of the first and behind the last: the guards come back
unchanged, and a frame that wrote past its slots has damaged its neighbour's.  No frame of any call is left out of the comparison."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

import generate_cases as GC
import sequences_cases as SC

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA7A7A7A7


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def bound(n):
    return n // 3 + 1 + n // 1024 + 1                     # ZSTD_sequenceBound


def run_batch(gpu, datas, level, caps=None, grid=0):
    """one call: ([uint32 [k, 4] array or -code per frame], last_generate()).  caps: slots per frame (default: the bound)."""
    import torch
    n = len(datas)
    if caps is None:
        caps = [bound(len(d)) for d in datas]
    src_off, seq_off = [0], [GUARD]
    for d, cap in zip(datas, caps):
        src_off.append(src_off[-1] + len(d)); seq_off.append(seq_off[-1] + cap)
    rows_h = np.full((seq_off[-1] + GUARD, 4), FILL, dtype=np.uint32)
    rows = torch.from_numpy(rows_h.view(np.int32)).cuda()
    src = torch.frombuffer(bytearray(b"".join(datas) or b"\0"), dtype=torch.uint8).cuda()
    tensor = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")                    # noqa: E731
    _, _, results = gpu.batch.generate_sequences(src, tensor(src_off), level, seqs=rows, seq_off=tensor(seq_off), _grid=grid)
    r = results.cpu().tolist()
    back = rows.cpu().numpy().view(np.uint32)
    assert (back[:GUARD] == FILL).all() and (back[seq_off[-1]:] == FILL).all(), "a guard row around the slots was written"
    out = []
    for i in range(n):
        assert r[i] < 0 or r[i] <= caps[i], (i, r[i], caps[i])
        if r[i] >= 0:
            assert (back[seq_off[i] + r[i]:seq_off[i + 1]] == FILL).all(), (i, "rows behind the frame's answer were written")
        out.append(r[i] if r[i] < 0 else back[seq_off[i]:seq_off[i] + r[i]].copy())
    return out, gpu.batch.last_generate()


def as_list(a):
    return a if isinstance(a, int) else [tuple(int(v) for v in row) for row in a]


def same(got, want):
    if isinstance(got, int) or isinstance(want, int):
        return isinstance(got, int) and isinstance(want, int) and got == want
    return got.shape == want.shape and bool((got == want).all())


def test_gpu_generate_every_case_one_call_per_level(gpu, oracle_ref):
    by_level = defaultdict(list)
    for c in GC.every_case():
        by_level[c.level].append(c)
    assert set(by_level) == {1, 2, 3, 4, 5, 6, 8, -5}
    checked = 0
    for level, cases in sorted(by_level.items()):
        got, last = run_batch(gpu, [c.data for c in cases], level)
        for c, g in zip(cases, got):
            GC.check(c, as_list(g))
            checked += 1
        assert last == {"lane": 0, "wave": len(cases), "refused": sum(isinstance(g, int) for g in got)}, (level, last)
    assert checked == len(GC.every_case())


def test_gpu_generate_one_workgroup_meets_every_frame(gpu, oracle_ref):
    """a grid of one: 40 mixed frames, every fifth of 3 bytes — the refusals stay in their own slots, and what a frame left in the workgroup does not reach the next"""
    cases = GC.small_random()[:40]
    datas = [b"abc" if i % 5 == 4 else c.data for i, c in enumerate(cases)]
    for level in (3, 1, 5):
        got, last = run_batch(gpu, datas, level, grid=1)
        for i, (d, g) in enumerate(zip(datas, got)):
            want = GC.ref_rows(d, level)
            assert same(g, want), (level, i, len(d))
            assert (i % 5 == 4) == isinstance(g, int) and (i % 5 != 4 or g == -GC.E_PRODUCER), (level, i, g if isinstance(g, int) else len(g))
        assert last == {"lane": 0, "wave": 40, "refused": 8}


def test_gpu_generate_every_capacity(gpu, oracle_ref):
    """two frames, one of them two blocks, every capacity from 0 to n + 1 in one call: 70 exactly where a block does not fit, the neighbours' slots intact"""
    a, _, b = GC.capacity_frames()
    assert a.level == b.level == 3
    datas, caps, wants = [], [], []
    for c in (a, b):
        full = GC.expected(c)
        for cap in range(0, len(full) + 2):
            datas.append(c.data); caps.append(cap); wants.append(full if cap >= len(full) else -GC.E_DST)
    got, _ = run_batch(gpu, datas, 3, caps=caps)
    for i, (g, w) in enumerate(zip(got, wants)):
        assert as_list(g) == w, (i, caps[i])
    assert sum(isinstance(w, int) for w in wants) >= 40 and len(GC.blocks_of(GC.expected(b))) == 2


def test_gpu_generate_host_forms(gpu, oracle_ref):
    zj = gpu
    for c in (GC.Case("host/text", GC.text(5000), 3, None), GC.Case("host/two-blocks", GC.text(GC.BLOCK + 700), 1, None), GC.Case("host/level-6", GC.text(9000), 6, None),
              GC.Case("host/empty", b"", 3, None), GC.Case("host/level-0", GC.text(3000), 0, None)):
        GC.check(c, as_list(zj.generate_sequences(c.data, c.level)))
    for data, level, code in ((b"abc", 3, GC.E_PRODUCER), (GC.text(GC.BLOCK + 7), 4, GC.E_UNSUPPORTED), (b"abcdefgh", 9, 42)):
        with pytest.raises(zj.ZstdException) as e:
            zj.generate_sequences(data, level)
        assert e.value.getErrorCode() == code, (level, e.value.getErrorCode())
    # the batch form: four frames, one refused, one with a slot too few
    L = zj.lib()
    datas = [GC.text(2000), b"abcd", GC.periodic(3000, 5), GC.text(900)]
    want = [GC.ref_rows(d, 1) for d in datas]
    caps = [len(want[0]) + 4, 8, len(want[2]), len(want[3]) - 1]
    outs = [np.full((cap, 4), FILL, dtype=np.uint32) for cap in caps]
    vp, sz = C.c_void_p, C.c_size_t
    res = (sz * 4)()
    r = L.zjni_generate_sequences_batch((vp * 4)(*[C.cast(C.c_char_p(d), vp) for d in datas]), (sz * 4)(*[len(d) for d in datas]), (vp * 4)(*[o.ctypes.data for o in outs]),
                                        (sz * 4)(*caps), res, 4, 1, 0)
    assert r == 0
    code = lambda v: -((1 << 64) - v) if v >= 1 << 63 else v                              # noqa: E731
    assert [code(v) for v in res] == [len(want[0]), -GC.E_PRODUCER, len(want[2]), -GC.E_DST]
    assert (outs[0][:res[0]] == want[0]).all() and (outs[0][res[0]:] == FILL).all() and (outs[2] == want[2]).all() and (outs[1] == FILL).all()
    merged = zj.merge_block_delimiters(zj.generate_sequences(GC.text(GC.BLOCK + 700), 3))
    assert len(merged) and (merged[:, 0] != 0).all() and int(merged[:, 1].sum() + merged[:, 2].sum()) <= GC.BLOCK + 700


def test_gpu_generate_round_trip_on_the_device(gpu, oracle_ref):
    """batch.generate_sequences into batch.compress_sequences into batch.decompress, 512 x 16 KiB: the decoded bytes are the source"""
    import torch
    zj = gpu
    n, size = 512, 16 * GC.KiB
    big = GC.text(2 << 20)
    data = b"".join(big[(i * 3001) % ((2 << 20) - size):][:size] if i % 4 else GC.periodic(size, i) for i in range(n))
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    src_off = zj.batch.uniform_offsets(n, size, "cuda")
    for level, flags in ((3, 0), (1, SC.REPCODES), (-3, 0)):
        seqs, seq_off, counts = zj.batch.generate_sequences(src, src_off, level)
        assert int(counts.min()) >= 1
        # the compress entry takes a frame's rows from its slots: what lies behind the block that ends the source is never looked at
        dst, dst_off, sizes = zj.batch.compress_sequences(src, src_off, seqs, seq_off, level, flags)
        assert int(sizes.min()) > 0, (level, int(sizes.min()))
        packed, packed_off = zj.batch.pack(sizes, dst, dst_off)
        out = torch.empty(n * size, dtype=torch.uint8, device="cuda")
        res = zj.batch.decompress(packed, packed_off, out, src_off)
        assert bool((res == size).all()), level
        assert bool((out == src).all()), level
        assert int(sizes.sum()) < n * size // 2
