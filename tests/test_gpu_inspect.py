"""GPU (-m gpu): sizing and placing a decompress batch on the device from its frames alone.  zjni_inspect_batch_device against zjni_inspect
and the reference for every buffer; zjni_decompress_offsets_device against a Python prefix sum; zjni_decompress_batch_device_sized against
zjni_decompress_batch_device_usingDDict called with the same offsets; batch.decompress_sized + pack against the original data.  One pool of
buffers (tests/inspect_cases.py: whole, concatenated, truncated and damaged frames, a 1 MiB stream frame, forty tiny frames in one buffer)
serves every batch size; the blob starts at an odd offset and ends with truncated and malformed buffers."""
import numpy as np
import pytest

import inspect_cases as ic

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)       # lane, wave and scan-group borders
MAXU = (1 << 64) - 1


class World:
    pass


@pytest.fixture(scope="module")
def world(zj, oracle_ref):
    import torch
    zj.batch.init(0)
    w = World()
    w.torch, w.zj = torch, zj
    R = ic.setup_ref(oracle_ref)
    cases, valid = ic.build_cases(oracle_ref, with_goldens=False, n_random=500)
    big = ic.stream_data(1 << 20)
    zbig = oracle_ref.compress_stream(big, 3, chunk=1 << 17)
    pool = [ic.join("stream_1MiB", [ic.Piece(zbig, big, nosize=True)])] + cases
    by_name = {c.name: c for c in pool}
    w.pool, w.tail = pool, [by_name["one"], by_name["stream_cut"], by_name["xmlsmall[:7]"], by_name["skip_short_by_one"]]
    for c in pool:
        fi = ic.host_info(zj.lib(), c.data)
        c.info = (fi.content, fi.bound, fi.firstFrameSize, fi.dictID, fi.frames, fi.skippable, fi.flags)
        assert c.info[:4] == ic.ref_info(R, c.data), c.name
    assert by_name["stream_1MiB"].info[0] == ic.UNKNOWN and by_name["stream_1MiB"].info[1] >= 8 << 17       # >= 8 blocks, no content size
    assert by_name["forty_tiny_frames"].info[4] == 40
    w.dict_bytes = ic.dictionary(oracle_ref)
    w.ddict = zj.ZstdDictDecompress(w.dict_bytes)
    w.batches = {}
    yield w
    w.ddict.close()


def batch_of(w, n):
    """n buffers of the pool in order (cyclically), the last four a valid frame and three truncated / malformed ones; the blob begins at byte 1"""
    if n not in w.batches:
        entries = [w.pool[i % len(w.pool)] for i in range(n)]
        if n >= 8:
            entries[-4:] = w.tail
        blob = b"\xAA" + b"".join(c.data for c in entries)
        off = np.cumsum([1] + [len(c.data) for c in entries]).astype(np.int64)
        assert len(blob) < 16 << 20
        t = w.torch
        w.batches[n] = (entries, t.frombuffer(bytearray(blob), dtype=t.uint8).cuda(), t.from_numpy(off).cuda())
    return w.batches[n]


def slots_of(entries, align, slot_max):
    out = []
    for c in entries:
        content, bound = c.info[0], c.info[1]
        s = content if content < ic.ERROR else (bound if bound != ic.ERROR else 0)
        if slot_max and s > slot_max:
            s = 0
        out.append(min((s + align - 1) // align * align, MAXU))
    return out


def prefix_of(slots, cap):
    pre, run = [0], 0
    for s in slots:
        run = min(run + s, MAXU)
        pre.append(run)
    return [min(p, cap) for p in pre], run


def u64(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", (0,) + SIZES)
def test_device_walk_equals_host_walk_and_reference(world, n):
    entries, blob, off = batch_of(world, n)
    info = world.zj.batch.inspect(blob, off)
    raw = u64(info.raw).reshape(n, 5)
    for i, c in enumerate(entries):
        got = (int(raw[i, 0]), int(raw[i, 1]), int(raw[i, 2]), int(raw[i, 3]) & 0xFFFFFFFF, int(raw[i, 3]) >> 32, int(raw[i, 4]) & 0xFFFFFFFF, int(raw[i, 4]) >> 32)
        assert got == c.info, (i, c.name)           # c.info[:4] is the reference's answer (checked in the fixture)
    if n:
        want = np.array([c.info[0] for c in entries], dtype=np.uint64).view(np.int64)
        assert (info.content.cpu().numpy() == want).all()
        assert (info.frames.cpu().numpy() == np.array([c.info[4] for c in entries])).all()
        assert (info.flags.cpu().numpy() == np.array([c.info[6] for c in entries])).all()
        assert (info.dict_id.cpu().numpy() == np.array([c.info[3] for c in entries])).all()


@pytest.mark.parametrize("n", (0,) + SIZES)
def test_offsets_equal_a_prefix_sum(world, n):
    zj = world.zj
    entries, blob, off = batch_of(world, n)
    info = zj.batch.inspect(blob, off)
    for align in (1, 64):
        for slot_max in (0, 1 << 20):
            slots = slots_of(entries, align, slot_max)
            _, needed = prefix_of(slots, MAXU)
            for cap in (MAXU, needed, max(needed - 1, 0), 0):
                dst_off, nd = zj.batch.decompress_offsets(info, cap, align, slot_max)
                want, _ = prefix_of(slots, cap)
                assert int(u64(nd)[0]) == needed, (n, align, slot_max, cap)
                assert [int(x) for x in u64(dst_off)] == want, (n, align, slot_max, cap)
    for bad_align in (3, 0, 1 << 17):
        with pytest.raises(zj.ZstdException) as e:
            zj.batch.decompress_offsets(info, None, bad_align, 0)
        assert e.value.getErrorCode() == 42


@pytest.mark.parametrize("with_dict", (False, True), ids=("plain", "ddict"))
@pytest.mark.parametrize("n", (0,) + SIZES)
def test_sized_decode_is_the_decode_with_the_same_offsets(world, n, with_dict):
    zj, torch = world.zj, world.torch
    entries, blob, off = batch_of(world, n)
    dd = world.ddict if with_dict else None
    slot_max = 4 << 20
    slots = slots_of(entries, 1, slot_max)
    _, needed = prefix_of(slots, MAXU)
    assert needed < 512 << 20
    for cap in sorted({needed, max(needed - 1, 0)}, reverse=True):
        dst = torch.full((max(needed, 1),), 0xCD, dtype=torch.uint8, device="cuda")
        _, dst_off, res, nd = zj.batch.decompress_sized(blob, off, dst[:cap], dictionary=dd, align=1, slot_max=slot_max)
        want_off, _ = prefix_of(slots, cap)
        assert int(u64(nd)[0]) == needed and [int(x) for x in u64(dst_off)] == want_off
        dst2 = torch.full((max(needed, 1),), 0xCD, dtype=torch.uint8, device="cuda")
        res2 = zj.batch.decompress(blob, off, dst2, dst_off, dictionary=dd)
        torch.cuda.synchronize()
        assert torch.equal(res, res2) and torch.equal(dst, dst2)
        r, out = res.cpu().tolist(), dst.cpu().numpy().tobytes()
        short = 0
        for i, c in enumerate(entries):
            have = want_off[i + 1] - want_off[i]
            decodable = c.orig is not None and (with_dict or not c.dict)
            if have == slots[i]:
                if decodable:
                    assert r[i] == len(c.orig) and out[want_off[i]:want_off[i] + r[i]] == c.orig, (i, c.name, r[i])
            elif decodable and not (c.info[6] & ic.NOSIZE):
                assert r[i] == -70, (i, c.name, r[i])
                short += 1
        assert short == (1 if cap < needed and n >= 8 else 0)


def test_sized_decode_with_aligned_slots(world):
    zj, torch = world.zj, world.torch
    entries, blob, off = batch_of(world, 65)
    slots = slots_of(entries, 64, 1 << 20)
    want_off, needed = prefix_of(slots, MAXU)
    dst = torch.empty(needed, dtype=torch.uint8, device="cuda")
    _, dst_off, res, nd = zj.batch.decompress_sized(blob, off, dst, align=64, slot_max=1 << 20)
    assert [int(x) for x in u64(dst_off)] == want_off and all(x % 64 == 0 for x in want_off)
    r, out = res.cpu().tolist(), dst.cpu().numpy().tobytes()
    for i, c in enumerate(entries):
        if c.orig is not None and not c.dict and slots[i] >= len(c.orig):
            assert out[want_off[i]:want_off[i] + r[i]] == c.orig, (i, c.name, r[i])


def test_python_decompress_sized_then_pack(world):
    """a batch mixing frames with and without a content size: the originals come back, packed, with and without a preallocated destination"""
    zj, torch = world.zj, world.torch
    entries = [c for c in world.pool[:40] if c.orig is not None and not c.dict]
    assert any(c.info[6] & ic.NOSIZE for c in entries) and any(not (c.info[6] & ic.NOSIZE) for c in entries) and len(entries) > 12
    blob = torch.frombuffer(bytearray(b"".join(c.data for c in entries)), dtype=torch.uint8).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(c.data) for c in entries]).astype(np.int64)).cuda()
    want = b"".join(c.orig for c in entries)
    dst, dst_off, res, needed = zj.batch.decompress_sized(blob, off)
    assert isinstance(needed, int) and needed == dst.numel() and needed > len(want)          # (bound-sized slots are larger than their content)
    assert res.cpu().tolist() == [len(c.orig) for c in entries]
    packed, packed_off = zj.batch.pack(res, dst, dst_off)
    assert packed.cpu().numpy().tobytes() == want
    given = torch.empty(needed, dtype=torch.uint8, device="cuda")
    dst2, dst_off2, res2, needed2 = zj.batch.decompress_sized(blob, off, given)
    assert dst2 is given and torch.equal(dst_off2, dst_off) and torch.equal(res2, res) and int(needed2.item()) == needed
    packed2, _ = zj.batch.pack(res2, dst2, dst_off2)
    assert packed2.cpu().numpy().tobytes() == want
