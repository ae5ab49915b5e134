"""GPU (-m gpu): the encoder's entropy stage on hand-written sequences (tests/seqrecords.py; the conditions on the inputs are asserted in
tests/test_emu_seqrecords.py) through zjni_test_compress_records_batch_device: zj_encode_kernel in mode 0 with the records placed in its frame
slots, with the dynamic LDS of both of the product's entropy launches (the stage alone; with frames to 4 KiB staged in LDS).  This is where the
wave64 code meets them — the 2 x 64-record gather and its ballot loop, LDS histograms, the Huffman build and the tANS tables by the wave, the
parallel stream packing.  Every frame must be the reference's (seqframes.build: ZSTD_compressSequences on the same triples), byte for byte, and
decode under the reference to its content.  Every batch mixes all families, so that different workgroups meet different paths in one launch;
one batch runs on a single workgroup, which then meets a frame of every kind right behind a large one: nothing may leak from frame to frame."""
import random

import pytest

import seqrecords as R

pytestmark = pytest.mark.gpu

ALONE = ("count32511", "count32512")           # the suite's largest blocks: a call of their own per level


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def run(gpu, ref, cases, level, **kw):
    built = [R.built(c, level) for c in cases]
    got = gpu.batch._test_compress_records([b.content for b in built], [(b.rec, b.lit_size, b.last_ll) for b in built], level, **kw)
    bad = [(c.family, c.name, R.explain(g, b.frame)) for c, b, g in zip(cases, built, got) if g != b.frame]
    assert not bad, (level, kw, len(bad), bad[:4])
    for c, b, g in zip(cases, built, got):
        assert ref.decompress(g, len(b.content)) == b.content, (c.family, c.name, level)
    return built


def mixed(level, alone=False):
    cases = [c for c in R.all_cases() if level in R.levels_of(c) and (c.name in ALONE) == alone]
    random.Random(level).shuffle(cases)
    return cases


@pytest.mark.parametrize("staged", (False, True))
@pytest.mark.parametrize("level", (1, 3, 4, 5))
def test_gpu_every_family_is_the_references_frame(gpu, oracle_ref, level, staged):
    cases = mixed(level)
    built = run(gpu, oracle_ref, cases, level, staged_lds=staged)
    assert {c.family for c in cases} == set(R.FAMILIES) - ({"U"} if level > 3 else set())       # (family U's blocks are all above 16 KiB)
    if level <= 3:
        assert sum(len(b.content) > 65536 for b in built) >= 20 and sum(len(b.content) <= 4096 for b in built) >= 100      # both launches, both sides of the staged path's edge


@pytest.mark.parametrize("level", (1, 3))
def test_gpu_largest_sequence_counts(gpu, oracle_ref, level):
    for c in mixed(level, alone=True):
        run(gpu, oracle_ref, [c], level)
        run(gpu, oracle_ref, [c], level, staged_lds=True)


@pytest.mark.parametrize("staged", (False, True))
def test_gpu_one_workgroup_meets_every_frame_in_turn(gpu, oracle_ref, staged):
    """129 frames on ONE workgroup: its LDS, its uniforms and its scratch slot outlive every frame, and a frame of at most 4 KiB follows one of 64 KiB (or, in the
    wide launch, one of 128 KiB follows another) — a stage that relies on what the previous frame left fails here"""
    every = [c for c in R.all_cases() if c.name not in ALONE]
    rnd = random.Random(129)
    small = [c for c in every if R.size_of(c) <= 4096]
    large = [c for c in every if 30000 <= R.size_of(c) <= 65536]
    wide = [c for c in every if R.size_of(c) > 65536]
    assert len(large) >= 8 and len(wide) >= 8
    rnd.shuffle(small)
    cases = []
    for i in range(43):
        cases += [large[i % len(large)], small[2 * i], small[2 * i + 1]]
    names = set()
    cases = [c for c in cases if (c.family, c.name) not in names and not names.add((c.family, c.name))]
    cases += rnd.sample(wide, 8)
    cases += [c for c in small[86:] if (c.family, c.name) not in names][:129 - len(cases)]
    assert len(cases) == 129 and len({c.family for c in cases}) >= 6
    run(gpu, oracle_ref, cases, 3, staged_lds=staged, grid=1)


def test_gpu_refuses_records_that_do_not_tile_their_source(gpu):
    data = b"abcdefgh" * 8
    for rec, lit, last in (([4, 4, 5, 0], 61, 56), ([4, 4, 5, 0], 60, 57), ([4, 2, 5, 0], 62, 58), ([4, 4, 5, 1], 60, 56), ([60, 8, 5, 0], 60, 0)):
        with pytest.raises(gpu.ZstdException):
            gpu.batch._test_compress_records([data], [(rec, lit, last)], 3)
    assert gpu.batch._test_compress_records([data], [([4, 4, 5, 0], 60, 56)], 3)[0][:4] == b"\x28\xb5\x2f\xfd"
