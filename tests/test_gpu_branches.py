"""GPU (-m gpu): the inputs of tests/branch_cases.py on the wave64 code — each exists for one line of the device headers that nothing else executes (see
tests/test_emu_branches.py, the CPU twin, and tests/test_emu_reached.py, which keeps the lines reached).  Every frame must be the reference's, byte for byte,
and decode on the GPU to its input."""
import pytest

import branch_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def check(gpu, ref, items, level, tag):
    outs = gpu.compress_batch([d for _, d in items], level)
    for (name, d), z in zip(items, outs):
        assert not isinstance(z, Exception), (name, level, tag, z)
        assert z == ref.compress(d, level), (name, level, tag, len(z))
    assert gpu.decompress_batch(outs, [len(d) for _, d in items]) == [d for _, d in items], (level, tag)


@pytest.mark.parametrize("level", (1, 3, 4, -5))
def test_gpu_backward_extensions_on_the_wave_matcher(gpu, oracle_ref, level):
    """a small batch takes the wave route: fast (1, -5) and double-fast (3; 4 with its tables in global memory) extend a match found thousands of bytes into a copy
    of noise backwards over all of them — count_back's second and later trips — to a mismatch, to the frame's first byte, to the anchor, to the block's first byte"""
    items = [(n, d) for n, d in B.backward_inputs() if level != 4 or len(d) <= 131072]
    assert len(items) >= 5
    check(gpu, oracle_ref, items, level, "wave")


def test_gpu_long_backward_extensions_on_the_lds_wave_matcher(gpu, oracle_ref):
    """branch_cases.lds_wave_backward_inputs (the CPU twin: tests/test_emu_wave.py): level 3 with hashLog 14 / chainLog 13 in a small batch is ZJNI_ROUTE_WAVE, whose
    count_back goes round two, three and four times over these frames"""
    items = B.lds_wave_backward_inputs()
    outs = gpu.compress_batch([d for _, d, _ in items], 3, hash_log=14, chain_log=13)
    assert gpu.lib().zjni_last_route() == 2                        # ZJNI_ROUTE_WAVE
    for (name, d, _), z in zip(items, outs):
        assert not isinstance(z, Exception), (name, z)
        assert z == oracle_ref.compress(d, 3, False, 14, 13), (name, len(z))
    assert gpu.decompress_batch(outs, [len(d) for _, d, _ in items]) == [d for _, d, _ in items]


@pytest.mark.parametrize("need", ("0", "1", "2"))
def test_gpu_backward_extensions_on_the_lane_pipeline(gpu, oracle_ref, monkeypatch, need):
    """the lane-per-frame match kernels (the run machine at level 3 with flags for no frame, every frame, the picked frames; the lane machine at levels 1 and 2):
    the backward state goes on for as long as eight more bytes are equal"""
    monkeypatch.setenv("ZJNI_SPLIT_MIN", "1")
    monkeypatch.setenv("ZJNI_NEED", need)
    items = [(n, d) for n, d in B.backward_inputs() if len(d) <= 131072]
    for level in (3,) if need != "0" else (1, 2, 3):
        check(gpu, oracle_ref, items * 3, level, "lane/" + need)


@pytest.mark.parametrize("split_min", ["1", "1000000000"])
def test_gpu_decoder_frames_answer_like_the_reference(gpu, oracle_ref, monkeypatch, split_min):
    """branch_cases.decoder_frames through the three-stage pipeline and the fused kernel: the reference's content, or its refusal's code"""
    import os
    if not os.path.exists(oracle_ref.PORTABLE_PATH):
        pytest.skip("oracle/_ref/libzstd_ref_portable.so not built")
    monkeypatch.setenv("ZJNI_DSPLIT_MIN", split_min)
    cases = B.decoder_frames() * 3
    outs = gpu.decompress_batch([z for _, _, z, _ in cases], [cap for _, _, _, cap in cases])
    codes = {"Data corruption detected": 20, "Destination buffer is too small": 70}
    for (name, _, z, cap), o in zip(cases, outs):
        try:
            want = oracle_ref.decompress_portable(z, cap)
        except oracle_ref.ZstdRefError as e:
            want = -codes[str(e)]
        got = -abs(o.getErrorCode()) if isinstance(o, Exception) else o
        assert got == want, (name, split_min, got if isinstance(got, int) else len(got))
