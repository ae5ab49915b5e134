"""CPU (-m "not gpu"): the inputs of tests/branch_cases.py — each exists for one line of the device headers that nothing else executes — through the lane-serial
builds, byte for byte against the reference.  tests/test_emu_reached.py asserts from line counts that they still reach their lines; the -m gpu twin is
tests/test_gpu_branches.py."""
import pytest

import branch_cases as B
from util import emu_lib, emu_compress, emu_compress_multi, emu_decompress, emu_decompress_split

from test_emu_negative_levels import emu as fast_emu, fast_compress          # noqa: F401 (the fixture of the negative levels' library)


@pytest.fixture(scope="module")
def emu():
    return emu_lib()


@pytest.mark.parametrize("name,data", B.backward_inputs(), ids=[n for n, _ in B.backward_inputs()])
def test_backward_extensions_are_the_references(emu, fast_emu, oracle_ref, name, data):
    """levels 1 and 3 (fast and double-fast on the wave matcher, and level 3's lane routes for frames to 64 KiB), level 4 above 16 KiB (double-fast, tables in
    global memory), -5 (the fast loop with a stride of 6)"""
    for level in (1, 3, 4):
        if level == 4 and len(data) > 131072:
            continue                                               # (level 4 is served to 128 KiB)
        want = oracle_ref.compress(data, level)
        if level == 3 or not name.startswith("second-block/"):     # (the fast levels' tables have lost the first block's entries by then: their frames are compared all the same)
            assert len(want) < len(data) - 1000, (name, level, "the copy was not found")
        assert emu_compress_multi(emu, data, level) == want, (name, level, "wave")
        if level <= 3:
            assert emu_compress_multi(emu, data, level, serial=True) == want, (name, level, "serial")
            if len(data) > 131072:                                 # the pipelined route's parse role, on the wave and on the one-lane parse (the library's ZJNI_MULTI_WAVE=0)
                assert emu_compress_multi(emu, data, level, pipelined=True) == want, (name, level, "pipelined")
                assert emu_compress_multi(emu, data, level, pipelined=True, serial=True) == want, (name, level, "pipelined, serial")
        if len(data) <= 65536 and level == 3:
            for split in (False, True):
                assert emu_compress(emu, data, level, split=split) == want, (name, level, split)
    for route in (0, 1):
        assert fast_compress(fast_emu, data, -5, route) == oracle_ref.compress(data, -5), (name, -5, route)


@pytest.mark.parametrize("mode", ["", "1", "2", "5", "6", "7", "8"])
def test_backward_extensions_on_the_lane_machines(emu, oracle_ref, monkeypatch, mode):
    """the lane-per-frame machines of level 3 (zj_match_lane.h: plain and need-gated; zj_match_run.h: the run machine with flags, without, taken over late), whose
    backward extension goes on for as long as eight more bytes are equal; levels 1 and 2 on the plain machine"""
    if mode:
        monkeypatch.setenv("ZJNI_EMU_NEED", mode)
    for name, data in B.backward_inputs():
        if len(data) > 131072:
            continue
        for level in (3,) if mode else (1, 2, 3):
            assert emu_compress(emu, data, level, split=True) == oracle_ref.compress(data, level), (name, level, mode)


def test_decoder_frames_answer_like_the_reference(emu, oracle_ref):
    """the fused decoder and both split pipelines (single-block frames, block stages) on branch_cases.decoder_frames: the reference's content, or its refusal"""
    import ctypes as C
    import os
    if not os.path.exists(oracle_ref.PORTABLE_PATH):
        pytest.skip("oracle/_ref/libzstd_ref_portable.so not built")
    emu.emu_decompress_mb.restype = C.c_ulonglong
    emu.emu_decompress_mb.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_ulonglong, C.POINTER(C.c_int)]
    codes = {"Data corruption detected": 20, "Destination buffer is too small": 70}
    answers = set()
    for name, _, z, cap in B.decoder_frames():
        try:
            want = oracle_ref.decompress_portable(z, cap)
        except oracle_ref.ZstdRefError as e:
            want = -codes[str(e)]
        dst = C.create_string_buffer(max(cap, 1))
        r = emu.emu_decompress_mb(z, len(z), dst, cap, C.byref(C.c_int(0)))
        for how, got in (("fused", emu_decompress(emu, z, cap)), ("split", emu_decompress_split(emu, z, cap)[0]), ("blocks", dst.raw[:r] if r < (1 << 63) else -((1 << 64) - r))):
            assert got == want, (name, how, got if isinstance(got, int) else len(got))
        answers.add(want if isinstance(want, int) else "content")
    assert answers == {"content", -20, -70}
