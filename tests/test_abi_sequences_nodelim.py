"""CPU (-m "not gpu"): ZJNI_SEQ_NO_DELIMITERS is declared and exported, and the sequence entries accept it — alone and beside the other two bits — where they
refuse every bit they do not know, before any device is asked for."""
import ctypes as C
import os
import re

from conftest import ROOT


def test_no_delimiters_flag_declared_and_exported(zj):
    text = open(os.path.join(ROOT, "include", "zjni_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+ZJNI_SEQ_NO_DELIMITERS\s+16\b", code)
    assert zj.SEQ_NO_DELIMITERS == 16 and zj.batch.SEQ_NO_DELIMITERS == 16
    assert "ZSTD_sf_noBlockDelimiters" in text and "ZJNI_SEQ_NO_DELIMITERS" in text.split("zjni_compress_sequences_batch_device(")[0]
    assert zj.sequences_block_headers(300000, 5, 16) == 3 * (4 + 8) and zj.sequences_block_headers(300000, 5, 8) == 3 * 6


def test_sequence_entries_accept_the_flag_and_refuse_the_next_bit(zj):
    L = zj.lib()
    bad = (1 << 64) - 42
    res = (C.c_size_t * 1)()
    one = C.create_string_buffer(1)
    for flags in (32, 16 | 32, 64, 1 << 30):                                                    # bits the entries do not know
        assert L.zjni_compress_sequences(one, 1, None, 0, None, 0, 3, flags) == bad
        assert L.zjni_compress_sequences_batch(None, None, None, None, None, None, None, 0, 3, flags) == bad
        assert L.zjni_compress_sequences_batch_device(None, None, None, None, None, None, None, 0, 3, flags, None) == bad
    for flags in (16, 16 | 8 | 1):
        # an empty call is served whatever the device; one frame of nothing with no room gets past the flag check: no device (200) on a machine without one,
        # dstSize_tooSmall in the frame's slot with one — never 42
        assert L.zjni_compress_sequences_batch(None, None, None, None, None, None, None, 0, 3, flags) == 0
        assert L.zjni_compress_sequences_batch_device(None, None, None, None, None, None, None, 0, 3, flags, None) == 0
        assert L.zjni_compress_sequences(one, 1, None, 0, None, 0, 3, flags) in ((1 << 64) - 200, (1 << 64) - 70)
        assert L.zjni_compress_sequences(None, 0, None, 0, None, 0, 3, flags) == bad                             # the one-buffer form wants a destination in this mode
        assert L.zjni_compress_sequences_batch(None, None, None, None, None, None, res, 1, 3, flags) == bad      # null arrays are refused as before
        assert L.zjni_compress_sequences(None, 0, None, 0, None, 0, 9, flags) == bad                             # and so is a level the entries do not serve
