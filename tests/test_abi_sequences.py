"""CPU (-m "not gpu"): the sequence entries of include/zjni_amd.h are declared, exported and bound, zjni_sequenceBound is the reference's
ZSTD_sequenceBound, zjni_sequence is ZSTD_Sequence, and the entries refuse what they can refuse without a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("zjni_sequenceBound", "zjni_compress_sequences_batch_device", "zjni_compress_sequences_batch", "zjni_compress_sequences", "zjni_debug_sequences_grid")


def test_sequence_symbols_declared_and_exported(zj):
    text = open(os.path.join(ROOT, "include", "zjni_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = zj.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/zjni_amd.h"
        assert hasattr(L, name) and name in zj.EXPORTS, name
    assert re.search(r"#define\s+ZJNI_SEQ_REPCODES\s+8\b", code) and zj.SEQ_REPCODES == 8
    assert re.search(r"typedef struct zjni_sequence \{ uint32_t offset, litLength, matchLength, rep; \} zjni_sequence;", code)
    assert L.zjni_compress_sequences_batch_device.argtypes is not None and len(L.zjni_compress_sequences_batch_device.argtypes) == 11


def test_sequence_bound_is_the_references(zj, oracle_ref):
    R = oracle_ref.lib()
    R.ZSTD_sequenceBound.restype = C.c_size_t
    R.ZSTD_sequenceBound.argtypes = [C.c_size_t]
    for n in (0, 1, 2, 3, 1023, 1024, 131071, 131072, 2 << 20, (2 << 20) + 1):
        assert zj.sequence_bound(n) == R.ZSTD_sequenceBound(n), n


def test_sequence_entries_refuse_bad_arguments_before_any_device(zj):
    L = zj.lib()
    bad = (1 << 64) - 42
    res = (C.c_size_t * 1)()
    assert L.zjni_compress_sequences(None, 0, None, 0, None, 0, 3, 16) == bad                   # a flag bit the entries do not know
    assert L.zjni_compress_sequences(None, 0, None, 0, None, 0, 9, 0) == bad                    # a level the batch entries do not serve
    assert L.zjni_compress_sequences_batch(None, None, None, None, None, None, res, 1, 3, 0) == bad
    assert L.zjni_compress_sequences_batch(None, None, None, None, None, None, None, 0, 3, 0) == 0
    assert L.zjni_compress_sequences_batch_device(None, None, None, None, None, None, None, 0, 3, 1 | 8, None) == 0
    assert L.zjni_compress_sequences_batch_device(None, None, None, None, None, None, None, 1, 3, 2, None) == bad
    assert L.zjni_debug_sequences_grid(0) == 0
