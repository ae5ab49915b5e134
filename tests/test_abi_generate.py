"""CPU (-m "not gpu"): the generate entries of include/zjni_amd.h are declared, exported and bound, zjni_mergeBlockDelimiters is the reference's
ZSTD_mergeBlockDelimiters, and the entries refuse what they can refuse without a device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

NAMES = ("zjni_generate_sequences_batch_device", "zjni_generate_sequences_batch", "zjni_generate_sequences", "zjni_mergeBlockDelimiters", "zjni_last_generate",
         "zjni_debug_generate_grid")


def test_generate_symbols_declared_and_exported(zj):
    text = open(os.path.join(ROOT, "include", "zjni_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = zj.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/zjni_amd.h"
        assert hasattr(L, name) and name in zj.EXPORTS, name
    assert len(L.zjni_generate_sequences_batch_device.argtypes) == 9 and len(L.zjni_generate_sequences_batch.argtypes) == 8
    assert callable(zj.generate_sequences) and callable(zj.merge_block_delimiters) and callable(zj.batch.generate_sequences) and callable(zj.batch.last_generate)


def test_merge_block_delimiters_is_the_references(zj, oracle_ref):
    R = oracle_ref.lib()
    R.ZSTD_mergeBlockDelimiters.restype = C.c_size_t
    R.ZSTD_mergeBlockDelimiters.argtypes = [C.c_void_p, C.c_size_t]
    for seqs in ([(5, 3, 4, 0), (9, 0, 7, 1), (0, 9, 0, 0)],                                             # a trailing delimiter
                 [(5, 3, 4, 0), (0, 2, 0, 0), (0, 7, 0, 0), (9, 1, 6, 1), (0, 0, 0, 0)],                 # two adjacent delimiters
                 [(5, 3, 4, 0), (7, 0, 5, 2)],                                                           # no delimiter
                 [(0, 4, 0, 0)], []):
        mine = zj.merge_block_delimiters(seqs)
        theirs = np.array(seqs, dtype=np.uint32).reshape(-1, 4).copy()
        n = R.ZSTD_mergeBlockDelimiters(theirs.ctypes.data if len(theirs) else None, len(theirs))
        assert len(mine) == n and (mine == theirs[:n]).all(), seqs
    assert zj.lib().zjni_mergeBlockDelimiters(None, 0) == 0


def test_generate_entries_refuse_bad_arguments_before_any_device(zj):
    L = zj.lib()
    bad = (1 << 64) - 42
    res = (C.c_size_t * 1)()
    assert L.zjni_generate_sequences_batch_device(None, None, None, None, None, 1, 3, 1, None) == bad          # a flags bit: none is defined
    assert L.zjni_generate_sequences_batch_device(None, None, None, None, None, 1, 9, 0, None) == bad          # a level the batch entries do not serve
    assert L.zjni_generate_sequences_batch_device(None, None, None, None, None, (1 << 32) + 1, 3, 0, None) == (1 << 64) - 72
    assert L.zjni_generate_sequences_batch_device(None, None, None, None, None, 0, -5, 0, None) == 0
    assert L.zjni_generate_sequences_batch_device(None, None, None, None, None, 3, 3, 0, None) == bad
    assert L.zjni_generate_sequences_batch(None, None, None, None, res, 1, 3, 8) == bad
    assert L.zjni_generate_sequences_batch(None, None, None, None, res, 1, 9, 0) == bad
    assert L.zjni_generate_sequences_batch(None, None, None, None, res, (1 << 32) + 1, 3, 0) == (1 << 64) - 72
    assert L.zjni_generate_sequences_batch(None, None, None, None, None, 0, 3, 0) == 0
    assert L.zjni_generate_sequences_batch(None, None, None, None, res, 1, 3, 0) == bad
    assert L.zjni_generate_sequences(None, 0, None, 0, 9) == bad
    assert L.zjni_debug_generate_grid(0) == 0
