"""Device-resident batches: the HBM layout the kernels consume (include/zjni_amd.h).

A batch is one uint8 blob in HBM plus an int64[n+1] offsets tensor (buffer i = blob[off[i]:off[i+1]]).
torch is used only for device memory and the stream handle; all compute is in libzjni_amd.so.
"""
import torch

from . import lib, ZstdException, SEQ_NO_DELIMITERS, sequences_block_headers      # noqa: F401  (SEQ_NO_DELIMITERS: batch.compress_sequences' flag, exported here too)


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _check(r):
    L = lib()
    if L.zjni_isError(r):
        raise ZstdException(r)


def init(device_index=None):
    """Bind the calling thread to a GPU and create its persistent-kernel state."""
    if not torch.cuda.is_available():
        raise ZstdException(200, "zjni: no gfx950 device available")
    if device_index is None:
        device_index = torch.cuda.current_device()
    torch.cuda.set_device(device_index)
    r = lib().zjni_init(device_index)
    if r != 0:
        raise ZstdException(-r, "zjni_init failed")
    return device_index


def uniform_offsets(n, size, device):
    return torch.arange(0, n + 1, dtype=torch.int64, device=device) * size


def synth(n, buf_size, first_index=0, device="cuda"):
    """n mixed-entropy buffers of buf_size bytes generated in HBM."""
    blob = torch.empty(n * buf_size, dtype=torch.uint8, device=device)
    _check(lib().zjni_synth_fill_device(blob.data_ptr(), buf_size, first_index, n, _stream_ptr()))
    return blob


def compress(src_blob, src_off, dst_blob, dst_off, level=3, results=None, checksum=False, dictionary=None, hash_log=0, chain_log=0):
    """Enqueue zjni_compress_batch_device[2 / _usingCDict] on the current stream; returns the int64[n] result tensor
    (compressed size per buffer, or a negative ZSTD/ZJNI error code).  `dictionary`: a ZstdDictCompress (its level applies)."""
    n = src_off.numel() - 1
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    if dictionary is not None:
        _check(lib().zjni_compress_batch_device_usingCDict(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(),
                                                           results.data_ptr(), n, dictionary._ptr, 1 if checksum else 0, _stream_ptr()))
        return results
    if hash_log or chain_log:
        _check(lib().zjni_compress_batch_device_advanced(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(),
                                                         results.data_ptr(), n, level, 1 if checksum else 0, hash_log, chain_log, _stream_ptr()))
        return results
    _check(lib().zjni_compress_batch_device2(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(),
                                             results.data_ptr(), n, level, 1 if checksum else 0, _stream_ptr()))
    return results


def decompress(src_blob, src_off, dst_blob, dst_off, results=None, dictionary=None):
    """Enqueue zjni_decompress_batch_device[_usingDDict] on the current stream; returns int64[n] results."""
    n = src_off.numel() - 1
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    dd = dictionary._ptr if dictionary is not None else None    # a zstd_jni_amd.ZstdDictDecompress
    _check(lib().zjni_decompress_batch_device_usingDDict(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(),
                                                         results.data_ptr(), n, dd, _stream_ptr()))
    return results


class BatchInfo:
    """zjni_frame_info per buffer as tensors: content / bound / first_frame_size int64[n] (-1 unknown, -2 error, a negative ZSTD error code
    for first_frame_size: the values read as signed, as elsewhere), dict_id / frames / skippable / flags int64[n].  `raw` is the
    int64[n, 5] image of the device's zjni_frame_info[n] the fields are views of or made from."""

    def __init__(self, raw):
        self.raw = raw
        self.content, self.bound, self.first_frame_size = raw[:, 0], raw[:, 1], raw[:, 2]
        self.dict_id, self.frames = raw[:, 3] & 0xFFFFFFFF, (raw[:, 3] >> 32) & 0xFFFFFFFF
        self.skippable, self.flags = raw[:, 4] & 0xFFFFFFFF, (raw[:, 4] >> 32) & 0xFFFFFFFF


def inspect(src_blob, src_off):
    """Enqueue zjni_inspect_batch_device on the current stream: what every buffer of concatenated frames decodes to, from its headers
    alone (ZSTD_findDecompressedSize, ZSTD_decompressBound, ZSTD_findFrameCompressedSize, ZSTD_getDictID_fromFrame).  Returns a BatchInfo."""
    n = src_off.numel() - 1
    raw = torch.empty((n, 5), dtype=torch.int64, device=src_blob.device)
    _check(lib().zjni_inspect_batch_device(src_blob.data_ptr(), src_off.data_ptr(), raw.data_ptr(), n, _stream_ptr()))
    return BatchInfo(raw)


def decompress_offsets(info, capacity=None, align=1, slot_max=0, dst_off=None, needed=None):
    """Enqueue zjni_decompress_offsets_device: (dst_off int64[n + 1], needed int64[1]) from a BatchInfo.  capacity None = unlimited."""
    n = info.raw.shape[0]
    if dst_off is None:
        dst_off = torch.empty(n + 1, dtype=torch.int64, device=info.raw.device)
    if needed is None:
        needed = torch.empty(1, dtype=torch.int64, device=info.raw.device)
    cap = (1 << 64) - 1 if capacity is None else capacity
    _check(lib().zjni_decompress_offsets_device(info.raw.data_ptr(), n, cap, align, slot_max, dst_off.data_ptr(), needed.data_ptr(), _stream_ptr()))
    return dst_off, needed


def decompress_sized(src_blob, src_off, dst_blob=None, dictionary=None, align=1, slot_max=0):
    """Decompress a batch whose decoded sizes the caller does not know: returns (dst_blob, dst_off int64[n + 1], results int64[n], needed).
    With a `dst_blob` (uint8) it is one library call (zjni_decompress_batch_device_sized) and nothing synchronises with the host: `needed`
    is an int64[1] tensor, to be compared with dst_blob.numel() when the results are read — buffers that did not fit report -70.
    Without one the batch is inspected, the offsets computed, `needed` read (the only host wait; returned as an int), the blob allocated
    and the existing decompress() called.  Frames without a content size land in slots of their bound; pack(results, dst_blob, dst_off)
    compacts them."""
    n = src_off.numel() - 1
    dev = src_blob.device
    dd = dictionary._ptr if dictionary is not None else None
    if dst_blob is not None:
        if dst_blob.dtype != torch.uint8 or not dst_blob.is_contiguous():
            raise ValueError("decompress_sized: dst_blob must be a contiguous uint8 tensor")
        raw = torch.empty((n, 5), dtype=torch.int64, device=dev)
        dst_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        needed = torch.empty(1, dtype=torch.int64, device=dev)
        results = torch.empty(n, dtype=torch.int64, device=dev)
        _check(lib().zjni_decompress_batch_device_sized(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_blob.numel(), align, slot_max,
                                                        raw.data_ptr(), dst_off.data_ptr(), needed.data_ptr(), results.data_ptr(), n, dd, _stream_ptr()))
        return dst_blob, dst_off, results, needed
    dst_off, needed = decompress_offsets(inspect(src_blob, src_off), None, align, slot_max)
    total = int(needed.item())
    if total < 0:
        raise ZstdException(64, "decompress_sized: the batch declares more than 2^63 bytes; set slot_max")
    dst_blob = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
    results = decompress(src_blob, src_off, dst_blob, dst_off, dictionary=dictionary)
    return dst_blob, dst_off, results, total


def compress_bound_chunked(size, chunk):
    """zjni_compressBound_chunked: the sum of zjni_compressBound over the max(1, ceil(size / chunk)) pieces of a buffer — a slot that always fits."""
    r = lib().zjni_compressBound_chunked(size, chunk)
    _check(r)
    return r


def compress_chunked(src_blob, src_off, dst_blob=None, dst_off=None, level=3, checksum=False, chunk=1 << 16, results=None):
    """Enqueue zjni_compress_chunked_batch_device on the current stream: buffer i becomes max(1, ceil(size / chunk)) independent frames laid end to end
    in its slot — each the frame compress() writes for that piece — which every zstd decoder reads as one buffer; buffers of any size, `chunk` from 256
    to 131072 bytes.  Returns (dst_blob, dst_off int64[n + 1], results int64[n]): results[i] is the total, -70 when it exceeds the slot, or the first
    piece's error.  Without a dst_blob the slots are compress_bound_chunked-sized (src_off is read on the host for that: one wait).  The library itself
    waits once per call for the number of pieces."""
    n = src_off.numel() - 1
    dev = src_blob.device
    if dst_blob is None:
        sizes = (src_off[1:] - src_off[:-1]).clamp(min=0).cpu().tolist()
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + compress_bound_chunked(s, chunk))
        dst_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        dst_blob = torch.empty(max(offs[-1], 1), dtype=torch.uint8, device=dev)[:offs[-1]]
    elif dst_off is None:
        raise ValueError("compress_chunked: a dst_blob needs its dst_off")
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=dev)
    _check(lib().zjni_compress_chunked_batch_device(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(), results.data_ptr(), n,
                                                    level, 1 if checksum else 0, chunk, _stream_ptr()))
    return dst_blob, dst_off, results


def compress_bound_pieces(size, pieces):
    """zjni_compressBound_pieces: size + (size >> 8) + 64 * max(pieces, 1) — a slot that fits any `pieces` pieces of a buffer of `size` bytes."""
    return lib().zjni_compressBound_pieces(size, pieces)


def compress_pieces(src_blob, src_off, dst_blob=None, dst_off=None, level=3, checksum=False, chunk=1 << 16, cuts=None, cut_off=None, dictionary=None, dict_id=True,
                    sizes=False, piece_cap=None, results=None):
    """Enqueue zjni_compress_pieces_batch_device on the current stream: compress_chunked() with three additions.  `cuts` / `cut_off` (int64 tensors; buffer i's cuts
    are cuts[cut_off[i]:cut_off[i + 1]], bytes from its start) put the frame boundaries where the caller's records end instead of on the fixed grid; `chunk` is then
    the largest piece allowed, and a buffer with an illegal list answers -42, writes nothing and owns no entry.  `dictionary` (a ZstdDictCompress; its level applies,
    dict_id=False keeps its ID out of the headers) makes every frame the one compress(dictionary=...) writes for the piece.  sizes=True also returns the index:
    piece_first int64[n + 1] (entries before buffer i; the last is E) and piece_size int64[E] (compressed size of every frame, in order), with which
    decompress() reads single records without walking the buffer.  Returns (dst_blob, dst_off, results[, piece_first, piece_size]).  Without a dst_blob the slots
    are compress_bound_pieces-sized (src_off and cut_off are read on the host for that: one wait).  `piece_cap`: the size of the piece_size tensor (default: the
    number of pieces the lists describe); the call raises ZstdException(70) when E exceeds it."""
    import torch
    n = src_off.numel() - 1
    dev = src_blob.device
    if (cuts is None) != (cut_off is None):
        raise ValueError("compress_pieces: cuts and cut_off go together")
    src_sizes = counts = None
    if dst_blob is None or (sizes and piece_cap is None):
        src_sizes = (src_off[1:] - src_off[:-1]).clamp(min=0).cpu().tolist()
        if cut_off is not None:
            counts = [c + 1 for c in (cut_off[1:] - cut_off[:-1]).clamp(min=0).cpu().tolist()]
        else:
            counts = [max(1, -(-s // chunk)) for s in src_sizes]
    if dst_blob is None:
        offs = [0]
        for s, c in zip(src_sizes, counts):
            offs.append(offs[-1] + compress_bound_pieces(s, c))
        dst_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        dst_blob = torch.empty(max(offs[-1], 1), dtype=torch.uint8, device=dev)[:offs[-1]]
    elif dst_off is None:
        raise ValueError("compress_pieces: a dst_blob needs its dst_off")
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=dev)
    piece_first = piece_size = None
    if sizes:
        if piece_cap is None:
            piece_cap = sum(counts)
        piece_first = torch.empty(n + 1, dtype=torch.int64, device=dev)
        piece_size = torch.empty(max(piece_cap, 1), dtype=torch.int64, device=dev)
    if cuts is not None and cuts.numel() == 0:
        cuts = torch.zeros(1, dtype=torch.int64, device=dev)          # (an empty tensor has no address, and no address means the fixed grid)
    flags = (1 if checksum else 0) | (0 if dict_id else 4)
    _check(lib().zjni_compress_pieces_batch_device(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(), results.data_ptr(), n, level, flags, chunk,
                                                   cuts.data_ptr() if cuts is not None else None, cut_off.data_ptr() if cut_off is not None else None,
                                                   dictionary._ptr if dictionary is not None else None,
                                                   piece_first.data_ptr() if sizes else None, piece_size.data_ptr() if sizes else None, piece_cap if sizes else 0, _stream_ptr()))
    if sizes:
        return dst_blob, dst_off, results, piece_first, piece_size[:int(piece_first[n].item())]
    return dst_blob, dst_off, results


def decompress_frames(src_blob, src_off, dst_blob, dst_off, results=None, dictionary=None):
    """Enqueue zjni_decompress_frames_batch_device on the current stream: decompress() for buffers of MANY concatenated frames (compress_chunked's output,
    pzstd, appended logs).  A buffer of at least two zstd frames that all record their content size is decoded one frame per wave slot instead of frame
    after frame by one wave; any other buffer takes decompress()'s route.  Same arguments, same results, same bytes as decompress().  The library waits
    once per call for the number of frames.  last_frames() says how the last call went."""
    n = src_off.numel() - 1
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    dd = dictionary._ptr if dictionary is not None else None
    _check(lib().zjni_decompress_frames_batch_device(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(),
                                                     results.data_ptr(), n, dd, _stream_ptr()))
    return results


def last_frames():
    """zjni_last_frames (synchronises): {"split": buffers decoded frame by frame, "entries": frames and whole buffers handed to the decoder, "unsplit":
    buffers decoded as one entry, "redo": split buffers decoded again as a whole because one of their frames answered an error} of the last
    decompress_frames() on this device."""
    import ctypes as C
    out = (C.c_uint * 4)()
    r = lib().zjni_last_frames(out)
    if r != 0:
        raise ZstdException(-r, "zjni_last_frames failed")
    return dict(zip(("split", "entries", "unsplit", "redo"), [int(x) for x in out]))


def decompress_frames_range(src_blob, src_off, dst_blob, dst_off, ranges, results=None, totals=None, dictionary=None):
    """Enqueue zjni_decompress_frames_range_batch_device on the current stream: of buffer i (many concatenated frames that all record their content size) decode
    only the frames that hold the decoded bytes [lo_i, lo_i + len_i) and leave exactly those bytes, clamped to the buffer's content, at dst_off[i].  `ranges` is an
    int64[n, 2] (or [2n]) tensor of (lo, len).  Returns (results int64[n], totals int64[n]): the bytes written or a negative error code, and the buffer's whole
    decoded size (-2 when it cannot be indexed).  Damage in frames outside the range is not seen.  The library waits once per call for the entry counts.
    last_frames_range() says how the last call went."""
    n = src_off.numel() - 1
    if ranges.dtype != torch.int64 or not ranges.is_contiguous() or ranges.numel() != 2 * n:
        raise ValueError("decompress_frames_range: ranges must be a contiguous int64 tensor of n (lo, len) pairs")
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    if totals is None:
        totals = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    dd = dictionary._ptr if dictionary is not None else None
    _check(lib().zjni_decompress_frames_range_batch_device(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(), ranges.data_ptr(),
                                                           results.data_ptr(), totals.data_ptr(), n, dd, _stream_ptr()))
    return results, totals


def last_frames_range():
    """zjni_last_frames_range (synchronises): {"served": buffers answered without an error, "frames": frames handed to the decoder, "edges": frames among them
    decoded into scratch because the range cuts them, "errors": buffers that answered an error} of the last decompress_frames_range() on this device."""
    import ctypes as C
    out = (C.c_uint * 4)()
    r = lib().zjni_last_frames_range(out)
    if r != 0:
        raise ZstdException(-r, "zjni_last_frames_range failed")
    return dict(zip(("served", "frames", "edges", "errors"), [int(x) for x in out]))


def index_bytes(n, entries):
    """zjni_index_bytes: the bytes of a prepared index for n buffers and `entries` entries (first[n + 1], valid[n], C[entries + 1], U[entries + 1], all uint64)."""
    return lib().zjni_index_bytes(n, entries)


def _index_tensor(n, entries, device):
    return torch.empty(max(index_bytes(n, entries) // 8, 1), dtype=torch.int64, device=device)


def index_from_sizes(piece_first, piece_size, piece_content, index=None):
    """Enqueue zjni_index_from_sizes_device on the current stream: the prepared index (an int64 tensor; see index_bytes) of n buffers of concatenated frames from
    piece_first int64[n + 1], piece_size int64[E] and piece_content int64[E].  A buffer at which piece_first does not ascend or exceeds E, or with a size above
    2^32 - 1, carries 42 in the index and every read of it answers -42.  No host wait."""
    n, entries = piece_first.numel() - 1, piece_size.numel()
    if piece_content.numel() != entries:
        raise ValueError("index_from_sizes: piece_size and piece_content go together")
    if index is None:
        index = _index_tensor(n, entries, piece_first.device)
    _check(lib().zjni_index_from_sizes_device(n, piece_first.data_ptr(), piece_size.data_ptr() if entries else None, piece_content.data_ptr() if entries else None,
                                              entries, index.data_ptr(), _stream_ptr()))
    return index


def index_from_pieces(src_off, results, piece_first, piece_size, chunk=1 << 16, cuts=None, cut_off=None, index=None):
    """Enqueue zjni_index_from_pieces_device on the current stream: the prepared index of what compress_pieces(sizes=True) returned, from what that call took — the
    UNCOMPRESSED src_off, chunk, cuts / cut_off — and gave: results, piece_first, piece_size.  Content sizes come from the cuts (or the fixed grid); a buffer whose
    result is an error carries that code.  No host wait."""
    n, entries = src_off.numel() - 1, piece_size.numel()
    if (cuts is None) != (cut_off is None):
        raise ValueError("index_from_pieces: cuts and cut_off go together")
    if index is None:
        index = _index_tensor(n, entries, src_off.device)
    if cuts is not None and cuts.numel() == 0:
        cuts = torch.zeros(1, dtype=torch.int64, device=src_off.device)
    _check(lib().zjni_index_from_pieces_device(src_off.data_ptr(), n, chunk, cuts.data_ptr() if cuts is not None else None, cut_off.data_ptr() if cut_off is not None else None,
                                               results.data_ptr() if results is not None else None, piece_first.data_ptr(), piece_size.data_ptr() if entries else None,
                                               entries, index.data_ptr(), _stream_ptr()))
    return index


def index_from_frames(src_blob, src_off, index=None, sizes=False):
    """The prepared index of n buffers of concatenated frames from their bytes alone, for a reader who did not compress them: zjni_index_count_frames_device (a walk
    over the frame headers, one entry a frame), one read of E on the host — the only wait — and zjni_index_from_frames_device (the second walk and the scan), both on
    the current stream.  A buffer the ranged entry would not index (or with a frame whose content size exceeds 2^32 - 1) owns no entry and carries its code: every
    read of it answers that code.  Returns (index, E, piece_first int64[n + 1]); with sizes=True also piece_size int64[E] and piece_content int64[E], the compact
    form to store beside the bytes: index_from_sizes() rebuilds the index from them.  `index`: an int64 tensor of at least index_bytes(n, E) bytes to build into."""
    n = src_off.numel() - 1
    dev = src_blob.device
    piece_first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _check(lib().zjni_index_count_frames_device(src_blob.data_ptr(), src_off.data_ptr(), n, piece_first.data_ptr(), _stream_ptr()))
    entries = int(piece_first[n].item())
    if index is None:
        index = _index_tensor(n, entries, dev)
    elif index.numel() * 8 < index_bytes(n, entries):
        raise ValueError("index_from_frames: the index tensor is smaller than index_bytes(n, E)")
    piece_size = piece_content = None
    if sizes:
        piece_size = torch.empty(max(entries, 1), dtype=torch.int64, device=dev)[:entries]
        piece_content = torch.empty(max(entries, 1), dtype=torch.int64, device=dev)[:entries]
    _check(lib().zjni_index_from_frames_device(src_blob.data_ptr(), src_off.data_ptr(), n, piece_first.data_ptr(), entries, index.data_ptr(),
                                               piece_size.data_ptr() if sizes and entries else None, piece_content.data_ptr() if sizes and entries else None, _stream_ptr()))
    if sizes:
        return index, entries, piece_first, piece_size, piece_content
    return index, entries, piece_first


def decompress_index_range(src_blob, src_off, index, entries, requests, dst_blob, dst_off, results=None, totals=None, dictionary=None):
    """Enqueue zjni_decompress_index_range_batch_device on the current stream: `requests` is an int64[R, 3] (or [3R]) tensor of (buffer, lo, len); request r leaves
    the decoded bytes [lo, lo + len) of that buffer, clamped to its content, at dst_off[r].  The frames are found by bisection in `index` (index_from_sizes /
    index_from_pieces; `entries` = its E): no frame header outside the selection is read, and any number of requests may name one buffer.  Returns (results
    int64[R], totals int64[R]) as decompress_frames_range does.  The library waits once per call for the entry counts.  last_index_range() says how the call went."""
    n = src_off.numel() - 1
    if requests.dtype != torch.int64 or not requests.is_contiguous() or requests.numel() % 3:
        raise ValueError("decompress_index_range: requests must be a contiguous int64 tensor of (buffer, lo, len) triples")
    count = requests.numel() // 3
    if dst_off.numel() != count + 1:
        raise ValueError("decompress_index_range: dst_off needs one slot per request")
    if results is None:
        results = torch.empty(count, dtype=torch.int64, device=src_blob.device)
    if totals is None:
        totals = torch.empty(count, dtype=torch.int64, device=src_blob.device)
    dd = dictionary._ptr if dictionary is not None else None
    _check(lib().zjni_decompress_index_range_batch_device(src_blob.data_ptr(), src_off.data_ptr(), n, index.data_ptr(), entries, requests.data_ptr() if count else None,
                                                          dst_blob.data_ptr(), dst_off.data_ptr(), results.data_ptr() if count else None,
                                                          totals.data_ptr() if count else None, count, dd, _stream_ptr()))
    return results, totals


def last_index_range():
    """zjni_last_index_range (synchronises): {"served": requests answered without an error, "entries": index entries handed to the decoder, "edges": entries among
    them decoded into scratch because the range cuts them, "errors": requests that answered an error} of the last decompress_index_range() on this device."""
    import ctypes as C
    out = (C.c_uint * 4)()
    r = lib().zjni_last_index_range(out)
    if r != 0:
        raise ZstdException(-r, "zjni_last_index_range failed")
    return dict(zip(("served", "entries", "edges", "errors"), [int(x) for x in out]))


def stream_states(n, level, device="cuda"):
    """n compress-stream states of zjni_cstream_state_bytes(level) bytes each, zeroed: streams on which nothing has been done."""
    size = lib().zjni_cstream_state_bytes(level)
    if not size:
        raise ZstdException(42, "compress streams are not served at level %d" % level)
    return torch.zeros(n * size, dtype=torch.uint8, device=device)


def compress_stream_continue(src_blob, src_off, dst_blob, dst_off, states, level=3, checksum=False, flush_at=None, flush_off=None, mode=None, results=None):
    """Enqueue zjni_compress_stream_continue_batch_device on the current stream: src slot i holds everything written to stream i so far, dst slot i
    receives the frame's NEW bytes only, results[i] is their count (0: nothing flushed since the last call) or a negative error code.
    flush_at uint32 / flush_off int64[n + 1]: the flush positions of stream i (all of them or only the new ones); mode uint32[n]: 1 = close,
    | 2 = closed before anything else, | 4 = continue: a call that does not close also compresses every full 128 KiB piece behind the newest
    flush (None: all close)."""
    n = src_off.numel() - 1
    if results is None:
        results = torch.empty(n, dtype=torch.int64, device=src_blob.device)
    if states.dtype != torch.uint8 or not states.is_contiguous() or states.numel() < n * lib().zjni_cstream_state_bytes(level):
        raise ValueError("compress_stream_continue: states must be stream_states(n, level)")
    ptr = lambda t: t.data_ptr() if t is not None else None
    _check(lib().zjni_compress_stream_continue_batch_device(src_blob.data_ptr(), src_off.data_ptr(), dst_blob.data_ptr(), dst_off.data_ptr(), results.data_ptr(), n, level,
                                                            1 if checksum else 0, ptr(flush_at), ptr(flush_off), ptr(mode), states.data_ptr(), _stream_ptr()))
    return results


def stream_state_info(states, level):
    """The header words of every state (zj_encode.h ZEStreamState) as int64[n] tensors: consumed (source bytes compressed so far), produced (frame bytes
    written so far), parsed / blocks (sums over the blocks handed to the block compressor: their sizes, their count), closed, error."""
    size = lib().zjni_cstream_state_bytes(level)
    words = states.view(torch.int32).view(-1, size // 4)[:, :16].to(torch.int64)
    return {"error": words[:, 3], "closed": words[:, 4], "consumed": words[:, 5], "produced": words[:, 6], "parsed": words[:, 9], "blocks": words[:, 10]}


def pack(results, dst_blob, dst_off, out=None, out_off=None):
    """Tightly pack a compress batch's variable-size outputs (sizes = results) into one blob:
    returns (packed_blob, packed_off int64[n+1]).  With `out` (uint8, capacity >= sum of sizes) and `out_off`
    (int64[n+1]) preallocated the exclusive scan and the byte movement are one library call
    (zjni_pack_batch_device2) and nothing synchronises with the host; without `out` the scan is torch's,
    because the blob's size has to come back first."""
    n = results.numel()
    if out_off is None:
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=results.device)
    if out is not None and out_off.is_contiguous() and results.is_contiguous():
        if out_off.numel() != n + 1 or out_off.dtype != torch.int64 or out.dtype != torch.uint8 or results.dtype != torch.int64:
            raise ValueError("pack: out_off must be int64[n + 1], out uint8, results int64[n]")      # (the device writes n + 1 offsets: nothing else checks them)
        _check(lib().zjni_pack_batch_device2(dst_blob.data_ptr(), dst_off.data_ptr(), results.data_ptr(), out.data_ptr(),
                                             out_off.data_ptr(), n, _stream_ptr()))
        return out, out_off
    sizes = results.clamp(min=0)
    out_off[0] = 0
    torch.cumsum(sizes, 0, out=out_off[1:])
    if out is None:
        total = int(out_off[-1].item())
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=results.device)[:total]
    _check(lib().zjni_pack_batch_device(dst_blob.data_ptr(), dst_off.data_ptr(), sizes.data_ptr(), out.data_ptr(),
                                        out_off.data_ptr(), n, _stream_ptr()))
    return out, out_off


def compress_sequences(src, src_off, seqs, seq_off, level, flags=0, dst=None, dst_off=None, results=None, _grid=0):
    """Enqueue zjni_compress_sequences_batch_device on the current stream: frames from the CALLER's sequences (ZSTD_compressSequences with explicit
    block delimiters).  src uint8 blob and src_off int64[n + 1] as everywhere; seqs an int32 / uint32 [k, 4] device tensor of ZSTD_Sequence rows
    {offset, litLength, matchLength, rep}, seq_off int64[n + 1] counting rows.  flags: 1 checksum, 8 ZJNI_SEQ_REPCODES, 16 ZJNI_SEQ_NO_DELIMITERS (the
    array has no delimiters and the library cuts the blocks, ZSTD_sf_noBlockDelimiters).  Without dst / dst_off the destinations are sized here (compress
    bound plus a block header per sequence row — per block the library may cut without delimiters — which reads src_off and seq_off back).  Returns
    (dst, dst_off, results int64[n]): the frame's size, or a negative ZSTD / ZJNI error code (107: the frame's sequences are invalid).
    _grid: tests only, at most that many workgroups."""
    n = src_off.numel() - 1
    dev = src.device
    if seqs.element_size() != 4 or not seqs.is_contiguous():
        raise ValueError("compress_sequences: seqs must be a contiguous tensor of 32-bit rows")
    if dst is None:
        so, qo = src_off.cpu().tolist(), seq_off.cpu().tolist()
        caps = [0]
        for i in range(n):
            size = max(so[i + 1] - so[i], 0)
            caps.append(caps[-1] + lib().zjni_compressBound(size) + 64 + sequences_block_headers(size, max(qo[i + 1] - qo[i], 0), flags))
        dst = torch.empty(max(caps[-1], 1), dtype=torch.uint8, device=dev)
        dst_off = torch.tensor(caps, dtype=torch.int64, device=dev)
    if results is None:
        results = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    prev = lib().zjni_debug_sequences_grid(_grid) if _grid else 0
    try:
        _check(lib().zjni_compress_sequences_batch_device(src.data_ptr(), src_off.data_ptr(), seqs.data_ptr(), seq_off.data_ptr(), dst.data_ptr(), dst_off.data_ptr(),
                                                          results.data_ptr(), n, level, flags, _stream_ptr()))
    finally:
        if _grid:
            lib().zjni_debug_sequences_grid(prev)
    return dst, dst_off, results


def generate_sequences(src, src_off, level, seqs=None, seq_off=None, _grid=0):
    """Enqueue zjni_generate_sequences_batch_device on the current stream: the matchers' parse of every frame as ZSTD_Sequence rows {offset, litLength,
    matchLength, rep} with explicit block delimiters (ZSTD_generateSequences).  src uint8 blob and src_off int64[n + 1] as everywhere; seqs an int32 / uint32
    [k, 4] device tensor of slots and seq_off int64[n + 1] counting rows — without them the slots are sized here by sequence_bound (which reads src_off back).
    Returns (seqs, seq_off, results int64[n]): the rows written into the frame's slots, delimiters included, or a negative error code (106: a last block under
    7 bytes; 70: the slots are too few; 201: not served).  _grid: tests only, at most that many workgroups."""
    n = src_off.numel() - 1
    dev = src.device
    if seqs is None:
        so = src_off.cpu().tolist()
        rows = [0]
        for i in range(n):
            rows.append(rows[-1] + lib().zjni_sequenceBound(max(so[i + 1] - so[i], 0)))
        seqs = torch.empty((max(rows[-1], 1), 4), dtype=torch.int32, device=dev)
        seq_off = torch.tensor(rows, dtype=torch.int64, device=dev)
    if seqs.element_size() != 4 or not seqs.is_contiguous():
        raise ValueError("generate_sequences: seqs must be a contiguous tensor of 32-bit rows")
    results = torch.empty(max(n, 1), dtype=torch.int64, device=dev)[:n]
    prev = lib().zjni_debug_generate_grid(_grid) if _grid else 0
    try:
        _check(lib().zjni_generate_sequences_batch_device(src.data_ptr(), src_off.data_ptr(), seqs.data_ptr(), seq_off.data_ptr(), results.data_ptr(), n, level, 0, _stream_ptr()))
    finally:
        if _grid:
            lib().zjni_debug_generate_grid(prev)
    return seqs, seq_off, results


def last_generate():
    """zjni_last_generate (synchronises): {"lane": frames the last generate_sequences() sent through a lane route (none yet: 0), "wave": frames it sent
    through the wave-per-frame kernel, "refused": frames that answered an error code}."""
    import ctypes as C
    out = (C.c_uint * 4)()
    r = lib().zjni_last_generate(out)
    if r != 0:
        raise ZstdException(-r, "zjni_last_generate failed")
    return dict(zip(("lane", "wave", "refused"), [int(x) for x in out[:3]]))


def _test_compress_records(datas, records, level, checksum=False, staged_lds=False, grid=0):
    """TEST ENTRY (zjni_test_compress_records_batch_device): the entropy stage on sequences the caller wrote.  datas: the sources (bytes, one block each);
    records[i] = (flat [ll, ml, offBase, pos] * nbSeq, litSize, lastLL) for source i.  staged_lds: the dynamic LDS of the dictionary pipeline's entropy launch
    (frames to 4 KiB staged in LDS) instead of the plain one; grid: at most that many workgroups.  Returns a list of frames (bytes) or negative error codes."""
    import ctypes as C
    n = len(datas)
    for data, (rec, _, _) in zip(datas, records):                      # what the entry itself does not refuse: sizes the level's frames never have, offsets that reach in front of the source
        if len(data) > (131072 if level <= 4 else 16384):
            raise ValueError("_test_compress_records: levels 5 to 8 serve frames to 16 KiB, the others to 128 KiB")
        for q in range(0, len(rec), 4):
            if rec[q + 2] > rec[q + 3] + rec[q] + 3:
                raise ValueError("_test_compress_records: an offset beyond the start of the source")
    offs, rec_off, flat, meta = [0], [0], [], []
    for data, (rec, lit_size, last_ll) in zip(datas, records):
        offs.append(offs[-1] + len(data))
        rec_off.append(rec_off[-1] + len(rec) // 4)
        flat += rec
        meta += [len(rec) // 4, lit_size, last_ll]
    dev = "cuda"
    src = torch.frombuffer(bytearray(b"".join(datas) or b"\0"), dtype=torch.uint8).to(dev)
    src_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    caps = [0]
    for data in datas:
        caps.append(caps[-1] + lib().zjni_compressBound(len(data)) + 64)
    dst = torch.zeros(caps[-1], dtype=torch.uint8, device=dev)
    dst_off = torch.tensor(caps, dtype=torch.int64, device=dev)
    results = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    h_rec = (C.c_uint32 * max(len(flat), 1))(*flat)
    h_off = (C.c_uint64 * (n + 1))(*rec_off)
    h_meta = (C.c_uint32 * max(len(meta), 1))(*meta)
    _check(lib().zjni_test_compress_records_batch_device(src.data_ptr(), src_off.data_ptr(), C.addressof(h_rec), C.addressof(h_off), C.addressof(h_meta), dst.data_ptr(),
                                                         dst_off.data_ptr(), results.data_ptr(), n, level, 1 if checksum else 0, 1 if staged_lds else 0, grid, _stream_ptr()))
    res = results.cpu().tolist()
    out = dst.cpu().numpy().tobytes()
    return [out[caps[i]:caps[i] + res[i]] if res[i] >= 0 else res[i] for i in range(n)]


def last_timing():
    """ms of the stages of the last large-batch device calls (HIP events on the launch stream, see zjni_last_timing2):
    {"match": .., "dec_prep": .., "dec_seq": .., "dec_exec": .., "dec_fused": .., "match_wide": ..}; -1 where a stage did not run."""
    import ctypes as C
    out = (C.c_float * 8)()
    _check(lib().zjni_last_timing2(out))
    return dict(zip(("match", "dec_prep", "dec_seq", "dec_exec", "dec_fused", "match_wide"), [float(x) for x in out][:6]))
