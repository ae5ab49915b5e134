/* zjni_amd.h — C-ABI of the MI355X-native zstd path for zstd-jni (libzjni_amd.so).
 *
 * Boundary: these entry points are what the reference's JNI glue
 * (/root/reference/src/main/native/jni_fast_zstd.c, jni_zstd.c; "N/" below) would bind instead of
 * calling libzstd's ZSTD_compress2 / ZSTD_decompressDCtx for batches of independent buffers.
 * Plain pointers and sizes only; no torch / HIP types in any signature (streams are passed as void*).
 *
 * Result convention everywhere = the reference's: a size_t byte count, or (size_t)(0 - code) with
 * `code` a ZSTD_ErrorCode (N/zstd_errors.h:60-98); test with zjni_isError (== N/jni_zstd.c:240-243
 * Zstd.isError) and map with zjni_getErrorCode / zjni_getErrorName (== Zstd.getErrorCode /
 * getErrorName, N/jni_zstd.c:252-267).
 *
 * The library REQUIRES a gfx950 device: every compute entry returns ZJNI_ERROR(no_device) (code 200,
 * outside libzstd's range) when HIP finds none.  There is no CPU fallback inside this library; the
 * JNI glue keeps libzstd for what the GPU path does not cover.
 */
#ifndef ZJNI_AMD_H
#define ZJNI_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZJNI_VERSION_STRING "0.1.0-zstd1.5.7"
#define ZJNI_ERROR_no_device 200u      /* no HIP device / kernel launch failure */
#define ZJNI_ERROR_unsupported 201u    /* input outside the GPU path's scope (see zjni_compress_batch) */
#define ZJNI_BLOCKSIZE_MAX (1u << 17)  /* ZSTD_BLOCKSIZE_MAX, N/zstd.h:147-148: inputs up to here become single-block frames */
#define ZJNI_FRAME_MAX (2u << 20)      /* largest input the compress entries take: multi-block frames (N/compress/zstd_compress.c:4591-4692),
                                        * byte-identical to ZSTD_compress2 with the level's own parameters, as long as the frame fits the level's
                                        * window — 512 KiB / 1 MiB / 2 MiB at levels 1 / 2 / 3, 512 KiB at negative levels; beyond that ZJNI_ERROR_unsupported */
#define ZJNI_LEVEL4_MAX (1u << 17)     /* level 4 (N/compress/clevels.h:84,110): greedy on the hash chain up to 16 KiB (ZSTD_compressBlock_greedy,
                                        * N/compress/zstd_lazy.c:1784), double-fast with 2^17-entry tables up to here; larger inputs run the
                                        * reference's row-based match finder, which this library does not restate: ZJNI_ERROR_unsupported */
#define ZJNI_LAZY_MAX (1u << 17)       /* levels 5-8 (N/compress/clevels.h:85-88,111-114): greedy / lazy / lazy2 (ZSTD_compressBlock_lazy_generic,
                                        * N/compress/zstd_lazy.c:1516-1780) on the hash chain for inputs up to 16 KiB and on the row-based finder
                                        * (ZSTD_RowFindBestMatch, :1141) above, one block per frame */

/* ---- library / device ---- */
const char* zjni_version(void);
/* Number of usable HIP devices (0 when none). */
int zjni_device_count(void);
/* Selects device `ordinal` for the calling thread's subsequent calls and creates its per-device
 * state (work counters, literal scratch). Returns 0 or a negative ZJNI/ZSTD error code. */
int zjni_init(int ordinal);
void zjni_shutdown(void);

/* ---- error helpers: N/jni_zstd.c:240-267 (Zstd.isError / getErrorName / getErrorCode) ---- */
unsigned zjni_isError(size_t result);
int zjni_getErrorCode(size_t result);
const char* zjni_getErrorName(size_t result);

/* ---- sizing helpers ---- */
/* == ZSTD_compressBound (N/zstd.h:249) == Zstd.compressBound (N/jni_zstd.c:229-232) */
size_t zjni_compressBound(size_t srcSize);
/* == ZSTD_getFrameContentSize (N/zstd.h:203-217) == Zstd.getFrameContentSize0 (N/jni_zstd.c:116-130):
 * content size, (uint64)-1 unknown, (uint64)-2 error.  Host-side header parse, no GPU needed. */
unsigned long long zjni_getFrameContentSize(const void* src, size_t srcSize);

/* ---- hot path, device-resident batch -------------------------------------------------------
 * HBM layout: n independent buffers packed in one blob; buffer i occupies
 * [d_src + d_src_off[i], d_src + d_src_off[i+1]) and may write
 * [d_dst + d_dst_off[i], d_dst + d_dst_off[i+1]).  Offsets are uint64[n+1] in device memory.
 * d_result[i] receives buffer i's produced size or error (uint64, same convention as size_t).
 * Asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream).
 * Returns 0 when the launch was enqueued, else an error code result. */

/* Replaces ZSTD_decompressDCtx (N/jni_fast_zstd.c:798-799, :825-826) for n frames at once.
 * Every source buffer may hold several concatenated frames and skippable frames, exactly as
 * ZSTD_decompressMultiFrame accepts (N/decompress/zstd_decompress.c:1070-1168). */
size_t zjni_decompress_batch_device(const void* d_src, const uint64_t* d_src_off,
                                    void* d_dst, const uint64_t* d_dst_off,
                                    uint64_t* d_result, size_t n, void* stream);

/* Replaces ZSTD_CCtx_reset + ZSTD_compress2 (N/jni_fast_zstd.c:606-607, :633-635) for n buffers at
 * once: each buffer becomes one standard zstd frame (content size in the header, no checksum,
 * no dictID) that any zstd decoder accepts.  level: 1..3 (N/compress/clevels.h), or 4 for inputs up to ZJNI_LEVEL4_MAX / 5..8 up to ZJNI_LAZY_MAX (plain
 * entries only: no dictionary, no explicit table sizes; a wave-per-frame kernel with one lane parsing — exact, not fast).  Negative levels (zstd's
 * --fast=N, down to ZSTD_minCLevel() = -131072; lower ones are clamped to it, as the reference clamps them): the fast strategy with the parameters of
 * row 0 of the size's table, the match loop stepping N + 1 and raw literals, on level 1's routes (every entry that takes a level, the blocking
 * ones, the aggregator, begin/finish and the multi-device entry included; no explicit table sizes; dictionaries and streams at these levels: below).  Buffers larger than
 * ZJNI_BLOCKSIZE_MAX become multi-block frames (one wavefront per frame, block after block; see ZJNI_FRAME_MAX for the
 * range); beyond it d_result[i] reports ZJNI_ERROR_unsupported and the buffer stays on the CPU path.
 * Destination capacity (d_dst_off[i+1] - d_dst_off[i]): with zjni_compressBound(srcSize) a frame always fits.  With less, the answer is
 * ZSTD_compress2's for that capacity — which wants working room beyond the frame's bytes (18 bytes for any header, 8 bytes of slack behind
 * each bit stream, N/compress/zstd_compress.c:4711, 3024-3030; DESIGN.md section 1 "tight destination"): ZSTD_error_dstSize_tooSmall possibly
 * although the frame would have fitted, or a raw block where the compressed one found no room — same size, bytes or code. */
size_t zjni_compress_batch_device(const void* d_src, const uint64_t* d_src_off,
                                  void* d_dst, const uint64_t* d_dst_off,
                                  uint64_t* d_result, size_t n, int level, void* stream);
/* Same with ZSTD_c_checksumFlag = checksum (ZstdCompressCtx.setChecksum0, N/jni_fast_zstd.c:276-282;
 * Zstd.compressUnsafe(..., checksumFlag), N/jni_zstd.c:50-63): frames end with the low 32 bits of
 * XXH64(content, 0).  The decompress entries verify a frame's checksum whenever its header announces one
 * (ZSTD_error_checksum_wrong on mismatch), like ZSTD_decompressDCtx. */
size_t zjni_compress_batch_device2(const void* d_src, const uint64_t* d_src_off,
                                   void* d_dst, const uint64_t* d_dst_off,
                                   uint64_t* d_result, size_t n, int level, int checksum, void* stream);

/* ---- sizing a decompress batch from its frames alone ----
 * A consumer that holds frames only (the root of the multi-GPU gather, frames read from storage or a peer straight into HBM) does not know
 * d_dst_off.  The entries below take a buffer of concatenated zstd and skippable frames and answer what the reference's header-only calls
 * answer for it, for every input, valid or not; nothing outside [src, src + srcSize) is read.  Legacy formats are off, as in the bundled build. */
typedef struct zjni_frame_info {   /* 40 bytes, 8-aligned, same layout on host and device */
    uint64_t content;         /* ZSTD_findDecompressedSize(buf): sum over all frames; ~0 unknown, ~0 - 1 error */
    uint64_t bound;           /* ZSTD_decompressBound(buf); ~0 - 1 error */
    uint64_t firstFrameSize;  /* ZSTD_findFrameCompressedSize(buf): bytes of the first (zstd or skippable) frame,
                                 or the reference's own error code in the size_t convention */
    uint32_t dictID;          /* ZSTD_getDictID_fromFrame(buf) */
    uint32_t frames;          /* complete zstd frames walked before the end or the first malformed spot */
    uint32_t skippable;       /* complete skippable frames, likewise */
    uint32_t flags;           /* ZJNI_INFO_* over the frames counted above */
} zjni_frame_info;
#define ZJNI_INFO_CHECKSUM 1u   /* some zstd frame carries a checksum */
#define ZJNI_INFO_UNKNOWN  2u   /* some zstd frame has no content size */
#define ZJNI_INFO_SINGLE   4u   /* exactly one zstd frame filling the buffer, nothing else */
/* Replaces ZSTD_findDecompressedSize + ZSTD_decompressBound + ZSTD_findFrameCompressedSize + ZSTD_getDictID_fromFrame
 * (N/decompress/zstd_decompress.c:643-680, :820-836, :809-812, :1644-1650) for one buffer, in one walk over its frame and block
 * headers.  Runs on the host and needs no device, like zjni_getFrameContentSize.  Returns 0. */
size_t zjni_inspect(const void* src, size_t srcSize, zjni_frame_info* out);
/* The same four calls for n buffers in HBM (layout below: buffer i = d_src[d_src_off[i] .. d_src_off[i + 1])), one lane per buffer:
 * d_info[i] = what zjni_inspect answers for buffer i.  Replaces a copy of every header to the host, one ZSTD_getFrameContentSize /
 * ZSTD_findFrameCompressedSize per frame there (N/jni_zstd.c:116-130) and an upload of the sizes.  Asynchronous on `stream`. */
size_t zjni_inspect_batch_device(const void* d_src, const uint64_t* d_src_off, zjni_frame_info* d_info, size_t n, void* stream);
/* d_dst_off[0 .. n] for a decompress call, from d_info[0 .. n): replaces the host loop that sums ZSTD_getFrameContentSize /
 * ZSTD_decompressBound results into destination offsets.  Buffer i's slot is its `content` when known, else its `bound` when that is not
 * the error value, else 0; with slotMax != 0 a slot above slotMax counts as 0 (one hostile header declaring 2^60 bytes would starve every
 * buffer behind it); slots are rounded up to `align`, a power of two from 1 to 65536 (anything else: ZSTD_error_parameter_outOfBound).
 * d_needed[0] = the sum of all slots; d_dst_off[k] = min(sum of slots 0 .. k - 1, dstCapacity): buffers that do not fit get a short or
 * empty slot, the decoder answers ZSTD_error_dstSize_tooSmall for them by itself, and the caller compares d_needed[0] with its capacity
 * and retries.  Sums saturate at 2^64 - 1.  n == 0 is legal.  Asynchronous on `stream`. */
size_t zjni_decompress_offsets_device(const zjni_frame_info* d_info, size_t n, uint64_t dstCapacity, uint64_t align, uint64_t slotMax,
                                      uint64_t* d_dst_off, uint64_t* d_needed, void* stream);

/* ---- dictionaries, decompress side (SURVEY.md §8a last rows; BASELINE config 4) ----
 * zjni_ddict == ZSTD_DDict as zstd-jni holds it in ZstdDictDecompress.nativePtr (J/ZstdDictDecompress.java,
 * N/jni_fast_zstd.c:56-96): created once from the dictionary bytes (zstd dictionary format with magic
 * 0xEC30A437, or raw content), shared read-only by any number of batch calls on the device it was created on.
 * createDDict returns NULL for a corrupted dictionary (ZSTD_createDDict does the same) or without a device. */
typedef struct zjni_ddict zjni_ddict;
zjni_ddict* zjni_createDDict(const void* dict, size_t dictSize);
size_t zjni_freeDDict(zjni_ddict* ddict);
unsigned zjni_getDictID_fromDDict(const zjni_ddict* ddict);
/* Replaces ZSTD_decompress_usingDDict (N/jni_fast_zstd.c:133-183 decompress*FastDict0, and
 * ZstdDecompressCtx.loadDict + decompress*0) for n frames at once.  ddict == NULL behaves like
 * zjni_decompress_batch_device.  Frames naming another dictionary ID report ZSTD_error_dictionary_wrong. */
size_t zjni_decompress_batch_device_usingDDict(const void* d_src, const uint64_t* d_src_off,
                                               void* d_dst, const uint64_t* d_dst_off,
                                               uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream);
size_t zjni_decompress_batch_usingDDict(const void* const* src, const size_t* srcSize,
                                        void* const* dst, const size_t* dstCapacity,
                                        size_t* result, size_t n, const zjni_ddict* ddict);
size_t zjni_decompress_usingDDict(void* dst, size_t dstCapacity, const void* src, size_t srcSize, const zjni_ddict* ddict);
/* zjni_inspect_batch_device + zjni_decompress_offsets_device + zjni_decompress_batch_device_usingDDict in one call, nothing waited for on the
 * host: replaces ZSTD_findDecompressedSize / ZSTD_decompressBound per buffer on the host (N/decompress/zstd_decompress.c:643-680, :820-836)
 * followed by ZSTD_decompress_usingDDict (N/jni_fast_zstd.c:133-183) for n buffers whose decoded sizes the caller does not know.  d_info[n],
 * d_dst_off[n + 1] and d_needed[1] are outputs; d_result and the bytes under d_dst are those of zjni_decompress_batch_device_usingDDict called
 * with the offsets this call wrote.  A d_needed[0] above dstCapacity says which capacity a second call needs; buffers that did fit are decoded
 * already.  Ordered with the device's other batch calls like every batch entry.  n == 0 is legal: d_dst_off[0] = 0, d_needed[0] = 0. */
size_t zjni_decompress_batch_device_sized(const void* d_src, const uint64_t* d_src_off, void* d_dst, uint64_t dstCapacity, uint64_t align,
                                          uint64_t slotMax, zjni_frame_info* d_info, uint64_t* d_dst_off, uint64_t* d_needed,
                                          uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream);

/* ---- large buffers as many frames ----
 * The batch entries above are built for many small independent buffers: a buffer of concatenated frames is decoded by ONE wavefront, frame after frame, and an
 * input above ZJNI_FRAME_MAX is not compressed at all.  zstd's own way to make large data parallel without leaving the format is to cut it into independent
 * frames laid end to end (pzstd, the seekable format, a log of appended frames, zjni_pack_batch_device2's output); every zstd decoder reads the result as one
 * buffer (ZSTD_decompressMultiFrame, N/decompress/zstd_decompress.c:1070-1168).  The entries below turn n large buffers into E small entries on the device, run
 * the batch pipelines above on the entries and fold their answers back into one per buffer.
 *
 * Frame-parallel decompress.  zjni_decompress_frames_batch_device takes the arguments, layout, ordering and result convention of
 * zjni_decompress_batch_device_usingDDict and answers, for every input, valid or not, what that entry answers: the same d_result[i] and, where that is a
 * size, the same bytes under d_dst.  Split rule: buffer i becomes one entry per frame when (a) its source is at most 2^32 - 1 bytes, (b) a walk over its frame
 * and block headers from byte 0 until no byte is left meets no error, (c) every zstd frame on the way records a content size and (d) there are at least two zstd
 * frames; any other buffer is one entry, the whole buffer, exactly as in the entry above.  A skippable frame of a split buffer is an entry that decodes to 0 bytes.
 * An entry's destination starts at the buffer's slot plus the content sizes before it, clamped to the slot's end: an interior frame's slot is exactly its content
 * size, the last one keeps the rest, and a buffer that does not fit gets short slots (the decoder answers ZSTD_error_dstSize_tooSmall by itself).  d_result[i] is the
 * sum of the entries' sizes; a split buffer with an entry that answered an error (damage the header walk cannot see, a wrong dictionary, a short slot) is decoded
 * again as a whole by the wave-per-buffer kernel over the caller's own offsets, and whatever that answers stands — so no rule of ZSTD_decompressMultiFrame is
 * restated here.  Asynchronous on `stream` except for one read-back: the host waits for the entry count E (eight bytes, behind the counting walk), because the
 * pipelines size their launches and scratch on the host.  The entry arrays live in the library's scratch (zjni_set_scratch_limit).  E above 2^32 - 1: 72, as for n.
 * n == 0 is legal.  With zjni_inspect_batch_device + zjni_decompress_offsets_device in front, this entry also serves callers who hold frames only (no d_dst_off).
 * zjni_last_frames (synchronises; diagnostics): out4[0] buffers split, out4[1] entries decoded, out4[2] buffers not split, out4[3] buffers decoded again as a
 * whole, of the last zjni_decompress_frames_batch_device on this device.
 *
 * Chunked compress.  zjni_compress_chunked_batch_device writes buffer i as max(1, ceil(size / chunkSize)) frames laid end to end from d_dst + d_dst_off[i]: frame
 * k is, byte for byte, the frame zjni_compress_batch_device2 writes for src[k * chunkSize, min((k + 1) * chunkSize, size)) into a zjni_compressBound destination
 * (ZSTD_compress2's frame for that piece at that level); an empty buffer is the one frame of an empty input.  d_result[i] is the total; ZSTD_error_dstSize_tooSmall
 * (70) when the total exceeds the slot — then nothing is written outside the slot; or, when a piece answers an error (201 / 42 for a level that does not serve
 * its size), the first such piece's code.  chunkSize: 256 .. ZJNI_BLOCKSIZE_MAX, anything else is ZSTD_error_parameter_outOfBound (42) as the call's return value —
 * every piece is a single-block frame on the fast routes.  Levels: whatever zjni_compress_batch_device2 serves at the piece's size, negative levels included; no
 * dictionary, no explicit table sizes.  zjni_compressBound_chunked(srcSize, chunkSize) = the sum of zjni_compressBound over the pieces: a slot of that size always
 * fits (42 for a chunkSize out of range).  The same one read-back of E as above; E above 2^32 - 1: 72.  The pieces' scratch destinations count as library scratch
 * and are sliced under zjni_set_scratch_limit.
 *
 * zjni_compress_chunked / zjni_decompress_frames: blocking forms for ONE host buffer, staged through pinned memory like zjni_compress2 / zjni_decompress; what
 * a per-buffer native binds for inputs above ZJNI_FRAME_MAX and for buffers of many frames. */
size_t zjni_decompress_frames_batch_device(const void* d_src, const uint64_t* d_src_off,
                                           void* d_dst, const uint64_t* d_dst_off,
                                           uint64_t* d_result, size_t n, const zjni_ddict* ddict /* may be NULL */, void* stream);
int zjni_last_frames(unsigned out4[4]);
size_t zjni_compressBound_chunked(size_t srcSize, size_t chunkSize);
size_t zjni_compress_chunked_batch_device(const void* d_src, const uint64_t* d_src_off,
                                          void* d_dst, const uint64_t* d_dst_off,
                                          uint64_t* d_result, size_t n, int level, int checksum, size_t chunkSize, void* stream);
size_t zjni_compress_chunked(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level, int checksum, size_t chunkSize);
size_t zjni_decompress_frames(void* dst, size_t dstCapacity, const void* src, size_t srcSize);

/* ---- ranged decompress: decode only the frames a byte range touches ----
 * A buffer of many frames allows random access: a reader who wants decoded bytes [lo, lo + len) of buffer i needs the frames that hold them and no others.
 * zjni_decompress_frames_range_batch_device takes the layout, ordering and result convention of zjni_decompress_frames_batch_device plus d_range[2n] = (lo_i,
 * len_i), in decoded bytes of buffer i.  A buffer is decided in this order; the first rule that applies answers for it.
 *  1. Not indexable.  The buffer is walked frame header by frame header from byte 0 until no byte is left.  A walk that meets an error answers that step's own
 *     code (what ZSTD_findFrameCompressedSize answers at that frame); a zstd frame without a content size, a source above 2^32 - 1 bytes and content sizes that
 *     sum past 64 bits answer ZSTD_error_frameParameter_unsupported (14); of these, whichever the walk meets first.  One frame is enough.  d_total[i] = ~0 - 1.
 *  2. Range clamp.  T = the sum of the recorded content sizes (a skippable frame counts 0); d_total[i] = T.  lo' = min(lo, T), hi' = min(lo + len, T) with a
 *     saturating sum.  lo' == hi': the result is 0, nothing is decoded or written.
 *  3. Slot.  A slot d_dst_off[i + 1] - d_dst_off[i] (0 when not ascending) below hi' - lo' answers 70; nothing is decoded or written.
 *  4. Selection.  `first` is the frame holding decoded byte lo', `last` the one holding byte hi' - 1.  Every frame from first to last is decoded, frames without
 *     content and skippable frames between them included.  NO OTHER FRAME IS DECODED: damage outside the selection, which a decode of the whole buffer would
 *     report, is not seen — as with any seekable reader, a range answers for the frames it touches only.  first is an EDGE when it begins before lo', last when
 *     it ends after hi' (they may be one frame); an edge frame is decoded into library scratch and its part copied out, so an edge frame whose content size
 *     exceeds ZJNI_RANGE_EDGE_MAX answers ZSTD_error_memory_allocation (64) and nothing is decoded.  All other selected frames decode straight into the slot.
 *  5. Answer.  hi' - lo', with exactly the bytes [lo', hi') of the buffer's decoded content at d_dst + d_dst_off[i] and no other byte of d_dst written.  When
 *     selected frames answer errors, the result is the code of the lowest-numbered such frame, where a frame's answer is what
 *     zjni_decompress_batch_device_usingDDict gives for that frame alone with a capacity of exactly its content size; bytes inside the first hi' - lo' bytes of
 *     the slot are then unspecified, and nothing outside them is written.
 * Asynchronous on `stream` except for one read-back of 40 bytes behind the counting walk (entry counts and scratch sizes: the pipelines size their launches on the
 * host).  The selected source bytes, the entry arrays and the edge frames' scratch live in the library's scratch (zjni_set_scratch_limit: 64 above it).
 * n == 0 is legal; n or an entry count above 2^32 - 1: 72; a ddict digested on another device: 32.  d_total may be NULL.
 * zjni_last_frames_range (synchronises; diagnostics) of the last ranged call on this device: out4[0] buffers served (rules 2-5 reached without an error), out4[1]
 * frames handed to the decoder, out4[2] edge frames among them, out4[3] buffers that answered an error.
 * zjni_decompress_frames_range: the blocking form for ONE host buffer, staged like zjni_decompress_frames; *total (may be NULL) receives d_total's value. */
#define ZJNI_RANGE_EDGE_MAX ((size_t)128 << 20)
size_t zjni_decompress_frames_range_batch_device(const void* d_src, const uint64_t* d_src_off,
                                                 void* d_dst, const uint64_t* d_dst_off,
                                                 const uint64_t* d_range /* [2n]: lo_i, len_i, in decoded bytes of buffer i */,
                                                 uint64_t* d_result, uint64_t* d_total /* [n] or NULL */, size_t n,
                                                 const zjni_ddict* ddict /* may be NULL */, void* stream);
int zjni_last_frames_range(unsigned out4[4]);
size_t zjni_decompress_frames_range(void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                                    unsigned long long lo, unsigned long long len, unsigned long long* total /* or NULL */);

/* ---- explicit table sizes: ZstdCompressCtx.setHashLog / setChainLog (J/ZstdCompressCtx.java; N/jni_fast_zstd.c setHashLog0 /
 * setChainLog0 -> ZSTD_c_hashLog / ZSTD_c_chainLog) on top of level + checksum; 0 = not set.  Honoured for level 3
 * (double-fast): hashLog 6..17, chainLog 6..16, frames byte-identical to the reference called with the same two
 * parameters.  Not set, level 3 uses the reference's own sizes for the input (16 / 15 at 64 KiB: the frames of a plain
 * Zstd.compress(x, 3)); 14 / 13 are the sizes the LDS-resident finders of small batches are built for, honoured when asked for.
 * Other levels with a non-zero value (negative levels included): ZSTD_error_parameter_unsupported; out of range: parameter_outOfBound. */
/* Frame-header parameters: the `checksum` argument of the *_advanced and *_usingCDict entries is a flag word —
 * ZSTD_c_checksumFlag, ZSTD_c_contentSizeFlag = 0 (ZstdCompressCtx.setContentSize0(false), N/jni_fast_zstd.c:301-308: no frame
 * content size, a window descriptor instead; without a dictionary only) and ZSTD_c_dictIDFlag = 0 (setDictID0(false), :313-320).
 * A plain 0 / 1 keeps meaning "checksum off / on" with the other two at their defaults. */
#define ZJNI_FRAME_CHECKSUM       1
#define ZJNI_FRAME_NO_CONTENTSIZE 2
#define ZJNI_FRAME_NO_DICTID      4
#define ZJNI_SEQ_REPCODES         8   /* the sequence entries below only: ZSTD_c_searchForExternalRepcodes = enable */
#define ZJNI_SEQ_NO_DELIMITERS    16  /* zjni_compress_sequences_* only: ZSTD_c_blockDelimiters = ZSTD_sf_noBlockDelimiters, the library cuts the blocks */
size_t zjni_compress_batch_device_advanced(const void* d_src, const uint64_t* d_src_off,
                                           void* d_dst, const uint64_t* d_dst_off,
                                           uint64_t* d_result, size_t n, int level, int checksum, int hashLog, int chainLog, void* stream);
size_t zjni_compress_batch_advanced(const void* const* src, const size_t* srcSize,
                                    void* const* dst, const size_t* dstCapacity,
                                    size_t* result, size_t n, int level, int checksum, int hashLog, int chainLog);

/* ---- stream frames: ZstdDirectBufferCompressingStream[NoFinalizer] / ZstdOutputStream[NoFinalizer] ----
 * Replaces ZSTD_compressStream / ZSTD_flushStream / ZSTD_endStream as the stream natives call them
 * (N/jni_directbuffercompress_zstd.c:97-161: compressDirectByteBuffer, flushStream, endStream; N/jni_outputstream_zstd.c) for a stream that is
 * BUFFERED UNTIL IT IS CLOSED, at most the level's unknown-size window (levels 1 / 2 / 3: 512 KiB / 1 MiB / 2 MiB): the frame ZSTD_compressStream2
 * produces without a pledged size, byte for byte (N/compress/zstd_compress.c:6103-6300, :4591-4692) — the level's default parameter row whatever
 * the total, no content size in the header, the input cut into the stream's 128 KiB pieces, blocks ended where the caller flushed, the empty raw
 * last block, the checksum.  Negative levels (zstd's --fast=N, clamped at -131072): row 0 of that table (window 19, chain 12, hash 13, minMatch 6),
 * the match loop stepping N + 1, raw literals, level 1's 512 KiB window.  flushAt[0 .. nFlush): ascending byte counts after which the caller flushed.  final_ = 0: flushed, not closed — returns the
 * frame's beginning up to the last flush (the bytes a later call with more input reproduces and continues).  knownEmpty: the stream was closed before
 * any other call (its size, 0, is then known: single-segment header).  201 above the window, 42 above level 3: the bundled library's stream.
 * The device form takes n streams: stream i = blob[off[i], off[i + 1]), its flush positions d_flush_at[d_flush_off[i] .. d_flush_off[i + 1]) (d_flush_off may be
 * NULL: none), d_mode[i] = final | knownEmpty << 1 (NULL: all final). */
/* ZSTD_findFrameCompressedSize + ZSTD_getFrameContentSize + ZSTD_decompressBound for one complete zstd frame at src (N/zstd.h:227-290;
 * N/decompress/zstd_decompress.c:739-850) — what the decompress-stream natives (N/jni_directbufferdecompress_zstd.c:58-79) need to know before they can hand a
 * whole frame to zjni_decompress instead of feeding ZSTD_decompressStream: returns the frame's size in bytes (0: src does not hold a complete well-formed zstd
 * frame), *content = the recorded content size or ~0, *bound = an upper bound of the decoded size. */
size_t zjni_frame_extent(const void* src, size_t srcSize, unsigned long long* content, unsigned long long* bound);
size_t zjni_compress_stream(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level, int checksum,
                            const uint32_t* flushAt, size_t nFlush, int final_, int knownEmpty);
size_t zjni_compress_stream_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                         uint64_t* d_result, size_t n, int level, int checksum,
                                         const uint32_t* d_flush_at, const uint64_t* d_flush_off, const uint32_t* d_mode, void* stream);

/* ---- stream frames continued from device state ----
 * Replaces ZSTD_compressStream2 with ZSTD_e_flush / ZSTD_e_end on a LIVE ZSTD_CStream (N/compress/zstd_compress.c:6103-6300): the entries above keep nothing
 * between calls, so every flush compresses the stream again from its first byte and returns the frame's beginning again.  Here the stream's state — its hash
 * table(s), the repcodes and the Huffman table of the last compressed block, what it has consumed and produced — stays in device memory between calls: a call
 * compresses only the bytes written since the last flush and returns only the frame's NEW bytes.  The calls' outputs, concatenated, are the frame the entries
 * above write for the whole stream, byte for byte; the levels, the windows and the buffering until a flush are theirs.
 *
 * Device form.  zjni_cstream_state_bytes(level): bytes of one stream's state, a multiple of 256 (0: a level the streams do not serve); the caller owns the
 * memory, state i lies at d_state + i * zjni_cstream_state_bytes(level), and an all-zero state (a memset) is a stream on which nothing has been done.
 * zjni_compress_stream_continue_batch_device takes zjni_compress_stream_batch_device's arguments plus d_state: d_src slot i holds EVERYTHING written to stream i
 * so far, d_dst slot i receives the new frame bytes only, d_result[i] is their count — 0 when nothing was flushed since the last call.  Flush positions at or
 * below what the stream has consumed are ignored (pass all of them or only the new ones, ascending); the streams of one call may be at different stages; the
 * call is ordered with the device's other batch calls.  A slot of  new + (new >> 8) + 4096 + 64 * (newFlushes + 4)  bytes always suffices, `new` being the
 * source bytes behind what the stream has consumed.  Besides a size d_result[i] answers 201 (the total exceeds the level's window: the bundled library's
 * stream takes over from byte 0), ZSTD_error_stage_wrong (60: the state is closed already, was begun with another level or checksum flag, or the source is
 * shorter than what was consumed) and ZSTD_error_dstSize_tooSmall (70).  After an error the state is dead and answers that code from then on.
 *
 * Host form, after ZSTD_CStream (ZSTD_createCStream / ZSTD_freeCStream / ZSTD_CCtx_reset(session_only) / ZSTD_compressStream2): the handle owns the device copy
 * of the source so far, the state and a staging slot, so only new bytes cross the link, once.  zjni_cstream_compress: `src` holds the NEW bytes only;
 * directive 0 (ZSTD_e_continue) buffers them and returns 0, 1 (ZSTD_e_flush) and 2 (ZSTD_e_end) return the count of new frame bytes written to dst.  With
 * dstCapacity below the bound above (new = every byte not yet flushed, these included; newFlushes = 1) the call answers dstSize_tooSmall before touching
 * anything: neither the buffered bytes nor the state change.  201 beyond the window leaves the handle dead (the caller's CPU path replays the stream) until
 * zjni_cstream_reset, which starts the next frame with the same parameters.  ZSTD_e_end as the first directive on a fresh handle, without bytes, is the
 * knownEmpty case above.  A handle is bound to the device of the thread that created it and serves one thread at a time.
 *
 * Full pieces compressed as they are written (ZSTD_e_continue as ZSTD_compressStream_generic's zcss_load stage serves it: the stream's 128 KiB input buffer is
 * compressed the moment it is full).  Device form: bit 2 (value 4) of d_mode[i], beside 1 (close) and 2 (closed before anything else).  With it a call that
 * does not close consumes, behind the newest flush position F it was given (F = what the stream has consumed when there is none), every full piece as well:
 * F + ((size - F) / 131072) * 131072 bytes in all.  d_result[i] is 0 when that completes no piece.  The bit means nothing on a closing call; the streams of one
 * call may mix all directives; the refusals, the state's layout and size are as above.  The slot bound above holds unchanged: such a call writes a prefix of
 * what a closing call on the same bytes would write.  A piece that is full is never the frame's last block: the close behind it writes the buffered rest, or
 * the 3-byte empty last block, which is ZstdOutputStream's frame (it closes without bytes).
 * Host form: zjni_createCStream2(level, checksum, ZJNI_CSTREAM_EAGER); zjni_createCStream(l, c) is zjni_createCStream2(l, c, 0).  On an eager handle directive 0
 * copies the new bytes, sends the pieces they complete to the device and launches their compression on the handle's stream WITHOUT waiting, then returns the
 * frame bytes of the pieces launched by EARLIER calls (it waits for those), as many as dstCapacity allows; the rest stays held.  zjni_cstream_pending: the
 * frame bytes finished or in flight and not yet handed out (it waits for the work in flight to know them; 0 on a plain handle).  Directives 1 and 2 hand out
 * what is held first, then their own bytes, and want dstCapacity >= zjni_cstream_pending + the bound above for the bytes no piece has taken; below that they
 * answer dstSize_tooSmall and nothing changes.  zjni_cstream_reset and zjni_freeCStream wait for the work in flight and drop it; 201 drops what is held (the
 * CPU path replays from byte 0).  A piece in flight holds the device's batch order: other batch calls on the device run behind it. */
size_t zjni_cstream_state_bytes(int level);
size_t zjni_compress_stream_continue_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                                  uint64_t* d_result, size_t n, int level, int checksum,
                                                  const uint32_t* d_flush_at, const uint64_t* d_flush_off, const uint32_t* d_mode,
                                                  void* d_state, void* stream);
typedef struct zjni_cstream zjni_cstream;
zjni_cstream* zjni_createCStream(int level, int checksum);
#define ZJNI_CSTREAM_EAGER 1
zjni_cstream* zjni_createCStream2(int level, int checksum, int flags);
size_t zjni_cstream_pending(const zjni_cstream* cs);
size_t zjni_freeCStream(zjni_cstream* cs);
size_t zjni_cstream_reset(zjni_cstream* cs);
size_t zjni_cstream_compress(zjni_cstream* cs, void* dst, size_t dstCapacity, const void* src, size_t srcSize, int directive);

/* ---- compression dictionaries ----
 * zjni_cdict == ZSTD_CDict as zstd-jni holds it in ZstdDictCompress.nativePtr (J/ZstdDictCompress.java;
 * N/jni_fast_zstd.c:18-66: init = ZSTD_createCDict(dict, size, level), free = ZSTD_freeCDict).  The dictionary is
 * digested once on the device: parameters of (level, dictSize), tagged hash tables over the content, the entropy
 * tables and repcodes of its header.  Levels 1..3, and every negative level (zstd's --fast=N; below ZSTD_minCLevel() = -131072
 * clamped to it): row 0 of the table the dictionary's size picks (N/compress/clevels.h), targetLength = N, the fast strategy's digest; its
 * frames step N in the attach-mode search and N + 1 in copy mode, with raw literals (N/compress/zstd_fast.c:491, :717;
 * zstd_compress_internal.h:685).  NULL for a corrupted dictionary, a level above 3, fewer than 8 bytes, or without a device. */
typedef struct zjni_cdict zjni_cdict;
zjni_cdict* zjni_createCDict(const void* dict, size_t dictSize, int level);
size_t zjni_freeCDict(zjni_cdict* cdict);
unsigned zjni_getDictID_fromCDict(const zjni_cdict* cdict);
/* Replaces ZstdCompressCtx.loadDict(ZstdDictCompress) + compress*0 = ZSTD_CCtx_refCDict + ZSTD_compress2
 * (N/jni_fast_zstd.c:325-336, :586-640) and ZSTD_compress_usingCDict (compress*FastDict0, N/jni_fast_zstd.c:171-216)
 * for n buffers at once; frames are byte-identical to the reference's.  Covers the sizes at which the reference
 * searches the dictionary in place ("attach": srcSize <= 8 KiB when the dictionary's strategy is fast, <= 16 KiB when
 * it is double-fast) and, beyond them up to one block (128 KiB), its copy mode (ZSTD_resetCCtx_byCopyingCDict,
 * N/compress/zstd_compress.c:2402-2468: the dictionary as an external segment) as long as the reference compresses with
 * the dictionary's own parameters (srcSize < 128 KiB or < 6 x the dictionary's content, :5256-5257); otherwise the
 * result slot reports ZSTD_error_parameter_unsupported (more than one block: ZJNI_ERROR_unsupported).  The same at every level
 * the CDict was made for, negative levels included. */
size_t zjni_compress_batch_device_usingCDict(const void* d_src, const uint64_t* d_src_off,
                                             void* d_dst, const uint64_t* d_dst_off,
                                             uint64_t* d_result, size_t n, const zjni_cdict* cdict, int checksum, void* stream);
size_t zjni_compress_batch_usingCDict(const void* const* src, const size_t* srcSize,
                                      void* const* dst, const size_t* dstCapacity,
                                      size_t* result, size_t n, const zjni_cdict* cdict, int checksum);
size_t zjni_compress_usingCDict(void* dst, size_t dstCapacity, const void* src, size_t srcSize, const zjni_cdict* cdict);

/* ---- chunked compress with a dictionary, the caller's cuts and the frame sizes out (a record store: one segment = one buffer of one frame per record) ----
 * zjni_compress_pieces_batch_device takes the layout, ordering, result convention, the one eight-byte-per-count read-back behind the counting kernel, the slicing
 * under zjni_set_scratch_limit, n == 0 and the 72 for n or an entry count above 2^32 - 1 of zjni_compress_chunked_batch_device, and adds three things.
 *  Cuts.  d_cut == NULL: the fixed grid, max(1, ceil(size / chunkSize)) pieces; with cdict, d_piece_first and d_piece_size NULL as well the call writes the bytes and
 *    results of zjni_compress_chunked_batch_device(level, flags & 1, chunkSize).  d_cut given: buffer i's cuts are d_cut[d_cut_off[i] .. d_cut_off[i + 1]), in bytes
 *    from the buffer's start, and its pieces exactly the gaps [0, c0), [c0, c1), ..., [c_last, size).  A list is legal when d_cut_off ascends at i, the cuts ascend
 *    strictly, every cut lies in (0, size) and no piece exceeds chunkSize; an empty buffer with an empty list is the one frame of an empty input.  An illegal list
 *    answers ZSTD_error_parameter_outOfBound (42) in d_result[i]: no byte of that slot is written, the buffer contributes ZERO entries to the index below, and the
 *    other buffers of the call are not affected.  chunkSize (256 .. ZJNI_BLOCKSIZE_MAX, else the call returns 42) is then the largest piece allowed, and every piece
 *    gets zjni_compressBound(chunkSize) of library scratch; pieces may be as small as one byte.
 *  Dictionary.  Without cdict frame k is the frame zjni_compress_batch_device2 writes for the piece at `level` (0 means 3; a level not served: the call returns 42).
 *    With cdict `level` is ignored and frame k is, byte for byte, the frame zjni_compress_batch_device_usingCDict writes for the piece with the same flag word into a
 *    zjni_compressBound destination (attach and copy mode, negative levels); a piece that entry refuses answers its code, and the first such code is the buffer's
 *    result.  A cdict digested on another device: what that entry answers (32).  flags: ZJNI_FRAME_CHECKSUM always, ZJNI_FRAME_NO_DICTID with a cdict;
 *    ZJNI_FRAME_NO_CONTENTSIZE makes the call return 42 (frames without a content size can be neither split nor range-read afterwards).
 *  Index.  d_piece_first[i] (when given, [n + 1]) = the entries before buffer i, d_piece_first[n] = E.  d_piece_size[e] (when given) = the compressed size of entry e:
 *    for a buffer whose result is a size they sum to it, and frame e starts at d_dst_off[i] plus the sizes of the buffer's entries before e; for a buffer that
 *    answered an error they are unspecified.  With d_piece_size given and E > pieceCap the call returns 70 before any compress work is queued; d_result is then
 *    untouched.  A caller who keeps the index hands exactly the frames it wants to zjni_decompress_batch_device[_usingDDict]: no walk over the buffer.  The index is
 *    the caller's memory: nothing about it is written into the stream.
 * zjni_compressBound_pieces(srcSize, nPieces) = srcSize + (srcSize >> 8) + 64 * max(nPieces, 1), at least the sum of zjni_compressBound over any nPieces pieces of
 * srcSize bytes: a slot of this size always fits.
 * zjni_compress_pieces: the blocking form for ONE host buffer (cut == NULL: the fixed grid); pieceSize[0 .. min(E, pieceCap)) and *nPieces = E when given.
 * zjni_decompress_frames_usingDDict / zjni_decompress_frames_range_usingDDict: zjni_decompress_frames / zjni_decompress_frames_range with a dictionary. */
size_t zjni_compressBound_pieces(size_t srcSize, size_t nPieces);
size_t zjni_compress_pieces_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                         uint64_t* d_result, size_t n, int level, int flags, size_t chunkSize,
                                         const uint64_t* d_cut /* or NULL */, const uint64_t* d_cut_off /* [n + 1], with d_cut */,
                                         const zjni_cdict* cdict /* or NULL */,
                                         uint64_t* d_piece_first /* [n + 1] or NULL */, uint64_t* d_piece_size /* [pieceCap] or NULL */, size_t pieceCap,
                                         void* stream);
size_t zjni_compress_pieces(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level, int flags, size_t chunkSize,
                            const uint64_t* cut, size_t nCut, const zjni_cdict* cdict,
                            uint64_t* pieceSize /* or NULL */, size_t pieceCap, size_t* nPieces /* or NULL */);
size_t zjni_decompress_frames_usingDDict(void* dst, size_t dstCapacity, const void* src, size_t srcSize, const zjni_ddict* ddict);
size_t zjni_decompress_frames_range_usingDDict(void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                                               unsigned long long lo, unsigned long long len, unsigned long long* total /* or NULL */, const zjni_ddict* ddict);

/* ---- indexed range reads: many byte ranges per call by a caller-held index, no walk over the frame headers ----
 * The ranged entry above walks every frame header of every buffer for any range and answers one range per buffer.  A caller who knows the sizes of its frames
 * (zjni_compress_pieces_batch_device returns them) prepares an index once and reads by it: R requests per call, any number per buffer, found by bisection.
 *
 * THE INDEX of n buffers and E entries lives in the caller's device memory, zjni_index_bytes(n, E) bytes (a multiple of 256), all values uint64, in this order:
 *     first[n + 1]   entries before each buffer; first[n] = E
 *     valid[n]       0, or the error code (2 .. 2^32 - 1) that answers every request for the buffer
 *     C[E + 1]       exclusive running sums of the entries' compressed sizes over the whole batch (C[0] = 0)
 *     U[E + 1]       exclusive running sums of the entries' content sizes over the whole batch (U[0] = 0)
 * An entry is a whole number of frames, usually one; a coarser index (several frames an entry) is legal, the decoder reads such a slice as it reads any buffer.
 * Callers may store the index and may write one themselves.
 * zjni_index_from_sizes_device builds it from d_piece_first[n + 1], d_piece_size[E] and d_piece_content[E] for any buffers of concatenated frames.  Buffer i is
 * illegal, valid[i] = ZSTD_error_parameter_outOfBound (42), when d_piece_first does not ascend at i, when d_piece_first[i + 1] exceeds E, or when one of its sizes
 * or content sizes exceeds 2^32 - 1 (such a value counts 0 in the sums); the other buffers are not affected.  The sums are one parallel scan over E.
 * zjni_index_from_pieces_device writes the same index from what a zjni_compress_pieces_batch_device call took (the UNCOMPRESSED d_src_off, chunkSize, d_cut,
 * d_cut_off) and gave (d_result, d_piece_first, d_piece_size; E = d_piece_first[n]): content sizes come from the cuts, or from the fixed grid when d_cut is NULL,
 * and a buffer whose d_result is an error carries that code in valid.  Both builders are asynchronous on `stream`, wait for nothing on the host, and take n == 0
 * and E == 0; n or E above 2^32 - 1: 72.
 *
 * zjni_decompress_index_range_batch_device: d_src / d_src_off[n + 1] are the n buffers of frames, d_req[3R] = (b_r, lo_r, len_r) asks for decoded bytes
 * [lo, lo + len) of buffer b, and request r's slot is d_dst + d_dst_off[r] .. d_dst_off[r + 1] (ascending with r).  Requests are independent: any number per
 * buffer, in any buffer order, overlapping or not; a frame two requests select is decoded twice.  A request is decided in this order, the first rule that applies
 * answers for it.
 *  1. Index.  b >= n answers 42; valid[b] != 0 answers that code (a value outside 2 .. 2^32 - 1, or first[b] .. first[b + 1] not inside 0 .. E: 42); a source extent
 *     d_src_off[b + 1] - d_src_off[b] (0 when not ascending) other than C[first[b + 1]] - C[first[b]] answers ZSTD_error_srcSize_wrong (72).  d_total[r] = ~0 - 1.
 *  2. Range clamp.  T = U[first[b + 1]] - U[first[b]]; d_total[r] = T; lo' = min(lo, T), hi' = min(lo + len, T) with a saturating sum.  lo' == hi': the result
 *     is 0, nothing is decoded or written.
 *  3. Slot.  A slot below hi' - lo' answers 70; nothing is decoded or written.
 *  4. Selection, by bisection over U: `first` is the entry holding decoded byte lo', `last` the one holding byte hi' - 1 (an entry without content holds no byte);
 *     every entry from first to last is decoded, entries without content between them included, AND NO OTHER ENTRY IS LOOKED AT: neither its header nor its bytes
 *     are read.  Edge and interior entries, the scratch of an edge and ZJNI_RANGE_EDGE_MAX (64 above it) are rule 4 of the ranged entry above.
 *  5. Answer.  hi' - lo', with exactly the bytes [lo', hi') of the buffer's decoded content in the slot and no other byte of d_dst written.  When selected entries
 *     answer errors the result is the code of the lowest-numbered such entry, as in the ranged entry, where an entry's answer is what
 *     zjni_decompress_batch_device_usingDDict gives for its bytes alone with a capacity of exactly the content size the index states; an entry that decodes WITHOUT
 *     error to another size than the index states answers ZSTD_error_corruption_detected (20) (an entry that holds more than the index states does not fit its
 *     slot and answers the decoder's 70).  Bytes inside the first hi' - lo' bytes of the slot are then unspecified, and nothing outside them is written.
 * The index is the caller's memory and may hold anything.  Whatever it holds, no byte outside buffer b's source extent is read for request r and no byte outside
 * request r's slot or the library's scratch is written: every derived offset is clamped, and a request whose selected entries' sums do not ascend inside the
 * selection answers 20: its interior entries are handed to the decoder with slots of no byte, so none of them is written anywhere.  What a false index answers otherwise is wrong data or an entry's error, as a false header would.
 * Asynchronous on `stream` except for one read-back of 40 bytes behind the request kernel and its scans (entry counts and scratch sizes: the pipelines size their
 * launches on the host), as in the ranged entry.  Scratch as there (zjni_set_scratch_limit: 64 above it).  R == 0, n == 0 and E == 0 are legal; n, E, R or an entry
 * count above 2^32 - 1: 72; a ddict digested on another device: 32.  d_total may be NULL.
 * zjni_last_index_range (synchronises; diagnostics) of the last indexed call on this device: out4[0] requests served (rules 2-5 reached without an error), out4[1]
 * entries handed to the decoder, out4[2] edge entries among them, out4[3] requests that answered an error.
 * zjni_decompress_index_range: the blocking form for ONE host buffer with its nPieces sizes and content sizes in host memory.  It selects on the host by the same
 * rules and sends ONLY the selected entries' compressed bytes and their slice of the index across the link; answer, bytes and *total (may be NULL) are those of
 * staging the whole buffer.
 *
 * THE INDEX FROM THE FRAMES ALONE, for whoever holds only the bytes (another process, a file read back, frames of the reference or of pzstd): two walks over the
 * frame headers, once, and every later read is the indexed one.  One entry is one frame; a skippable frame is an entry of content 0.
 * A buffer is INDEXABLE by exactly rule 1 of the ranged entry above, in walk order, first failure first (a source above 2^32 - 1 bytes: 14; a step's error: that
 * step's code; a zstd frame without a content size: 14; content sizes summing past 64 bits: 14) WITH ONE ADDITION the entry format forces: a frame that records
 * a content size above 2^32 - 1 answers 14 at that frame.  It is the only place where the ranged entry and a read by this index may answer differently.  A
 * buffer that is not indexable owns 0 entries and carries its code in valid[i]: every read of it answers that code.  An empty buffer owns 0 entries, valid 0.
 *  zjni_index_count_frames_device: the first walk, one lane per buffer, and the exclusive scan: d_piece_first[i] = the entries before buffer i,
 *    d_piece_first[n] = E.  The caller reads those eight bytes and allocates zjni_index_bytes(n, E).
 *  zjni_index_from_frames_device: the second walk writes each buffer's sizes at d_piece_first[i], then valid, then C and U by the builders' scan.  d_piece_size
 *    and d_piece_content ([E] each, either may be NULL) receive the entries' compressed and content sizes: the compact form a caller stores beside the file,
 *    from which zjni_index_from_sizes_device rebuilds the index without the bytes.  The second walk trusts nothing of the first: it is bounded by
 *    d_piece_first[i + 1] - d_piece_first[i] and writes inside that extent only; a d_piece_first that does not ascend at i or exceeds E gives valid[i] = 42, and so
 *    does a walk that does not end at the buffer's end with exactly that count (the bytes changed between the calls, or the array is not the first call's); the
 *    buffer's entries are then written as 0 and the other buffers are not affected.
 * Both are asynchronous on `stream` and wait for nothing on the host; n == 0 and E == 0 are legal; n or E above 2^32 - 1: 72.
 * zjni_index_from_frames: the same walk for ONE host buffer, pure host code, no device: pieceSize[] and pieceContent[] as zjni_decompress_index_range takes
 * them and *nPieces = the entry count.  Returns 0; the buffer's code when it is not indexable (*nPieces = 0); 70 with *nPieces = the count needed when
 * `capacity` is below it (capacity == 0 with NULL arrays is the counting call).  A host reader of a file then uploads only the frames a range selects. */
size_t zjni_index_count_frames_device(const void* d_src, const uint64_t* d_src_off /* [n + 1] */, size_t n, uint64_t* d_piece_first /* [n + 1] out */, void* stream);
size_t zjni_index_from_frames_device(const void* d_src, const uint64_t* d_src_off /* [n + 1] */, size_t n, const uint64_t* d_piece_first /* [n + 1] */, size_t E,
                                     void* d_index, uint64_t* d_piece_size /* [E] out, or NULL */, uint64_t* d_piece_content /* [E] out, or NULL */, void* stream);
size_t zjni_index_from_frames(const void* src, size_t srcSize, uint64_t* pieceSize, uint64_t* pieceContent, size_t capacity, size_t* nPieces);
size_t zjni_index_bytes(size_t n, size_t E);
size_t zjni_index_from_sizes_device(size_t n, const uint64_t* d_piece_first /* [n + 1] */, const uint64_t* d_piece_size /* [E] */,
                                    const uint64_t* d_piece_content /* [E] */, size_t E, void* d_index, void* stream);
size_t zjni_index_from_pieces_device(const uint64_t* d_src_off /* [n + 1], of the uncompressed buffers */, size_t n, size_t chunkSize,
                                     const uint64_t* d_cut /* or NULL */, const uint64_t* d_cut_off /* [n + 1], with d_cut */,
                                     const uint64_t* d_result /* [n] or NULL */, const uint64_t* d_piece_first /* [n + 1] */, const uint64_t* d_piece_size /* [E] */,
                                     size_t E, void* d_index, void* stream);
size_t zjni_decompress_index_range_batch_device(const void* d_src, const uint64_t* d_src_off /* [n + 1] */, size_t n, const void* d_index, size_t E,
                                                const uint64_t* d_req /* [3R]: b_r, lo_r, len_r */,
                                                void* d_dst, const uint64_t* d_dst_off /* [R + 1] */,
                                                uint64_t* d_result /* [R] */, uint64_t* d_total /* [R] or NULL */, size_t R,
                                                const zjni_ddict* ddict /* may be NULL */, void* stream);
int zjni_last_index_range(unsigned out4[4]);
size_t zjni_decompress_index_range(void* dst, size_t dstCapacity, const void* src, size_t srcSize,
                                   unsigned long long lo, unsigned long long len,
                                   const uint64_t* pieceSize, const uint64_t* pieceContent, size_t nPieces,
                                   unsigned long long* total /* or NULL */, const zjni_ddict* ddict /* may be NULL */);

/* ---- hot path, host buffers (what a JNI batch native binds; stages through pinned memory) ---- */
size_t zjni_decompress_batch(const void* const* src, const size_t* srcSize,
                             void* const* dst, const size_t* dstCapacity,
                             size_t* result, size_t n);
size_t zjni_compress_batch(const void* const* src, const size_t* srcSize,
                           void* const* dst, const size_t* dstCapacity,
                           size_t* result, size_t n, int level);
size_t zjni_compress_batch2(const void* const* src, const size_t* srcSize,
                            void* const* dst, const size_t* dstCapacity,
                            size_t* result, size_t n, int level, int checksum);

/* ---- the same entries, asynchronous: two host batches in flight (round 5) ----
 * zstd-jni's natives block (N/jni_fast_zstd.c:586-640: one ZSTD_compress2 per call); a batch native over this library would too, and a single host batch is
 * a chain: gather + H2D, kernels, D2H + scatter (75 + 143 + 35 ms on 65 536 x 64 KiB at level 3) — the lane pipeline wants the whole batch resident before its
 * kernels start.  The overlap comes from the NEXT batch: every device has two staging slots with their own streams, so while one call's kernels run the other
 * call's sources cross the link one way and a finished call's frames the other.  Two threads inside zjni_compress_batch2 / zjni_decompress_batch get that by
 * themselves; these entries give it to one thread: _begin returns at once with a job that runs the blocking entry on a thread of the library (bound to the
 * caller's device), zjni_batch_finish waits for it, returns the call's code and frees the job.  Every array and buffer passed to _begin belongs to the job until
 * _finish returns; `result` is written as in the blocking entries.  NULL: no device bound, or no thread to be had.  More than two jobs may be begun; the third
 * waits for a slot.  What compressBatch0 / decompressBatch0 of the JNI library would call to keep two Java-side batches in flight. */
typedef struct zjni_batch_job zjni_batch_job;
zjni_batch_job* zjni_compress_batch_begin(const void* const* src, const size_t* srcSize,
                                          void* const* dst, const size_t* dstCapacity,
                                          size_t* result, size_t n, int level, int checksum);
zjni_batch_job* zjni_decompress_batch_begin(const void* const* src, const size_t* srcSize,
                                            void* const* dst, const size_t* dstCapacity,
                                            size_t* result, size_t n);
size_t zjni_batch_finish(zjni_batch_job* job);

/* ---- one host batch over several GPUs of this process (a JVM is one process) ----
 * The batch is cut into contiguous index ranges of about equal source bytes, one per entry of `devices` (ordinals, nDevices <= 64;
 * an ordinal may repeat); one thread per device runs its range.  Frames and results are what the single-device entries give.
 * mode 0: every device returns its frames to the host over its own PCIe link — no inter-GPU traffic, the right choice for host
 *         consumers (JVM buffers).
 * mode 1: (compress) every device packs its frames and sends them to devices[0] over xGMI (peer copies: the output gather of
 *         section 8e, 7 links into one device), which returns the whole batch in one transfer.
 * The calling thread's own device binding is left as it was. */
size_t zjni_compress_batch_multi(const void* const* src, const size_t* srcSize,
                                 void* const* dst, const size_t* dstCapacity,
                                 size_t* result, size_t n, int level, int checksum,
                                 const int* devices, int nDevices, int mode);
size_t zjni_decompress_batch_multi(const void* const* src, const size_t* srcSize,
                                   void* const* dst, const size_t* dstCapacity,
                                   size_t* result, size_t n, const int* devices, int nDevices);

/* ---- cross-thread aggregation of per-buffer calls ----
 * zstd-jni's per-buffer natives (N/jni_fast_zstd.c:586-640, :777-905) are called from many threads, one buffer each.  An aggregator
 * turns concurrent blocking calls into batches: the first caller of a kind (compress at a level + checksum flag / decompress) opens a
 * batch and waits up to maxWaitMicros (or until maxBatch callers have joined), then runs zjni_compress_batch2 / zjni_decompress_batch
 * once for everybody.  Each call returns what the per-buffer form would (frame size or error code).  stats: calls made, batches run. */
typedef struct zjni_aggregator zjni_aggregator;
zjni_aggregator* zjni_createAggregator(int device, size_t maxBatch, unsigned maxWaitMicros);
void zjni_freeAggregator(zjni_aggregator* a);
size_t zjni_aggregator_compress(zjni_aggregator* a, void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level, int checksum);
size_t zjni_aggregator_decompress(zjni_aggregator* a, void* dst, size_t dstCapacity, const void* src, size_t srcSize);
void zjni_aggregator_stats(zjni_aggregator* a, unsigned long long* calls, unsigned long long* batches);

/* ---- per-buffer forms with the exact argument meaning of the calls they replace ---- */
/* ZSTD_compress2(cctx{level}, dst, dstCapacity, src, srcSize): N/jni_fast_zstd.c:607 */
size_t zjni_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level);
/* the same with ZSTD_c_checksumFlag (Zstd.compress(dst, src, level, checksumFlag), J/Zstd.java) */
size_t zjni_compress2(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int level, int checksum);
/* ZSTD_decompressDCtx(dctx, dst, dstCapacity, src, srcSize): N/jni_fast_zstd.c:799 */
size_t zjni_decompress(void* dst, size_t dstCapacity, const void* src, size_t srcSize);

/* ---- synthetic mixed-entropy workload, identical bytes on host and device ---- */
void zjni_synth_fill_host(void* dst, size_t bufSize, uint64_t firstIndex, size_t nBuffers);
size_t zjni_synth_fill_device(void* d_dst, size_t bufSize, uint64_t firstIndex, size_t nBuffers, void* stream);

/* ---- output assembly for the multi-GPU gather ----
 * Moves frame i from d_src[d_src_off[i] .. +d_sizes[i]) to d_dst[d_dst_off[i] ..): tight packing of a
 * compress batch's variable-size outputs before the RCCL payload gather.  Entries of d_sizes that are
 * error results are skipped. */
size_t zjni_pack_batch_device(const void* d_src, const uint64_t* d_src_off, const uint64_t* d_sizes,
                              void* d_dst, const uint64_t* d_dst_off, size_t n, void* stream);
/* The same with the packed offsets made on the device: d_packed_off[0 .. n] (out) = exclusive prefix sums of the sizes (error results count as 0),
 * then the frames move there.  One call instead of a scan by the caller plus the pack (round 5). */
size_t zjni_pack_batch_device2(const void* d_src, const uint64_t* d_src_off, const uint64_t* d_sizes,
                               void* d_dst, uint64_t* d_packed_off, size_t n, void* stream);

/* ---- resource policy ----
 * The large-batch pipelines keep per-frame scratch in HBM (match-finder tables and sequence records, decode cells): one buffer
 * per pipeline and device, allocated on first use and kept, sized for a 288 GB part (65 536 frames in flight: ~26 GiB compress,
 * ~49 GiB for frames > 64 KiB, ~34 GiB with a dictionary, ~22 GiB decompress).  A process that shares the GPU bounds that:
 *   zjni_set_scratch_limit(bytes)  total scratch the library may hold per device (0 = no limit; values below 4 GiB are raised to
 *                                  4 GiB).  Batches are cut into slices whose scratch fits — results are unchanged, throughput
 *                                  drops as slices shrink — and a pipeline that needs room evicts the others' buffers.
 *                                  Returns the limit in force.  The limit is process-wide.
 *   zjni_scratch_bytes()           scratch currently held on the calling thread's device.
 *   zjni_release_scratch()         free-on-idle: waits for the device's outstanding batch calls, then frees all of it (the next
 *                                  call allocates again).  0 or an error code.
 * Concurrent callers of one device are serialised: batch calls are enqueued under a per-device mutex and each call's first kernel
 * waits (on the GPU) for the previous call's last one, whatever streams the callers use; the scratch is shared, results are not. */
size_t zjni_set_scratch_limit(size_t bytes);
size_t zjni_scratch_bytes(void);
size_t zjni_release_scratch(void);

/* ---- introspection for tests/bench ---- */
/* Workgroups the persistent kernels launch per device and LDS bytes per workgroup. */
int zjni_kernel_info(int* decodeGrid, int* decodeLdsBytes, int* encodeGrid, int* encodeLdsBytes);
/* Stage durations (ms) of the last large-batch device calls, from HIP events recorded on the caller's stream
 * around the kernels: out5[0] lane-per-frame match-finder kernel (compress); out5[1..4] decode stages prep /
 * lane-per-frame sequence decode / execute / fused leftovers.  Blocks until those stages have completed;
 * stages that did not run read -1.  Profiling aid (bench.py roofline), not on the data path. */
int zjni_last_timing(float* out5);
/* The same five plus out8[5] = the wide match-finder kernel (frames > 64 KiB), last slice of the call; out8[6..7] read -1. */
int zjni_last_timing2(float* out8);
/* Which match finder served list A of the last large compress call on this device (bench.py names the roofline's kernel from this, not from the
 * environment: a refused LDS attribute, a scratch budget or a failed allocation changes the route silently).  Negative: no device. */
#define ZJNI_ROUTE_NONE 0         /* no large-batch compress call yet */
#define ZJNI_ROUTE_FUSED 1        /* zj_encode_kernel alone (small batches, levels 1-2 and negative levels) */
#define ZJNI_ROUTE_WAVE 2         /* zj_enc_match_wave_kernel (small level-3 batches, tables in LDS) */
#define ZJNI_ROUTE_LANE 3         /* zj_enc_match_kernel (levels 1-2; level 3 under ZJNI_LANE_MACHINE=0 without flags); negative levels: the same machine in zj_enc_match_kernel_neg */
#define ZJNI_ROUTE_LANE_GATED 4   /* zj_enc_match_gated_kernel (ZJNI_LANE_MACHINE=0 with flags) */
#define ZJNI_ROUTE_RUN 5          /* zj_enc_match_run_kernel without need flags */
#define ZJNI_ROUTE_RUN_FLAGS 6    /* zj_enc_match_run_kernel behind zj_enc_worth_kernel / zj_enc_need_kernel */
#define ZJNI_ROUTE_HYBRID 7       /* ZJNI_HYBRID=1: lane and wave kernels side by side */
#define ZJNI_ROUTE_OTHER 8        /* levels 4-8, dictionaries, multi-block only */
#define ZJNI_ROUTE_WAVE_HBM 9     /* zj_encode_multi_kernel: level-3 frames of batches below ZJNI_L3_WAVE_MAX, wave per frame over HBM tables (zj_match_wavex.h) */
#define ZJNI_ROUTE_WIDE 10        /* zj_enc_match_wide_kernel: the launch of frames above 64 KiB (list B; negative levels: zj_enc_match_wide_kernel_neg); never zjni_last_route()'s answer — see zjni_last_lists */
#define ZJNI_ROUTE_PIPE 11        /* zj_encode_pipe_kernel (round 6): multi-block frames of a batch that leaves wave slots empty, a parse wave a block ahead of an entropy wave per frame;
                                     decided on the device from the list counts, so zjni_last_route() says it only after zjni_last_lists() has read them */
int zjni_last_route(void);
/* How the last large compress call's frames were split: out3[0] the common launch (the route above), out3[1] the wide launch (ZJNI_ROUTE_WIDE), out3[2] the
 * multi-block / wave-per-frame kernel.  A batch of 128 KiB buffers has out3[1] = n: its match-finder time is zjni_last_timing2's out8[5] and its kernel
 * zjni_route_kernel(ZJNI_ROUTE_WIDE).  Synchronises with the device (diagnostics only). */
int zjni_last_lists(unsigned* out3);
/* The same for the last large decompress call: out4[0] frames of the single-block pipeline (prep -> lane-per-frame sequence decode -> execute), out4[1] frames the
 * fused wave-per-frame kernel decoded (what no pipeline took, or handed over), out4[2] frames of the multi-block stages (lane per BLOCK; frames of several blocks
 * or without a content size), out4[3] their blocks.  Synchronises with the device (diagnostics only). */
int zjni_last_decode_lists(unsigned* out4);
/* zjni_last_decode_lists plus out5[4]: frames that are a header and ONE stored (raw or RLE) block — what ZSTD_compress2 writes for data that does not compress
 * (N/compress/zstd_compress.c:4591-4692, ZSTD_noCompressBlock) — which stage 1 of the large-batch pipeline copies itself; they are on none of the three lists. */
int zjni_last_decode_lists2(unsigned* out5);
/* TEST ENTRY, not on any data path: the entropy stage (zj_encode_kernel, mode 0) on sequences the CALLER wrote instead of a match finder's.  n sources on the device
 * (offsets as everywhere), each ONE block of at most 128 KiB; HOST arrays: h_rec = {ll, ml, offBase, pos} per sequence (pos: where its literals start; the sequences
 * tile the source in order), frame i's at h_rec[4 * h_rec_off[i] .. 4 * h_rec_off[i + 1]), h_meta[3 i ..] = {nbSeq, litSize, lastLL}.  Records that do not tile their
 * source answer an error (42) before anything is launched.  stagedLds: 0 = the dynamic LDS of the entropy launches without a dictionary (the stage alone), 1 = that of
 * the dictionary pipeline's (frames of at most 4096 bytes are staged in LDS).  grid > 0: at most that many workgroups (1: one workgroup meets every frame in turn).
 * One launch for the frames to 64 KiB, one for the wider ones.  d_result[i] as zjni_compress_batch_device2.  Synchronous. */
size_t zjni_test_compress_records_batch_device(const void* d_src, const uint64_t* d_src_off, const uint32_t* h_rec, const uint64_t* h_rec_off, const uint32_t* h_meta,
                                               void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int checksum, int stagedLds, int grid, void* stream);
/* ---- frames from the CALLER's sequences: ZSTD_compressSequences (N/compress/zstd_compress.c:7063-7110) for batches ----
 * The seam inside the library made public: a match finder writes sequences, the entropy stage turns them into blocks.  These entries take the sequences from
 * outside — a parse of the caller's own, a hardware match finder, a transcoder — and run only the entropy stage, at its speed.  Frame i is, byte for byte, what
 * the reference writes for ZSTD_compressSequences(cctx, dst, cap, seqs, nSeqs, src, srcSize) on a fresh CCtx with ZSTD_c_compressionLevel = level,
 * ZSTD_c_checksumFlag = flags & ZJNI_FRAME_CHECKSUM, ZSTD_c_blockDelimiters = ZSTD_sf_explicitBlockDelimiters, ZSTD_c_validateSequences = 1 and
 * ZSTD_c_searchForExternalRepcodes = enable with ZJNI_SEQ_REPCODES, disable without; any other flag bit: 42.
 *   - the caller cuts the blocks: a delimiter is a sequence with offset == 0 and matchLength == 0 whose litLength counts the block's last literals.  A block of
 *     less than 7 bytes is stored raw; a block that ends where the source ends is the last one and whatever follows it in the array is ignored; `rep` is ignored.
 *   - ZSTD_error_externalSequences_invalid (107) in the frame's slot, and only there: offset == 0 with a match length; no delimiter before the array ends; a block
 *     above 128 KiB or blocks that sum past the source; blocks that end before the source does; a match shorter than 4 (3 where the level's minMatch is 3); an
 *     offset beyond the bytes that precede the END of its match.  That last bound is the reference's: an offset may reach up to matchLength bytes in front of the
 *     source, the reference then writes a frame no decoder accepts, and so do these entries.  It is safe because the entropy stage never dereferences a match,
 *     only literals: nothing is read outside the sequence array and the source whatever the array holds.  (Lengths above 128 KiB answer 107 here; the reference
 *     adds litLength + matchLength in 32 bits first and is not defined on arrays that wrap.)
 *   - levels and sizes: those zjni_compress_batch_device serves (1-3 to ZJNI_FRAME_MAX inside the level's window, 4 to 128 KiB, 5-8 as there, every negative
 *     level), 201 otherwise; 0 means 3.  Where the level's row for the size is lazy or lazy2 (level 5 to 16 KiB, levels 6-8) a frame is served while its first block
 *     of 7 bytes or more is its last, a second one answers 201: those strategies weigh the previous block's sequence tables, which the entropy stage does not carry.
 *   - destinations as zjni_compress_batch_device2: every capacity gives the reference's size, bytes or dstSize_tooSmall (18 bytes for the header first).
 *   - no dictionary.
 * With ZJNI_SEQ_NO_DELIMITERS the array is in libzstd's other format, ZSTD_sf_noBlockDelimiters (its default, and what zjni_mergeBlockDelimiters returns): no
 * delimiters, the LIBRARY cuts the blocks by the reference's rule (ZSTD_transferSequences_noDelim, N/compress/zstd_compress.c:6744-6868), and frame i is the
 * reference's frame for that setting, byte for byte, or its error code.  Without the bit nothing changes.
 *   - a block aims at min(128 KiB, what is left); the sequence that straddles the edge decides where it ends: inside its literals the block ends at the edge; a
 *     match is split only if it is longer than the block's target and its first half is at least the level's cParams.minMatch (the edge moves back when the second
 *     half would be shorter than that), otherwise the block is shortened to end in front of the match.  Bytes the sequences do not cover are last literals, and
 *     sequences behind the end of the source are never read.  A frame whose last block was shortened holds fewer bytes than its header says: the reference writes
 *     it, so do these entries.
 *   - offset == 0 is no delimiter but an offset like any other (the reference accepts it and writes a frame no decoder takes).  Repcodes are always searched, as
 *     in the reference: ZJNI_SEQ_REPCODES is accepted and changes nothing.  Validation runs on the sequences as stored, trimmed and split; 107 in the frame's slot.
 *   - litLength + matchLength that does not fit 32 bits, where the reference's arithmetic wraps and reads out of bounds, answers 107 if the frame reaches it.
 *   - levels, sizes and destinations as above.  Where the level's row is lazy or lazy2 a source above 128 KiB answers 201 — a second compressed block does, as
 *     above, and in this mode the caller cannot cut the blocks to avoid one.
 *   - zjni_compress_sequences (one host buffer) with the bit answers 42 for dst == NULL, whatever the capacity: no frame, not even the empty one, fits in no
 *     destination, and a null pointer there is an argument error before it is a size.  (Without the bit a null destination of capacity 0 is answered as before.)
 *   - both offset arrays must ascend over the whole call (the slots of frame i are placed by d_seq_off[i] and d_src_off[i]): if one frame's pair descends or
 *     passes d_seq_off[n] / d_src_off[n], EVERY frame of the call answers srcSize_wrong (72).  Scratch: 24 bytes per sequence, 40 per 64 KiB of the sources and
 *     320 per frame; d_src_off[n] comes back in the same read as d_seq_off[n], still the one host wait.
 * d_seq_off[n + 1] counts SEQUENCES (frame i's are d_seqs[d_seq_off[i] .. d_seq_off[i + 1])).  Scratch: 20 bytes per sequence of the call from the library's
 * pool (zjni_set_scratch_limit applies; 64 when the call's records alone exceed it), sized from d_seq_off[n], which is read back once — the entry's one host wait;
 * everything else is enqueued on `stream`. */
typedef struct zjni_sequence { uint32_t offset, litLength, matchLength, rep; } zjni_sequence;      /* == ZSTD_Sequence, 16 bytes */
size_t zjni_sequenceBound(size_t srcSize);                                                         /* == ZSTD_sequenceBound: sequences a source of this size can need, delimiters included */
size_t zjni_compress_sequences_batch_device(const void* d_src, const uint64_t* d_src_off, const zjni_sequence* d_seqs, const uint64_t* d_seq_off,
                                            void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int flags, void* stream);
/* The same with host arrays (as zjni_compress_batch2, plus seqs[i] / nSeqs[i]); staged through a device buffer of the call's own.  Synchronous. */
size_t zjni_compress_sequences_batch(const void* const* src, const size_t* srcSize, const zjni_sequence* const* seqs, const size_t* nSeqs,
                                     void* const* dst, const size_t* dstCapacity, size_t* result, size_t n, int level, int flags);
size_t zjni_compress_sequences(void* dst, size_t dstCapacity, const zjni_sequence* seqs, size_t nSeqs, const void* src, size_t srcSize, int level, int flags);
/* Tests: at most `grid` workgroups for the two launches of the sequence entries (1: one workgroup meets every frame in turn); 0 restores the default.  Returns the previous value. */
int zjni_debug_sequences_grid(int grid);
/* ---- the matchers' sequences OUT: ZSTD_generateSequences (N/compress/zstd_compress.c:3520-3553, ZSTD_copyBlockSequences :3429-3512) for batches ----
 * The first half of the same seam: the match finders' parse of a source as ZSTD_Sequence[], for a caller who wants the parse alone — a transcoder, a match
 * statistics pass, a second entropy coder, a dictionary trainer — or who feeds it back to zjni_compress_sequences_*.  Frame i's slots hold what the reference
 * writes for ZSTD_generateSequences(cctx, out, cap, src, srcSize) on a fresh CCtx with only ZSTD_c_compressionLevel = level set:
 *   - per block its sequences {offset, litLength, matchLength, rep} — `offset` the RAW offset, `rep` 0 or the repcode number 1-3 the parser used — and one
 *     delimiter {0, lastLiterals, 0, 0} behind them (the reference leaves a delimiter's `rep` as the caller's memory held it; these entries write 0).  Lengths
 *     of 65 536 and more come out as they are.  A block is min(128 KiB, what is left) and every block confirms its repcodes (collecting mode, :4408-4411).
 *   - d_result[i]: the entries written, delimiters included, or an error code in the frame's slot, and only there: ZSTD_error_sequenceProducer_failed (106) for a
 *     source whose last block has fewer than 7 bytes (1-6 bytes, k x 128 KiB + 1 .. 6), as the reference; an empty source answers 0; dstSize_tooSmall (70) when
 *     a block's sequences plus its delimiter do not fit what is left of the slots (checked per block, before the block is written); 201 for a (level, size)
 *     zjni_compress_batch_device refuses.  On an error the slots' content is undefined; nothing is written outside them.  zjni_sequenceBound(srcSize) slots are always enough.
 *   - levels and sizes: those zjni_compress_batch_device serves without a dictionary (1-3 and every negative level to ZJNI_FRAME_MAX inside the level's window,
 *     multi-block frames included; 4-8 to 128 KiB); 0 means 3, and level 3 parses with the reference's own table sizes.  Any `flags` bit: 42, none is defined yet.
 *   - fed to zjni_compress_sequences_* the result gives a frame that decodes to the source; it is NOT ZSTD_compress2's frame (the reference's is not either).
 * d_seq_off[n + 1] counts SLOTS: frame i owns d_seqs[d_seq_off[i] .. d_seq_off[i + 1]).  Everything is enqueued on `stream`; the host waits only where scratch has
 * to grow (64 bytes of counters, once).  Every frame takes one wave of one kernel (parse, then export); the lane match kernels of large batches are not used yet. */
size_t zjni_generate_sequences_batch_device(const void* d_src, const uint64_t* d_src_off,
        zjni_sequence* d_seqs, const uint64_t* d_seq_off /* [n + 1]: frame i owns slots d_seq_off[i] .. d_seq_off[i + 1] */,
        uint64_t* d_result, size_t n, int level, int flags, void* stream);
/* The same with host arrays; staged through a device buffer of the call's own.  Synchronous. */
size_t zjni_generate_sequences_batch(const void* const* src, const size_t* srcSize, zjni_sequence* const* seqs,
        const size_t* seqCapacity, size_t* result, size_t n, int level, int flags);
size_t zjni_generate_sequences(zjni_sequence* seqs, size_t seqCapacity, const void* src, size_t srcSize, int level);
size_t zjni_mergeBlockDelimiters(zjni_sequence* seqs, size_t nSeqs);                         /* == ZSTD_mergeBlockDelimiters, host code */
/* The last generate call: out4[0] frames sent through a lane route (none yet: always 0), out4[1] through the wave route, out4[2] frames that answered an error code,
 * out4[3] 0.  Waits for the device (diagnostics: benches, tests); -1 when no generate call's counters are there to read. */
int    zjni_last_generate(unsigned out4[4]);
/* Tests: at most `grid` workgroups for the launch of the generate entries; 0 restores the default.  Returns the previous value. */
int    zjni_debug_generate_grid(int grid);
/* Name of the kernel a route's match-finder time (zjni_last_timing out[0]) belongs to. */
const char* zjni_route_kernel(int route);
/* The source revision the library was built from ("unknown" when the build had no git): profiles and PMC passes are stamped with it. */
const char* zjni_build_stamp(void);

#ifdef __cplusplus
}
#endif
#endif /* ZJNI_AMD_H */
