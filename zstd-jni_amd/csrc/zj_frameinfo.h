// zj_frameinfo.h — what a buffer of concatenated frames decodes to, from its headers alone: one walk, host and device.
//
// zj_frame_walk restates, for the zstd1 format with legacy support off, the four header-only entries of the reference:
//   ZSTD_findDecompressedSize   N/decompress/zstd_decompress.c:643-680   -> zjni_frame_info.content
//   ZSTD_decompressBound        :820-836 over ZSTD_findFrameSizeInfo :734-799   -> .bound
//   ZSTD_findFrameCompressedSize :809-812   -> .firstFrameSize
//   ZSTD_getDictID_fromFrame    :1644-1650 over ZSTD_getFrameHeader_advanced :447-551   -> .dictID
// The reference runs them as four passes; they agree on every frame's extent, so one pass frame by frame and block header by block
// header (ZSTD_getcBlockSize, N/decompress/zstd_decompress_block.c:63-77) gives all four.  Every read is checked against the buffer's
// end first — truncated input is the common case — and a block header is read as one 32-bit word where 4 bytes remain.
#pragma once
#include "zj_common.h"
#include "../../include/zjni_amd.h"

#define ZJ_FI_UNKNOWN (~(u64)0)                 /* ZSTD_CONTENTSIZE_UNKNOWN */
#define ZJ_FI_ERROR (~(u64)0 - 1)               /* ZSTD_CONTENTSIZE_ERROR */
#define ZJ_FI_MAGIC 0xFD2FB528u
#define ZJ_FI_SKIP_MAGIC 0x184D2A50u            /* ZSTD_MAGIC_SKIPPABLE_START; the low nibble is the frame's "magic variant" */
#define ZJ_FI_WINDOWLOG_MAX 31u                 /* ZSTD_WINDOWLOG_MAX of a 64-bit build */

// one frame at p, `rem` bytes left in the buffer: ZSTD_findFrameSizeInfo's answer plus what ZSTD_getFrameHeader saw on the way
struct ZFStep {
    u64 csize;        // bytes of the frame, or ZJ_ERR64(code)
    u64 dbound;       // decompressedBound: the content size when recorded, else blocks x block maximum; ZJ_FI_ERROR with an error
    u64 fcs;          // frame content size of a zstd frame (ZJ_FI_UNKNOWN: none)
    u32 hdr;          // ZSTD_getFrameHeader: 0 filled, else its error code (72: it asked for more input)
    u32 dictID;       // zfh.dictID (a skippable frame: its magic variant)
    u32 skippable, checksum;
};

ZJ_HD bool zj_fi_is_err(u64 r) { return r > ZJ_ERR64(120); }      // ZSTD_isError (ZSTD_error_maxCode = 120)

ZJ_HD void zj_frame_step(const u8* p, u64 rem, ZFStep& s) {
    s.csize = ZJ_ERR64(ZJ_E_SRCSIZE_WRONG); s.dbound = ZJ_FI_ERROR; s.fcs = ZJ_FI_UNKNOWN;
    s.hdr = ZJ_E_SRCSIZE_WRONG; s.dictID = 0; s.skippable = 0; s.checksum = 0;
    if (rem < 5) {      // :458-477: fewer bytes than the smallest header; those present must begin one of the two magic numbers
        if (rem > 0) {
            u32 const k = rem < 4 ? (u32)rem : 4u, keep = k == 4 ? 0xFFFFFFFFu : ((1u << (8 * k)) - 1u);
            u32 m = 0;
            for (u32 i = 0; i < k; i++) m |= (u32)p[i] << (8 * i);
            bool const zstd = ((m ^ ZJ_FI_MAGIC) & keep) == 0;
            bool const skip = ((((m & keep) | (ZJ_FI_SKIP_MAGIC & ~keep)) & 0xFFFFFFF0u) == ZJ_FI_SKIP_MAGIC);
            if (!zstd && !skip) s.hdr = ZJ_E_PREFIX_UNKNOWN;
        }
        s.csize = ZJ_ERR64(s.hdr);
        return;
    }
    u32 const magic = ld32(p);
    if ((magic & 0xFFFFFFF0u) == ZJ_FI_SKIP_MAGIC) {      // :482-492, :587-601
        s.skippable = 1;
        if (rem < 8) return;                              // the header wants 8 bytes: srcSize_wrong
        s.hdr = 0; s.dictID = magic - ZJ_FI_SKIP_MAGIC; s.fcs = 0;
        u32 const size32 = ld32(p + 4);
        if ((u32)(size32 + 8u) < size32) { s.csize = ZJ_ERR64(ZJ_E_FRAMEPARAM_UNSUPPORTED); return; }
        u64 const total = (u64)size32 + 8u;
        if (total > rem) return;
        s.csize = total; s.dbound = 0;
        return;
    }
    if (magic != ZJ_FI_MAGIC) { s.hdr = ZJ_E_PREFIX_UNKNOWN; s.csize = ZJ_ERR64(ZJ_E_PREFIX_UNKNOWN); return; }
    u32 const fhd = p[4], didc = fhd & 3u, single = (fhd >> 5) & 1u, fcsid = fhd >> 6;
    u32 const didSz = didc == 3 ? 4u : didc, fcsSz = fcsid == 0 ? single : (1u << fcsid);
    u64 pos = 5u + !single + didSz + fcsSz;               // ZSTD_frameHeaderSize_internal :416-429
    if (rem < pos) return;                                // srcSize_wrong, before the header's content is looked at (:497-499)
    if (fhd & 8u) { s.hdr = ZJ_E_FRAMEPARAM_UNSUPPORTED; s.csize = ZJ_ERR64(s.hdr); return; }
    u64 window = 0;
    u32 at = 5;
    if (!single) {
        u32 const wl = (p[5] >> 3) + 10u;
        if (wl > ZJ_FI_WINDOWLOG_MAX) { s.hdr = ZJ_E_WINDOW_TOO_LARGE; s.csize = ZJ_ERR64(s.hdr); return; }
        window = ((u64)1 << wl) + (((u64)1 << wl) >> 3) * (p[5] & 7u);
        at = 6;
    }
    s.dictID = didc == 0 ? 0u : didc == 1 ? (u32)p[at] : didc == 2 ? ld16(p + at) : ld32(p + at);
    at += didSz;
    u64 fcs = ZJ_FI_UNKNOWN;
    if (fcsid == 0) { if (single) fcs = p[at]; }
    else if (fcsid == 1) fcs = (u64)ld16(p + at) + 256u;
    else if (fcsid == 2) fcs = ld32(p + at);
    else fcs = ld64(p + at);
    if (single) window = fcs;
    s.hdr = 0; s.fcs = fcs; s.checksum = (fhd >> 2) & 1u;
    u32 const blockMax = (u32)(window < ZJNI_BLOCKSIZE_MAX ? window : ZJNI_BLOCKSIZE_MAX);
    u64 blocks = 0;
    ZJ_NO_UNROLL
    for (;;) {                                            // :769-783
        u64 const left = rem - pos;
        if (left < 3) return;
        u32 const bh = left >= 4 ? (ld32(p + pos) & 0xFFFFFFu) : ld24(p + pos), type = (bh >> 1) & 3u;
        if (type == 3) { s.csize = ZJ_ERR64(ZJ_E_CORRUPTION); return; }
        u64 const step = 3u + (type == 1 ? 1u : (u64)(bh >> 3));
        if (step > left) return;
        pos += step; blocks++;
        if (bh & 1u) break;
    }
    if (s.checksum) { if (rem - pos < 4) return; pos += 4; }
    s.csize = pos;
    s.dbound = fcs != ZJ_FI_UNKNOWN ? fcs : blocks * (u64)blockMax;
}

// The whole buffer [p, p + n).  `bound` follows ZSTD_decompressBound's loop (until no byte is left), `content` follows
// ZSTD_findDecompressedSize's beside it (it stops below 5 bytes and then objects to what is left, answers "unknown" at the first frame
// without a content size whatever follows, and checks its sum for overflow).  frames / skippable count the frames the bound's loop got
// past; the flags describe those frames.
ZJ_HD void zj_frame_walk(const u8* p, u64 n, zjni_frame_info* out) {
    ZFStep s;
    zj_frame_step(p, n, s);
    u64 const firstSize = s.csize;
    u32 const dictID = s.hdr == 0 ? s.dictID : 0u;        // ZSTD_getDictID_fromFrame: 0 unless the header was filled
    u64 content = 0, bound = 0, pos = 0;
    u32 frames = 0, skippable = 0, flags = 0;
    bool contentOpen = true, clean = true;
    ZJ_NO_UNROLL
    while (pos < n) {
        u64 const rem = n - pos;
        if (pos) zj_frame_step(p + pos, rem, s);
        bool const bad = zj_fi_is_err(s.csize);
        if (contentOpen) {
            if (rem < 5) { content = ZJ_FI_ERROR; contentOpen = false; }
            else if (s.skippable) { if (bad) { content = ZJ_FI_ERROR; contentOpen = false; } }
            else if (s.hdr != 0) { content = ZJ_FI_ERROR; contentOpen = false; }
            else if (s.fcs >= ZJ_FI_ERROR) { content = s.fcs; contentOpen = false; }
            else if (content + s.fcs < content || bad) { content = ZJ_FI_ERROR; contentOpen = false; }
            else content += s.fcs;
        }
        if (bad || s.dbound == ZJ_FI_ERROR) { bound = ZJ_FI_ERROR; clean = false; break; }
        bound += s.dbound;
        pos += s.csize;
        if (s.skippable) skippable++;
        else {
            frames++;
            if (s.checksum) flags |= ZJNI_INFO_CHECKSUM;
            if (s.fcs == ZJ_FI_UNKNOWN) flags |= ZJNI_INFO_UNKNOWN;
        }
    }
    if (clean && frames == 1 && skippable == 0) flags |= ZJNI_INFO_SINGLE;
    out->content = content; out->bound = bound; out->firstFrameSize = firstSize;
    out->dictID = dictID; out->frames = frames; out->skippable = skippable; out->flags = flags;
}

// ---- destination slots from the walk's answers (zjni_decompress_offsets_device) ----
ZJ_HD u64 zj_sat_add(u64 a, u64 b) { u64 const s = a + b; return s < a ? ~(u64)0 : s; }
// content when known, else the bound when it is no error, else 0; above slotMax (non-zero): 0; rounded up to alignMask + 1.  Sums and the rounding
// saturate at 2^64 - 1 instead of wrapping: a header may declare anything.
ZJ_HD u64 zj_info_slot(u64 content, u64 bound, u64 alignMask, u64 slotMax) {
    u64 s = content < ZJ_FI_ERROR ? content : (bound != ZJ_FI_ERROR ? bound : 0);
    if (slotMax && s > slotMax) s = 0;
    return s > ~(u64)0 - alignMask ? ~(u64)0 : ((s + alignMask) & ~alignMask);
}
