// tests/emu_cstream_pieces/emu_cstream_pieces.cpp — lane-serial (W = 1) build of ze_compress_stream_resume (zj_encode.h) as zj_encode_stream_continue_kernel calls it:
// the entry takes the device form's MODE WORD (1 = close, 2 = closed before anything else, 4 = continue: compress the full 128 KiB pieces now) and takes it apart as
// the kernel does, over a state in host memory; beside it the one-call ze_compress_stream the calls' outputs must add up to.  For tests/test_emu_cstream_pieces.py.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_cdict.h"
#include <stdlib.h>
#include <string.h>

static u32 emu_csp_word(int level) {
    if (level == 0) level = 3;
    if (level > 0) return (u32)level;
    return ZE_LW_NEGATIVE((u32)(level < -131072 ? 131072 : -level));
}
// persistent, poisoned workgroup state (as tests/emu/emu.cpp keeps it): whatever a call leaves in the workgroup and the next one reads shows up
struct EmuCspWg { ZEncShared* sh; u8* lds; u8* ws; };
static EmuCspWg& emu_csp_wg() {
    static EmuCspWg w = { nullptr, nullptr, nullptr };
    if (!w.sh) { w.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); w.lds = (u8*)malloc(160 * 1024); w.ws = (u8*)malloc(ZE_SCRATCH_BYTES); }
    memset(w.sh, 0xA5, sizeof(ZEncShared)); memset(w.lds, 0x5A, 160 * 1024); memset(w.ws, 0xC3, ZE_SCRATCH_BYTES);
    w.sh->dictLoaded = 0; w.sh->ctDict[0] = 0; w.sh->ctDict[1] = 0; w.sh->ctDict[2] = 0;       // (the kernels clear these once)
    return w;
}
// zjni_cstream_state_bytes
extern "C" unsigned emu_csp_state_bytes(int level) {
    if (level == 0) level = 3;
    return level > 3 ? 0u : ze_stream_state_bytes(emu_csp_word(level));
}
// One call of zjni_compress_stream_continue_batch_device on one stream, d_mode[i] = mode.  Returns the NEW frame bytes or ZJ_ERR64(code).
extern "C" unsigned long long emu_csp_continue(void* state, const unsigned char* src, unsigned long long srcSize, unsigned char* dst, unsigned dstCap, int level, int checksum,
                                               const unsigned* flushAt, unsigned nFlush, unsigned mode) {
    if (level == 0) level = 3;
    if (level > 3) return ZJ_ERR64(42);
    Grp<1> g;
    EmuCspWg& wg = emu_csp_wg();
    ZjProf pf; pf.start(nullptr);
    u32 const flags = (checksum ? ZE_FLAG_CHECKSUM : 0u) | ZE_FLAG_MULTI_FAST_SERIAL;
    u32 const size = srcSize > ZE_MULTI_MAX ? ZE_MULTI_MAX + 1u : (u32)srcSize;                  // (the kernel's clamp: beyond every window)
    return ze_compress_stream_resume(g, *wg.sh, wg.lds, src, size, dst, dstCap, emu_csp_word(level), wg.ws, pf, flags, (ZEStreamState*)state, 160u * 1024u, flushAt, nFlush,
                                     mode & 1u, (mode >> 1) & 1u, (mode >> 2) & 1u);
}
// {consumed, produced, parsedBytes, blocks, closed, error, notFirst, lastFlag}
extern "C" void emu_csp_info(const void* state, unsigned* out) {
    const ZEStreamState* s = (const ZEStreamState*)state;
    out[0] = s->consumed; out[1] = s->produced; out[2] = s->parsedBytes; out[3] = s->blocks; out[4] = s->closed; out[5] = s->error; out[6] = s->notFirst; out[7] = s->lastFlag;
}
// zjni_compress_stream's frame, in one call from byte 0
extern "C" unsigned long long emu_csp_compress_stream(const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, int checksum,
                                                      const unsigned* flushAt, unsigned nFlush, int final_, int knownEmpty) {
    if (level == 0) level = 3;
    if (level > 3) return ZJ_ERR64(42);
    if (srcSize > (1u << ze_stream_window_log(level < 0 ? 1u : (u32)level)) || srcSize > ZE_MULTI_MAX) return ZJ_ERR64(201);
    Grp<1> g;
    EmuCspWg& wg = emu_csp_wg();
    u32* tables = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(tables, 0xA5, ZE_MULTI_TABLE_BYTES);
    ZjProf pf; pf.start(nullptr);
    u32 const flags = (checksum ? ZE_FLAG_CHECKSUM : 0u) | ZE_FLAG_MULTI_FAST_SERIAL;
    u64 const r = ze_compress_stream(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, emu_csp_word(level), wg.ws, pf, flags, tables, 160u * 1024u, flushAt, nFlush, final_ ? 1u : 0u, knownEmpty ? 1u : 0u);
    free(tables);
    return r;
}
