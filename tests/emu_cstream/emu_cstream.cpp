// tests/emu_cstream/emu_cstream.cpp — lane-serial (W = 1) build of ze_compress_stream_resume (zj_encode.h: a compress stream continued from its state, here in
// host memory) and, beside it, of the one-call ze_compress_stream it must agree with, for tests/test_emu_cstream.py.  The entries take the PUBLIC level, as the
// C-ABI does, and run what zj_encode_stream_continue_kernel / zj_encode_stream_kernel run with the entries' default flags (the one-lane block parses at levels 1-2).
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_cdict.h"
#include <stdlib.h>
#include <string.h>

static u32 emu_cs_word(int level) {
    if (level == 0) level = 3;
    if (level > 0) return (u32)level;
    return ZE_LW_NEGATIVE((u32)(level < -131072 ? 131072 : -level));
}
// persistent, poisoned workgroup state (as tests/emu/emu.cpp keeps it): whatever a call leaves in the workgroup and the next one reads shows up
struct EmuCsWg { ZEncShared* sh; u8* lds; u8* ws; };
static EmuCsWg& emu_cs_wg() {
    static EmuCsWg w = { nullptr, nullptr, nullptr };
    if (!w.sh) { w.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); w.lds = (u8*)malloc(160 * 1024); w.ws = (u8*)malloc(ZE_SCRATCH_BYTES); }
    memset(w.sh, 0xA5, sizeof(ZEncShared)); memset(w.lds, 0x5A, 160 * 1024); memset(w.ws, 0xC3, ZE_SCRATCH_BYTES);
    w.sh->dictLoaded = 0; w.sh->ctDict[0] = 0; w.sh->ctDict[1] = 0; w.sh->ctDict[2] = 0;       // (the kernels clear these once)
    return w;
}
// zjni_cstream_state_bytes
extern "C" unsigned emu_cs_state_bytes(int level) {
    if (level == 0) level = 3;
    return level > 3 ? 0u : ze_stream_state_bytes(emu_cs_word(level));
}
// One call of zjni_compress_stream_continue_batch_device on one stream.  Returns the NEW frame bytes or ZJ_ERR64(code).
extern "C" unsigned long long emu_cs_continue(void* state, const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, int checksum,
                                              const unsigned* flushAt, unsigned nFlush, int final_, int knownEmpty) {
    if (level == 0) level = 3;
    if (level > 3) return ZJ_ERR64(42);
    Grp<1> g;
    EmuCsWg& wg = emu_cs_wg();
    ZjProf pf; pf.start(nullptr);
    u32 const flags = (checksum ? ZE_FLAG_CHECKSUM : 0u) | ZE_FLAG_MULTI_FAST_SERIAL;
    return ze_compress_stream_resume(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, emu_cs_word(level), wg.ws, pf, flags, (ZEStreamState*)state, 160u * 1024u, flushAt, nFlush,
                                     final_ ? 1u : 0u, knownEmpty ? 1u : 0u);
}
// {consumed, produced, parsedBytes, blocks, closed, error, notFirst, lastFlag}
extern "C" void emu_cs_info(const void* state, unsigned* out) {
    const ZEStreamState* s = (const ZEStreamState*)state;
    out[0] = s->consumed; out[1] = s->produced; out[2] = s->parsedBytes; out[3] = s->blocks; out[4] = s->closed; out[5] = s->error; out[6] = s->notFirst; out[7] = s->lastFlag;
}
// zjni_compress_stream's frame, in one call from byte 0: the route that existed before the continuation and must not have moved
extern "C" unsigned long long emu_cs_compress_stream(const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, int checksum,
                                                    const unsigned* flushAt, unsigned nFlush, int final_, int knownEmpty) {
    if (level == 0) level = 3;
    if (level > 3) return ZJ_ERR64(42);
    if (srcSize > (1u << ze_stream_window_log(level < 0 ? 1u : (u32)level)) || srcSize > ZE_MULTI_MAX) return ZJ_ERR64(201);
    Grp<1> g;
    EmuCsWg& wg = emu_cs_wg();
    u32* tables = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(tables, 0xA5, ZE_MULTI_TABLE_BYTES);
    ZjProf pf; pf.start(nullptr);
    u32 const flags = (checksum ? ZE_FLAG_CHECKSUM : 0u) | ZE_FLAG_MULTI_FAST_SERIAL;
    u64 const r = ze_compress_stream(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, emu_cs_word(level), wg.ws, pf, flags, tables, 160u * 1024u, flushAt, nFlush, final_ ? 1u : 0u, knownEmpty ? 1u : 0u);
    free(tables);
    return r;
}
