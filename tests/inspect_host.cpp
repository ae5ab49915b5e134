// The walk of zstd-jni_amd/csrc/zj_frameinfo.h under a plain C++ compiler: tests/test_inspect.py builds this with the host sanitizers.
// Every call walks a malloc(srcSize) copy of its own (what -DEMU_EXACT does in tests/emu): the caller's buffer may live in an allocator the
// sanitizer does not watch (ctypes keeps small copies inside Python's own arenas), a malloc block of the exact size has a poisoned byte behind it.
// -DINSPECT_OVERREAD adds one read of that byte: the build tests/test_inspect.py uses to prove that the guard catches it.
#include <stdlib.h>
#include <string.h>
#include "../zstd-jni_amd/csrc/zj_frameinfo.h"

extern "C" size_t zjni_inspect(const void* src, size_t srcSize, zjni_frame_info* out) {
    u8* const copy = (u8*)malloc(srcSize);          // (malloc(0): a block of no bytes, every read of it is out of bounds)
    if (!copy) return ZJ_ERR64(64);
    if (srcSize) memcpy(copy, src, srcSize);
    zj_frame_walk(copy, (u64)srcSize, out);
#ifdef INSPECT_OVERREAD
    out->flags += ((volatile const u8*)copy)[srcSize] & 0u;
#endif
    free(copy);
    return 0;
}
