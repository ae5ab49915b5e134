/* tests/jni/negative_levels.c — Zstd.compressUnsafe at negative levels (zstd's --fast=N) through the JNI shim against the reference's own JNI
 * library: return values and bytes equal, and every call answered by the GPU path (zjni_shim_stats [0]; nothing forwarded, [1] = [2] = 0).
 * usage: negative_levels <reference JNI library> <shim>; run by tests/test_gpu_negative_levels.py with the bundled library behind the shim
 * (ZSTD_JNI_CPU_LIB) and ZSTD_JNI_GPU_PER_BUFFER=1, so that a call the GPU path declined would show up as a forward.  The native takes raw
 * pointers and never touches its JNIEnv. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jni.h"

typedef jlong (*compress_fn)(JNIEnv*, jclass, jlong, jlong, jlong, jlong, jint, jboolean);
typedef void (*stats_fn)(unsigned long long*);
#define NAME "Java_com_github_luben_zstd_Zstd_compressUnsafe"

static uint64_t g_x = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(void) { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (uint32_t)(g_x >> 11); }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <ref-jni.so> <shim.so>\n", argv[0]); return 2; }
    void* hr = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL); void* hs = dlopen(argv[2], RTLD_NOW | RTLD_LOCAL);
    if (!hr || !hs) { fprintf(stderr, "dlopen: %s\n", dlerror()); return 2; }
    compress_fn cr = (compress_fn)dlsym(hr, NAME), cs = (compress_fn)dlsym(hs, NAME);
    stats_fn st = (stats_fn)dlsym(hs, "zjni_shim_stats");
    if (!cr || !cs || !st) { fprintf(stderr, "missing symbols\n"); return 2; }
    static const int levels[] = { -1, -2, -3, -5, -7, -17, -100, -131072, -200000 };
    static const jlong sizes[] = { 0, 1, 100, 4096, 16384, 65536, 65537, 131072, 300000 };
    unsigned long long s0[4]; st(s0);
    int bad = 0, calls = 0;
    JNIEnv* env = NULL;
    for (size_t si = 0; si < sizeof sizes / sizeof *sizes; si++) {
        jlong const n = sizes[si];
        char* src = (char*)malloc((size_t)n + 1);
        for (jlong i = 0; i < n; i++) src[i] = (i % 7 == 0) ? (char)(rnd() & 0xFF) : "the quick brown fox jumps over the lazy dog "[(i / 3) % 44];
        jlong const cap = n + (n >> 7) + 128;
        char* a = (char*)malloc((size_t)cap); char* b = (char*)malloc((size_t)cap);
        for (size_t li = 0; li < sizeof levels / sizeof *levels; li++)
            for (int ck = 0; ck < 2; ck++) {
                jlong const ra = cr(env, NULL, (jlong)(intptr_t)a, cap, (jlong)(intptr_t)src, n, levels[li], ck ? JNI_TRUE : JNI_FALSE);
                jlong const rb = cs(env, NULL, (jlong)(intptr_t)b, cap, (jlong)(intptr_t)src, n, levels[li], ck ? JNI_TRUE : JNI_FALSE);
                calls++;
                if (ra != rb || (ra > 0 && ra < cap && memcmp(a, b, (size_t)ra) != 0)) {
                    bad++; fprintf(stderr, "differs: size %lld level %d checksum %d: reference %lld, shim %lld\n", (long long)n, levels[li], ck, (long long)ra, (long long)rb);
                }
            }
        free(src); free(a); free(b);
    }
    unsigned long long s1[4]; st(s1);
    unsigned long long const served = s1[0] - s0[0], policy = s1[1] - s0[1], declined = s1[2] - s0[2];
    printf("calls %d, differing %d, answered by the GPU %llu, forwarded by policy %llu, forwarded after a refusal %llu\n", calls, bad, served, policy, declined);
    if (bad || served != (unsigned long long)calls || policy || declined) { printf("NEGATIVE-LEVELS FAILED\n"); return 1; }
    printf("NEGATIVE-LEVELS OK\n");
    return 0;
}
