/* tests/jni/negative_dict_stream.c — negative levels (zstd's --fast=N) with dictionaries and in compress streams, through the JNI shim against the
 * reference's own JNI library: ZstdDictCompress(dict, -N) loaded on a ZstdCompressCtx (byte[] and direct buffers), Zstd.compress(dst, src, ZstdDictCompress)
 * (compressFastDict0), ZstdCompressCtx.setLevel(-N).loadDict(byte[]), ZstdOutputStream and ZstdDirectBufferCompressingStream at -N.  Return values and bytes
 * equal, and nothing forwarded to the bundled library (zjni_shim_stats [1] = [2] = 0) while the GPU answered (zjni_shim_stats [0] grew).
 * usage: negative_dict_stream <reference JNI library> <shim>; run by tests/test_gpu_negative_dict_stream.py with the bundled library behind the shim
 * (ZSTD_JNI_CPU_LIB) and ZSTD_JNI_GPU_PER_BUFFER=1, so that a call the GPU path declined would show up as a forward. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "jni.h"

/* a minimal JNIEnv: byte[] and direct buffers are Obj, an object's long fields (nativePtr, srcPos, dstPos) and int fields (consumed, produced) live in it */
typedef struct Obj { int kind; char* data; jsize len; jlong field, srcPos, dstPos; jint consumed, produced; } Obj;     /* kind 1 direct buffer, 2 byte[], 7 plain object */
static Obj* mk(int kind, jsize len) { Obj* o = (Obj*)calloc(1, sizeof(Obj)); o->kind = kind; o->len = len; o->data = (char*)calloc((size_t)len + 16, 1); return o; }
static void* JNICALL f_GetDirectBufferAddress(JNIEnv* e, jobject b) { (void)e; return (b && ((Obj*)b)->kind == 1) ? ((Obj*)b)->data : NULL; }
static jlong JNICALL f_GetDirectBufferCapacity(JNIEnv* e, jobject b) { (void)e; return (b && ((Obj*)b)->kind == 1) ? ((Obj*)b)->len : -1; }
static jsize JNICALL f_GetArrayLength(JNIEnv* e, jarray a) { (void)e; return ((Obj*)a)->len; }
static void* JNICALL f_GetPrimitiveArrayCritical(JNIEnv* e, jarray a, jboolean* c) { (void)e; if (c) *c = JNI_FALSE; return ((Obj*)a)->data; }
static void JNICALL f_ReleasePrimitiveArrayCritical(JNIEnv* e, jarray a, void* p, jint m) { (void)e; (void)a; (void)p; (void)m; }
static void JNICALL f_GetByteArrayRegion(JNIEnv* e, jbyteArray a, jsize s, jsize l, jbyte* buf) { (void)e; memcpy(buf, ((Obj*)a)->data + s, (size_t)l); }
static void JNICALL f_SetByteArrayRegion(JNIEnv* e, jbyteArray a, jsize s, jsize l, const jbyte* buf) { (void)e; memcpy(((Obj*)a)->data + s, buf, (size_t)l); }
static jbyte* JNICALL f_GetByteArrayElements(JNIEnv* e, jbyteArray a, jboolean* c) { (void)e; if (c) *c = JNI_FALSE; return (jbyte*)((Obj*)a)->data; }
static void JNICALL f_ReleaseByteArrayElements(JNIEnv* e, jbyteArray a, jbyte* p, jint m) { (void)e; (void)a; (void)p; (void)m; }
static jclass JNICALL f_GetObjectClass(JNIEnv* e, jobject o) { (void)e; return (jclass)o; }
static jfieldID JNICALL f_GetFieldID(JNIEnv* e, jclass c, const char* n, const char* sig) {
    (void)e; (void)c; (void)sig;
    return (jfieldID)(intptr_t)(!strcmp(n, "nativePtr") ? 1 : !strcmp(n, "consumed") ? 2 : !strcmp(n, "produced") ? 3 : !strcmp(n, "srcPos") ? 4 : !strcmp(n, "dstPos") ? 5 : 0);
}
static jint JNICALL f_GetIntField(JNIEnv* e, jobject o, jfieldID f) { (void)e; return (intptr_t)f == 2 ? ((Obj*)o)->consumed : ((Obj*)o)->produced; }
static void JNICALL f_SetIntField(JNIEnv* e, jobject o, jfieldID f, jint v) { (void)e; if ((intptr_t)f == 2) ((Obj*)o)->consumed = v; else ((Obj*)o)->produced = v; }
static jlong JNICALL f_GetLongField(JNIEnv* e, jobject o, jfieldID f) { (void)e; return (intptr_t)f == 4 ? ((Obj*)o)->srcPos : ((intptr_t)f == 5 ? ((Obj*)o)->dstPos : ((Obj*)o)->field); }
static void JNICALL f_SetLongField(JNIEnv* e, jobject o, jfieldID f, jlong v) { (void)e; if ((intptr_t)f == 4) ((Obj*)o)->srcPos = v; else if ((intptr_t)f == 5) ((Obj*)o)->dstPos = v; else ((Obj*)o)->field = v; }
static jobject JNICALL f_NewDirectByteBuffer(JNIEnv* e, void* addr, jlong cap) { (void)e; Obj* o = (Obj*)calloc(1, sizeof(Obj)); o->kind = 1; o->len = (jsize)cap; o->data = (char*)addr; return (jobject)o; }
static jbyteArray JNICALL f_NewByteArray(JNIEnv* e, jsize n) { (void)e; return (jbyteArray)mk(2, n); }
static jboolean JNICALL f_ExceptionCheck(JNIEnv* e) { (void)e; return JNI_FALSE; }
static void JNICALL f_DeleteLocalRef(JNIEnv* e, jobject o) { (void)e; (void)o; }
static struct JNINativeInterface_ g_fn;
static const struct JNINativeInterface_* g_envp = &g_fn;
static JNIEnv* env(void) {
    g_fn.GetDirectBufferAddress = f_GetDirectBufferAddress; g_fn.GetDirectBufferCapacity = f_GetDirectBufferCapacity; g_fn.GetArrayLength = f_GetArrayLength;
    g_fn.GetPrimitiveArrayCritical = f_GetPrimitiveArrayCritical; g_fn.ReleasePrimitiveArrayCritical = f_ReleasePrimitiveArrayCritical;
    g_fn.GetByteArrayRegion = f_GetByteArrayRegion; g_fn.SetByteArrayRegion = f_SetByteArrayRegion; g_fn.GetByteArrayElements = f_GetByteArrayElements;
    g_fn.ReleaseByteArrayElements = f_ReleaseByteArrayElements; g_fn.GetObjectClass = f_GetObjectClass; g_fn.GetFieldID = f_GetFieldID;
    g_fn.GetIntField = f_GetIntField; g_fn.SetIntField = f_SetIntField; g_fn.GetLongField = f_GetLongField; g_fn.SetLongField = f_SetLongField;
    g_fn.NewDirectByteBuffer = f_NewDirectByteBuffer; g_fn.NewByteArray = f_NewByteArray; g_fn.ExceptionCheck = f_ExceptionCheck; g_fn.DeleteLocalRef = f_DeleteLocalRef;
    return (JNIEnv*)&g_envp;
}

#define P "Java_com_github_luben_zstd_"
typedef struct {
    void* h;
    jlong (*cinit)(JNIEnv*, jclass); void (*cfree)(JNIEnv*, jclass, jlong); void (*setLevel)(JNIEnv*, jclass, jlong, jint); void (*setChecksum)(JNIEnv*, jclass, jlong, jboolean);
    jlong (*cDirect)(JNIEnv*, jclass, jlong, jobject, jint, jint, jobject, jint, jint);
    jlong (*cArray)(JNIEnv*, jclass, jlong, jbyteArray, jint, jint, jbyteArray, jint, jint);
    void (*dictInit)(JNIEnv*, jobject, jbyteArray, jint, jint, jint); void (*dictFree)(JNIEnv*, jobject);
    jlong (*loadCDict)(JNIEnv*, jclass, jlong, jobject); jlong (*loadRawDict)(JNIEnv*, jclass, jlong, jbyteArray);
    jlong (*fastDict)(JNIEnv*, jclass, jbyteArray, jint, jbyteArray, jint, jint, jobject);
    jlong (*bound)(JNIEnv*, jclass, jlong);
    jlong (*osCreate)(JNIEnv*, jclass); jint (*osFree)(JNIEnv*, jclass, jlong); jint (*osReset)(JNIEnv*, jobject, jlong);
    jint (*osComp)(JNIEnv*, jobject, jlong, jbyteArray, jint, jbyteArray, jint); jint (*osFlush)(JNIEnv*, jobject, jlong, jbyteArray, jint); jint (*osEnd)(JNIEnv*, jobject, jlong, jbyteArray, jint);
    jint (*setStreamLevel)(JNIEnv*, jclass, jlong, jint);
    jlong (*dsCreate)(JNIEnv*, jclass); jlong (*dsFree)(JNIEnv*, jclass, jlong); jlong (*dsInit)(JNIEnv*, jobject, jlong, jint);
    jlong (*dsComp)(JNIEnv*, jobject, jlong, jobject, jint, jint, jobject, jint, jint); jlong (*dsFlush)(JNIEnv*, jobject, jlong, jobject, jint, jint); jlong (*dsEnd)(JNIEnv*, jobject, jlong, jobject, jint, jint);
} Lib;
static int load(Lib* L, const char* path) {
    memset(L, 0, sizeof *L);
    L->h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!L->h) { fprintf(stderr, "dlopen %s: %s\n", path, dlerror()); return 0; }
#define S(field, name) *(void**)&L->field = dlsym(L->h, P name)
    S(cinit, "ZstdCompressCtx_init"); S(cfree, "ZstdCompressCtx_free"); S(setLevel, "ZstdCompressCtx_setLevel0"); S(setChecksum, "ZstdCompressCtx_setChecksum0");
    S(cDirect, "ZstdCompressCtx_compressDirectByteBuffer0"); S(cArray, "ZstdCompressCtx_compressByteArray0");
    S(dictInit, "ZstdDictCompress_init"); S(dictFree, "ZstdDictCompress_free"); S(loadCDict, "ZstdCompressCtx_loadCDictFast0"); S(loadRawDict, "ZstdCompressCtx_loadCDict0");
    S(fastDict, "Zstd_compressFastDict0"); S(bound, "Zstd_compressBound");
    S(osCreate, "ZstdOutputStreamNoFinalizer_createCStream"); S(osFree, "ZstdOutputStreamNoFinalizer_freeCStream"); S(osReset, "ZstdOutputStreamNoFinalizer_resetCStream");
    S(osComp, "ZstdOutputStreamNoFinalizer_compressStream"); S(osFlush, "ZstdOutputStreamNoFinalizer_flushStream"); S(osEnd, "ZstdOutputStreamNoFinalizer_endStream");
    S(setStreamLevel, "Zstd_setCompressionLevel");
    S(dsCreate, "ZstdDirectBufferCompressingStreamNoFinalizer_createCStream"); S(dsFree, "ZstdDirectBufferCompressingStreamNoFinalizer_freeCStream");
    S(dsInit, "ZstdDirectBufferCompressingStreamNoFinalizer_initCStream"); S(dsComp, "ZstdDirectBufferCompressingStreamNoFinalizer_compressDirectByteBuffer");
    S(dsFlush, "ZstdDirectBufferCompressingStreamNoFinalizer_flushStream"); S(dsEnd, "ZstdDirectBufferCompressingStreamNoFinalizer_endStream");
#undef S
    void** f = (void**)&L->cinit;
    for (size_t i = 0; i < (sizeof *L - sizeof L->h) / sizeof(void*); i++) if (!f[i]) { fprintf(stderr, "%s: native %zu missing\n", path, i); return 0; }
    return 1;
}

static uint64_t g_x = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(void) { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (uint32_t)(g_x >> 11); }
static void fill(char* p, jsize n) {           /* records with shared words: matches against the dictionary and inside the source */
    static const char* const w[] = { "{\"id\":", "\"name\":\"", "alpha", "beta", "gamma", "\",\"value\":", "}\n", "compress", "level", "delta" };
    for (jsize i = 0; i < n; ) { const char* s = w[rnd() % 10]; for (; *s && i < n; s++) p[i++] = (rnd() % 23 == 0) ? (char)(rnd() & 0xFF) : *s; }
}
static int g_bad, g_checks;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { if (g_bad++ < 12) { fprintf(stderr, "differs: "); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

/* one ZstdOutputStream frame (the Java class's write / flush / close loops): bytes into out, returns the size or a negative error */
static long os_frame(Lib* L, JNIEnv* e, jint level, Obj* src, jsize total, jsize chunk, int flushEvery, char* out) {
    Obj* self = mk(7, 0); Obj* dst = mk(2, 131591); long n = 0; jint r; int calls = 0;
    jlong const h = L->osCreate(e, NULL);
    if ((r = L->setStreamLevel(e, NULL, h, level)) < 0 || (r = L->osReset(e, (jobject)self, h)) < 0) return r;
    for (jsize at = 0; at < total; at += chunk) {
        jsize const len = total - at < chunk ? total - at : chunk;
        self->srcPos = at;
        while (self->srcPos < at + len) { if ((r = L->osComp(e, (jobject)self, h, (jbyteArray)dst, dst->len, (jbyteArray)src, at + len)) < 0) return r; memcpy(out + n, dst->data, (size_t)self->dstPos); n += (long)self->dstPos; }
        if (flushEvery && ++calls % flushEvery == 0)
            do { if ((r = L->osFlush(e, (jobject)self, h, (jbyteArray)dst, dst->len)) < 0) return r; memcpy(out + n, dst->data, (size_t)self->dstPos); n += (long)self->dstPos; } while (r > 0);
    }
    do { if ((r = L->osEnd(e, (jobject)self, h, (jbyteArray)dst, dst->len)) < 0) return r; memcpy(out + n, dst->data, (size_t)self->dstPos); n += (long)self->dstPos; } while (r > 0);
    L->osFree(e, NULL, h);
    return n;
}
/* one ZstdDirectBufferCompressingStream frame */
static long ds_frame(Lib* L, JNIEnv* e, jint level, Obj* src, jsize total, jsize chunk, int flushEvery, char* out) {
    Obj* self = mk(7, 0); Obj* dst = mk(1, 131591); long n = 0; jlong r; int calls = 0;
    jlong const h = L->dsCreate(e, NULL);
    if ((r = L->dsInit(e, (jobject)self, h, level)) < 0) return (long)r;
    for (jsize at = 0; at < total; ) {
        jsize const len = total - at < chunk ? total - at : chunk;
        jsize done = 0;
        while (done < len) {
            Obj sub = *src; sub.data = src->data + at + done; sub.len = len - done;
            if ((r = L->dsComp(e, (jobject)self, h, (jobject)dst, 0, dst->len, (jobject)&sub, 0, len - done)) < 0) return (long)r;
            memcpy(out + n, dst->data, (size_t)self->produced); n += self->produced; done += self->consumed;
        }
        at += len;
        if (flushEvery && ++calls % flushEvery == 0)
            do { if ((r = L->dsFlush(e, (jobject)self, h, (jobject)dst, 0, dst->len)) < 0) return (long)r; memcpy(out + n, dst->data, (size_t)self->produced); n += self->produced; } while (r > 0);
    }
    do { if ((r = L->dsEnd(e, (jobject)self, h, (jobject)dst, 0, dst->len)) < 0) return (long)r; memcpy(out + n, dst->data, (size_t)self->produced); n += self->produced; } while (r > 0);
    L->dsFree(e, NULL, h);
    return n;
}

int main(int argc, char** argv) {
    typedef void (*stats_fn)(unsigned long long*);
    Lib R, G; JNIEnv* e = env();
    if (argc < 3) { fprintf(stderr, "usage: %s <ref-jni.so> <shim.so>\n", argv[0]); return 2; }
    if (!load(&R, argv[1]) || !load(&G, argv[2])) return 2;
    stats_fn st = (stats_fn)dlsym(G.h, "zjni_shim_stats");
    if (!st) { fprintf(stderr, "zjni_shim_stats missing\n"); return 2; }
    static const jint levels[] = { -1, -3, -7, -100, -200000 };
    static const jsize sizes[] = { 0, 1, 100, 4096, 8192, 8193, 20000, 70000, 131072 };
    unsigned long long s0[4]; st(s0);
    jsize const dlen = 30000;                                     /* content > 128 KiB / 6: every source up to one block keeps the dictionary's parameters */
    Obj* darr = mk(2, dlen); fill(darr->data, dlen);
    for (size_t li = 0; li < sizeof levels / sizeof *levels; li++) {
        jint const level = levels[li];
        Obj* robj = mk(7, 0); Obj* gobj = mk(7, 0);
        R.dictInit(e, (jobject)robj, (jbyteArray)darr, 0, dlen, level); G.dictInit(e, (jobject)gobj, (jbyteArray)darr, 0, dlen, level);
        CHECK(robj->field && gobj->field, "ZstdDictCompress(dict, %d)", level);
        jlong rc = R.cinit(e, NULL), gc = G.cinit(e, NULL), rl = R.cinit(e, NULL), gl = G.cinit(e, NULL);
        CHECK(R.loadCDict(e, NULL, rc, (jobject)robj) == G.loadCDict(e, NULL, gc, (jobject)gobj), "loadCDictFast0 %d", level);
        R.setLevel(e, NULL, rl, level); G.setLevel(e, NULL, gl, level);                    /* ZstdCompressCtx.setLevel(-N).loadDict(byte[]) */
        CHECK(R.loadRawDict(e, NULL, rl, (jbyteArray)darr) == G.loadRawDict(e, NULL, gl, (jbyteArray)darr), "loadCDict0 %d", level);
        for (size_t si = 0; si < sizeof sizes / sizeof *sizes; si++) for (int kind = 1; kind <= 2; kind++) {
            jsize const n = sizes[si], cap = (jsize)R.bound(e, NULL, n) + 16;
            Obj* src = mk(kind, n + 4); Obj* a = mk(kind, cap); Obj* b = mk(kind, cap);
            fill(src->data + 2, n);
            if ((si + (size_t)kind) & 1) { R.setChecksum(e, NULL, rc, JNI_TRUE); G.setChecksum(e, NULL, gc, JNI_TRUE); }
            else { R.setChecksum(e, NULL, rc, JNI_FALSE); G.setChecksum(e, NULL, gc, JNI_FALSE); }
            jlong const ra = kind == 1 ? R.cDirect(e, NULL, rc, (jobject)a, 3, cap - 3, (jobject)src, 2, n) : R.cArray(e, NULL, rc, (jbyteArray)a, 3, cap - 3, (jbyteArray)src, 2, n);
            jlong const rb = kind == 1 ? G.cDirect(e, NULL, gc, (jobject)b, 3, cap - 3, (jobject)src, 2, n) : G.cArray(e, NULL, gc, (jbyteArray)b, 3, cap - 3, (jbyteArray)src, 2, n);
            CHECK(ra == rb && ra > 0 && !memcmp(a->data, b->data, (size_t)ra + 3), "ctx + ZstdDictCompress level %d size %d kind %d: reference %lld, shim %lld", level, n, kind, (long long)ra, (long long)rb);
            jlong const la = kind == 1 ? R.cDirect(e, NULL, rl, (jobject)a, 0, cap, (jobject)src, 2, n) : R.cArray(e, NULL, rl, (jbyteArray)a, 0, cap, (jbyteArray)src, 2, n);
            jlong const lb = kind == 1 ? G.cDirect(e, NULL, gl, (jobject)b, 0, cap, (jobject)src, 2, n) : G.cArray(e, NULL, gl, (jbyteArray)b, 0, cap, (jbyteArray)src, 2, n);
            CHECK(la == lb && la > 0 && !memcmp(a->data, b->data, (size_t)la), "ctx + byte[] dictionary level %d size %d kind %d: reference %lld, shim %lld", level, n, kind, (long long)la, (long long)lb);
            if (kind == 2) {                                                               /* Zstd.compress(dst, src, ZstdDictCompress) */
                jlong const fa = R.fastDict(e, NULL, (jbyteArray)a, 1, (jbyteArray)src, 2, n, (jobject)robj), fb = G.fastDict(e, NULL, (jbyteArray)b, 1, (jbyteArray)src, 2, n, (jobject)gobj);
                CHECK(fa == fb && fa > 0 && !memcmp(a->data, b->data, (size_t)fa + 1), "compressFastDict0 level %d size %d: reference %lld, shim %lld", level, n, (long long)fa, (long long)fb);
            }
            free(src->data); free(a->data); free(b->data); free(src); free(a); free(b);
        }
        R.cfree(e, NULL, rc); G.cfree(e, NULL, gc); R.cfree(e, NULL, rl); G.cfree(e, NULL, gl);
        R.dictFree(e, (jobject)robj); G.dictFree(e, (jobject)gobj);
    }
    {   /* streams at -N: totals up to the 512 KiB window, writes of several sizes, flushes */
        static const jsize totals[] = { 0, 1, 5000, 131072, 200000, 524288 };
        for (size_t ti = 0; ti < sizeof totals / sizeof *totals; ti++) for (int variant = 0; variant < 3; variant++) {
            jsize const total = totals[ti]; jint const level = levels[(ti + (size_t)variant) % 5];
            jsize const chunk = variant == 0 ? 50000 : (variant == 1 ? 131072 : 7000); int const flushEvery = variant == 2 ? 3 : 0;
            Obj* src = mk(2, total + 1); fill(src->data, total);
            char* a = (char*)malloc((size_t)total * 2 + 65536); char* b = (char*)malloc((size_t)total * 2 + 65536);
            long const ra = os_frame(&R, e, level, src, total, chunk, flushEvery, a), rb = os_frame(&G, e, level, src, total, chunk, flushEvery, b);
            CHECK(ra == rb && ra > 0 && !memcmp(a, b, (size_t)ra), "ZstdOutputStream level %d total %d writes %d flush every %d: reference %ld, shim %ld", level, total, chunk, flushEvery, ra, rb);
            src->kind = 1;
            long const da = ds_frame(&R, e, level, src, total, chunk, flushEvery, a), db = ds_frame(&G, e, level, src, total, chunk, flushEvery, b);
            CHECK(da == db && da > 0 && !memcmp(a, b, (size_t)da), "ZstdDirectBufferCompressingStream level %d total %d writes %d flush every %d: reference %ld, shim %ld", level, total, chunk, flushEvery, da, db);
            free(a); free(b); free(src->data); free(src);
        }
    }
    unsigned long long s1[4]; st(s1);
    unsigned long long const served = s1[0] - s0[0], policy = s1[1] - s0[1], declined = s1[2] - s0[2];
    printf("checks %d, differing %d, answered by the GPU %llu, forwarded by policy %llu, forwarded after a refusal %llu\n", g_checks, g_bad, served, policy, declined);
    if (g_bad || !served || policy || declined) { printf("NEGATIVE-DICT-STREAM FAILED\n"); return 1; }
    printf("NEGATIVE-DICT-STREAM OK\n");
    return 0;
}
