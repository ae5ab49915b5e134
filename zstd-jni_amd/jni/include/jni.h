/* zstd-jni_amd/jni/include/jni.h — the part of the Java Native Interface that zjni_shim.c and tests/jni/harness.c use, declared
 * from the JNI specification ("JNI Functions": every function's index in the interface function table), so that the shim and
 * the harness build on any machine, JDK or not.  The JNIEnv table keeps the specification's layout: a used function sits at its
 * index, the slots between are padding.  A library built against a full <jni.h> sees the same offsets (checked below).
 * Linux, LP64 and ILP32 as the JDK's jni_md.h declares them. */
#ifndef ZJNI_JNI_H
#define ZJNI_JNI_H

#include <stdarg.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JNIEXPORT __attribute__((visibility("default")))
#define JNIIMPORT __attribute__((visibility("default")))
#define JNICALL

typedef int jint;
#ifdef _LP64
typedef long jlong;
#else
typedef long long jlong;
#endif
typedef signed char jbyte;
typedef unsigned char jboolean;
typedef unsigned short jchar;
typedef short jshort;
typedef float jfloat;
typedef double jdouble;
typedef jint jsize;

struct _jobject;
typedef struct _jobject* jobject;
typedef jobject jclass;
typedef jobject jstring;
typedef jobject jarray;
typedef jarray jobjectArray;
typedef jarray jbyteArray;
typedef jarray jlongArray;

struct _jfieldID;
typedef struct _jfieldID* jfieldID;
struct _jmethodID;
typedef struct _jmethodID* jmethodID;

#define JNI_FALSE 0
#define JNI_TRUE 1
#define JNI_OK 0
#define JNI_ERR (-1)
#define JNI_COMMIT 1
#define JNI_ABORT 2

struct JNINativeInterface_;
typedef const struct JNINativeInterface_* JNIEnv;

/* _pN_M: table slots N..M, functions this project does not call */
struct JNINativeInterface_ {
    void* _p0_5[6];
    jclass (JNICALL* FindClass)(JNIEnv* env, const char* name);                                                    /* 6 */
    void* _p7_20[14];
    jobject (JNICALL* NewGlobalRef)(JNIEnv* env, jobject obj);                                                     /* 21 */
    void (JNICALL* DeleteGlobalRef)(JNIEnv* env, jobject ref);                                                     /* 22 */
    void (JNICALL* DeleteLocalRef)(JNIEnv* env, jobject ref);                                                      /* 23 */
    void* _p24_27[4];
    jobject (JNICALL* NewObject)(JNIEnv* env, jclass clazz, jmethodID methodID, ...);                              /* 28 */
    void* _p29_30[2];
    jclass (JNICALL* GetObjectClass)(JNIEnv* env, jobject obj);                                                    /* 31 */
    void* _p32;
    jmethodID (JNICALL* GetMethodID)(JNIEnv* env, jclass clazz, const char* name, const char* sig);               /* 33 */
    void* _p34_93[60];
    jfieldID (JNICALL* GetFieldID)(JNIEnv* env, jclass clazz, const char* name, const char* sig);                 /* 94 */
    void* _p95_99[5];
    jint (JNICALL* GetIntField)(JNIEnv* env, jobject obj, jfieldID fieldID);                                      /* 100 */
    jlong (JNICALL* GetLongField)(JNIEnv* env, jobject obj, jfieldID fieldID);                                    /* 101 */
    void* _p102_108[7];
    void (JNICALL* SetIntField)(JNIEnv* env, jobject obj, jfieldID fieldID, jint value);                          /* 109 */
    void (JNICALL* SetLongField)(JNIEnv* env, jobject obj, jfieldID fieldID, jlong value);                        /* 110 */
    void* _p111_166[56];
    jstring (JNICALL* NewStringUTF)(JNIEnv* env, const char* bytes);                                              /* 167 */
    void* _p168_170[3];
    jsize (JNICALL* GetArrayLength)(JNIEnv* env, jarray array);                                                   /* 171 */
    void* _p172;
    jobject (JNICALL* GetObjectArrayElement)(JNIEnv* env, jobjectArray array, jsize index);                       /* 173 */
    void* _p174_175[2];
    jbyteArray (JNICALL* NewByteArray)(JNIEnv* env, jsize length);                                               /* 176 */
    void* _p177_183[7];
    jbyte* (JNICALL* GetByteArrayElements)(JNIEnv* env, jbyteArray array, jboolean* isCopy);                      /* 184 */
    void* _p185_191[7];
    void (JNICALL* ReleaseByteArrayElements)(JNIEnv* env, jbyteArray array, jbyte* elems, jint mode);             /* 192 */
    void* _p193_199[7];
    void (JNICALL* GetByteArrayRegion)(JNIEnv* env, jbyteArray array, jsize start, jsize len, jbyte* buf);        /* 200 */
    void* _p201_207[7];
    void (JNICALL* SetByteArrayRegion)(JNIEnv* env, jbyteArray array, jsize start, jsize len, const jbyte* buf);  /* 208 */
    void* _p209_211[3];
    void (JNICALL* SetLongArrayRegion)(JNIEnv* env, jlongArray array, jsize start, jsize len, const jlong* buf);  /* 212 */
    void* _p213_221[9];
    void* (JNICALL* GetPrimitiveArrayCritical)(JNIEnv* env, jarray array, jboolean* isCopy);                     /* 222 */
    void (JNICALL* ReleasePrimitiveArrayCritical)(JNIEnv* env, jarray array, void* carray, jint mode);           /* 223 */
    void* _p224_227[4];
    jboolean (JNICALL* ExceptionCheck)(JNIEnv* env);                                                              /* 228 */
    jobject (JNICALL* NewDirectByteBuffer)(JNIEnv* env, void* address, jlong capacity);                          /* 229 */
    void* (JNICALL* GetDirectBufferAddress)(JNIEnv* env, jobject buf);                                           /* 230 */
    jlong (JNICALL* GetDirectBufferCapacity)(JNIEnv* env, jobject buf);                                          /* 231 */
    void* _p232_234[3];
};

#ifdef __cplusplus
#define ZJNI_JNI_SLOT(name, index) static_assert(offsetof(struct JNINativeInterface_, name) == (index) * sizeof(void*), #name)
#else
#define ZJNI_JNI_SLOT(name, index) _Static_assert(offsetof(struct JNINativeInterface_, name) == (index) * sizeof(void*), #name)
#endif
ZJNI_JNI_SLOT(FindClass, 6); ZJNI_JNI_SLOT(NewGlobalRef, 21); ZJNI_JNI_SLOT(DeleteGlobalRef, 22); ZJNI_JNI_SLOT(DeleteLocalRef, 23);
ZJNI_JNI_SLOT(NewObject, 28); ZJNI_JNI_SLOT(GetObjectClass, 31); ZJNI_JNI_SLOT(GetMethodID, 33); ZJNI_JNI_SLOT(GetFieldID, 94);
ZJNI_JNI_SLOT(GetIntField, 100); ZJNI_JNI_SLOT(GetLongField, 101); ZJNI_JNI_SLOT(SetIntField, 109); ZJNI_JNI_SLOT(SetLongField, 110);
ZJNI_JNI_SLOT(NewStringUTF, 167); ZJNI_JNI_SLOT(GetArrayLength, 171); ZJNI_JNI_SLOT(GetObjectArrayElement, 173); ZJNI_JNI_SLOT(NewByteArray, 176);
ZJNI_JNI_SLOT(GetByteArrayElements, 184); ZJNI_JNI_SLOT(ReleaseByteArrayElements, 192); ZJNI_JNI_SLOT(GetByteArrayRegion, 200);
ZJNI_JNI_SLOT(SetByteArrayRegion, 208); ZJNI_JNI_SLOT(SetLongArrayRegion, 212); ZJNI_JNI_SLOT(GetPrimitiveArrayCritical, 222);
ZJNI_JNI_SLOT(ReleasePrimitiveArrayCritical, 223); ZJNI_JNI_SLOT(ExceptionCheck, 228); ZJNI_JNI_SLOT(NewDirectByteBuffer, 229);
ZJNI_JNI_SLOT(GetDirectBufferAddress, 230); ZJNI_JNI_SLOT(GetDirectBufferCapacity, 231);
#undef ZJNI_JNI_SLOT

#ifdef __cplusplus
}
#endif

#endif
