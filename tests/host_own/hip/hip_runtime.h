/*
 * Stand-in for <hip/hip_runtime.h>, for tests/host_own/own_check.cpp ONLY (never on the product's include path): the
 * calls csrc/lh_hip_own.h makes, over malloc, with a table of what is live.  Freeing or destroying something that is
 * not live aborts with a message; stub::fail_next_alloc makes the next allocation fail; stub::log records the order of
 * the calls that matter for LhDevBuf::reserve.
 */
#ifndef LH_STUB_HIP_RUNTIME_H
#define LH_STUB_HIP_RUNTIME_H

#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
struct ihipEvent_t { int unused; };
struct ihipStream_t { int unused; };
typedef ihipEvent_t *hipEvent_t;
typedef ihipStream_t *hipStream_t;
enum { hipEventDefault = 0, hipEventDisableTiming = 2, hipStreamDefault = 0, hipStreamNonBlocking = 1 };

namespace stub {
    inline std::map < void *, char >live;       /* handle -> 'd'evice, 'p'inned, 'e'vent, 's'tream */
    inline std::vector < std::string > log;     /* "alloc", "free", "sync" in call order */
    inline bool fail_next_alloc = false;
    inline hipError_t make(void **out, size_t bytes, char kind) {
        if (kind == 'd' || kind == 'p') {
            if (fail_next_alloc) {
                fail_next_alloc = false;
                *out = nullptr;
                return hipErrorOutOfMemory;
            }
            log.push_back("alloc");
        }
        *out = malloc(bytes ? bytes : 1);
        live[*out] = kind;
        return hipSuccess;
    }
    inline hipError_t drop(void *p, char kind, const char *call) {
        auto    it = live.find(p);
        if (it == live.end() || it->second != kind) {
            fprintf(stderr, "stub HIP: %s(%p) of something that is not live (double release, or the wrong call)\n", call, p);
            abort();
        }
        if (kind == 'd' || kind == 'p')
            log.push_back("free");
        live.erase(it);
        free(p);
        return hipSuccess;
    }
}

inline hipError_t hipMalloc(void **p, size_t bytes) { return stub::make(p, bytes, 'd'); }
inline hipError_t hipFree(void *p) { return stub::drop(p, 'd', "hipFree"); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return stub::make(p, bytes, 'p'); }
inline hipError_t hipHostFree(void *p) { return stub::drop(p, 'p', "hipHostFree"); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t * e, unsigned) { return stub::make((void **) e, sizeof(ihipEvent_t), 'e'); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return stub::drop(e, 'e', "hipEventDestroy"); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t * s, unsigned) { return stub::make((void **) s, sizeof(ihipStream_t), 's'); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return stub::drop(s, 's', "hipStreamDestroy"); }
/* (the drain of LhDevBuf::reserve: only its place in the order of calls matters) */
inline hipError_t hipStreamSynchronize(hipStream_t) { stub::log.push_back("sync"); return hipSuccess; }

#endif
