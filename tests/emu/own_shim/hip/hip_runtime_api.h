// TEST INFRASTRUCTURE: the declarations crbm_amd/csrc/crbm_own.h needs of the HIP runtime, for tests/emu/own_main.cpp,
// which defines every one of them as a counting stand-in.  Never shipped, never linked against the HIP runtime.
#pragma once
#include <stddef.h>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
typedef struct ihipModule_t* hipModule_t;
struct hipIpcMemHandle_t { char reserved[64]; };
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipDeviceMallocFinegrained = 1, hipIpcMemLazyEnablePeerAccess = 1 };

hipError_t hipMalloc(void** p, size_t bytes);
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned flags);
hipError_t hipMemset(void* p, int value, size_t bytes);
hipError_t hipFree(void* p);
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipEventCreate(hipEvent_t* e);
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipModuleLoadData(hipModule_t* m, const void* image);
hipError_t hipModuleUnload(hipModule_t m);
hipError_t hipIpcOpenMemHandle(void** p, hipIpcMemHandle_t handle, unsigned flags);
hipError_t hipIpcCloseMemHandle(void* p);
