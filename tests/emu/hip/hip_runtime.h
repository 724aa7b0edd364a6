// Stand-in for <hip/hip_runtime.h>, TEST INFRASTRUCTURE ONLY (see ../hip_emu.h).  With tests/emu first on the include
// path the library's own .hip files compile as C++: their launchers run on the CPU and their kernels under emu::launch.
// It names what the host code of the preprocessing, statistics, covariance, resampling, histogram, Hilbert, cross-spectral,
// phase-consistency, lag, wavelet and Wilson / Granger launchers (and csrc/spy_common.h under them) uses of the runtime, nothing else; "device"
// memory is host memory and the one stream is synchronous.  Define one translation unit per emulator library: the launch log below lives in it.
#pragma once
#include "../hip_emu.h"
#include <algorithm>

using std::max;      // (device code calls the runtime's unqualified min / max)
using std::min;

typedef struct emuStream* hipStream_t;
typedef struct emuEvent* hipEvent_t;
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
enum { hipEventDisableTiming = 2 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
inline hipError_t hipMalloc(void** p, size_t bytes) { return (*p = std::malloc(bytes)) ? hipSuccess : hipErrorOutOfMemory; }
inline hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) { std::memset(dst, value, bytes); return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { static char one; *e = reinterpret_cast<hipEvent_t>(&one); return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
inline hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }

// ---- the launch log: grid, block and dynamic LDS bytes of every launch since the last reset, for the tests that assert
// workgroup counts and chosen tiles
namespace emu {
struct Launch { long long v[7]; };
inline std::vector<Launch>& launch_log() { static std::vector<Launch> log; return log; }
template <typename F>
void logged_launch(dim3 grid, dim3 block, size_t lds, F&& body) {
    launch_log().push_back(Launch{{grid.x, grid.y, grid.z, block.x, block.y, block.z, (long long)lds}});
    launch(grid, block, lds, body);
}
}  // namespace emu
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) \
    emu::logged_launch((grid), (block), (lds), [&] { kern(__VA_ARGS__); })

extern "C" void emu_launch_log_reset() { emu::launch_log().clear(); }
// copies up to `max` launches, 7 values each (grid x y z, block x y z, LDS bytes), oldest first; returns how many there are
extern "C" long long emu_launch_log(long long* rows, long long max) {
    const std::vector<emu::Launch>& log = emu::launch_log();
    for (size_t i = 0; i < log.size() && (long long)i < max; ++i) std::memcpy(rows + 7 * i, log[i].v, sizeof(log[i].v));
    return (long long)log.size();
}
