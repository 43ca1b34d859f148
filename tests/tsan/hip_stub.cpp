// hip_stub.cpp -- a stand-in for the HIP runtime for the ThreadSanitizer build of the HOST side (tests/tsan/build_and_run.sh).
// "Device" memory is host memory, copies are memcpy, streams and events complete immediately, kernel launches do nothing: no result means anything, but every
// lock, condition variable, atomic and thread of the host sources (training lanes, the online manager's protocol, snapshot publication, create / destroy
// under load) runs exactly as it does on the GPU box, and TSAN watches it.  TEST INFRASTRUCTURE: never linked into the product.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>

static std::atomic<long> g_launches{ 0 };
extern "C" long hip_stub_launches() { return g_launches.load(); }

// Launch trace (tests/tsan/trace_driver.cpp; off by default, the ThreadSanitizer driver never turns it on): one line on stdout per kernel launch and per
// asynchronous fill / copy -- the kernel's registered name, grid, block, dynamic LDS bytes, and the stream by its creation index (-1: the null stream).
// (a function-local static: the kernels' registrations run before this file's own globals are built)
struct Trace { std::mutex mu; std::map<const void*, std::string> names; std::map<hipStream_t, int> streams; int n_streams = 0; };
static Trace& trace() { static Trace* t = new Trace(); return *t; }
static std::atomic<bool> g_trace{ false };
extern "C" void hip_stub_trace(int on) { g_trace.store(on != 0); }
static hipStream_t new_stream() { hipStream_t s = (hipStream_t)std::malloc(8); Trace& t = trace(); std::lock_guard<std::mutex> l(t.mu);
    t.streams[s] = t.n_streams++; return s; }
static int stream_index(Trace& t, hipStream_t s) { auto it = t.streams.find(s); return it == t.streams.end() ? -1 : it->second; }
static void trace_async(const char* what, size_t bytes, hipStream_t s) {
    if (!g_trace.load(std::memory_order_relaxed)) return;
    Trace& t = trace(); std::lock_guard<std::mutex> l(t.mu); std::printf("%s %zu s%d\n", what, bytes, stream_index(t, s));
}
struct CallConfig { dim3 grid, block; size_t lds = 0; hipStream_t stream = nullptr; };
static thread_local CallConfig t_call;

extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
hipError_t hipMalloc(void** p, size_t n) { *p = std::calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = std::calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t q) { trace_async("memcpy", n, q); std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void* d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t q) { trace_async("memset", n, q); std::memset(d, v, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = new_stream(); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { *s = new_stream(); return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s) { *s = new_stream(); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { { Trace& t = trace(); std::lock_guard<std::mutex> l(t.mu); t.streams.erase(s); } std::free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t*) { return hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, hipGraphNode_t*, char*, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)std::malloc(8); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)std::malloc(8); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { std::free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipMemGetInfo(size_t* f, size_t* t) { *f = *t = (size_t)1 << 34; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t lds, hipStream_t s) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    if (g_trace.load(std::memory_order_relaxed)) {
        Trace& t = trace(); std::lock_guard<std::mutex> l(t.mu); auto it = t.names.find(f);
        std::printf("%s grid %u,%u,%u block %u,%u,%u lds %zu s%d\n", it == t.names.end() ? "?" : it->second.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds,
                stream_index(t, s));
    }
    return hipSuccess;
}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t lds, hipStream_t s) { t_call = CallConfig{ g, b, lds, s }; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = t_call.grid; *b = t_call.block; *sh = t_call.lds; *s = t_call.stream;
    return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { static void* h = nullptr; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* name, unsigned, void*, void*, void*, void*, int*) {
    Trace& t = trace(); std::lock_guard<std::mutex> l(t.mu); t.names[host_fn] = name; }
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
}
