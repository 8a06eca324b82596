// errors.cpp -- the error message behind moe_last_error, and the entry points that belong to no net and no plan.
#include "net.h"

#include <cstdarg>

using namespace moe;

static thread_local std::string g_err;

int moe::fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int moe::launched(const char* who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MOE_EHIP, "%s launch failed: %s", who, hipGetErrorString(e));
    return MOE_OK;
}

extern "C" {

const char* moe_last_error(void) { return g_err.c_str(); }
int moe_abi_version(void) { return MOE_ABI_VERSION; }
int moe_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int moe_device_info(int device, int64_t info[8])
{
    if (!info) return fail(MOE_EINVAL, "moe_device_info: NULL argument");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    int wall = 0;
    (void)hipDeviceGetAttribute(&wall, hipDeviceAttributeWallClockRate, device);
    const int64_t v[8] = {p.multiProcessorCount, p.clockRate, p.memoryClockRate, p.memoryBusWidth, p.l2CacheSize, (int64_t)p.totalGlobalMem, wall,
                          (int64_t)p.maxSharedMemoryPerMultiProcessor};
    memcpy(info, v, sizeof v);
    return MOE_OK;
}

}  // extern "C"
