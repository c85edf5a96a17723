// lib.hip -- what belongs to the library as a whole rather than to one kernel family: the error text, the ABI version, the device check.
#include "common.h"

thread_local char g_otter_err[512] = {0};   // written by OTTER_FAIL (common.h) in every source file

extern "C" {

int otter_abi_version(void) { return OTTER_ABI_VERSION; }
const char* otter_last_error(void) { return g_otter_err; }

int otter_device_check(void) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess)
        OTTER_FAIL(OTTER_ERR_LAUNCH, "no HIP device");
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
        OTTER_FAIL(OTTER_ERR_UNSUPPORTED, "device is %s, this library is built for gfx950 only", p.gcnArchName);
    return p.multiProcessorCount;
}

}  // extern "C"
