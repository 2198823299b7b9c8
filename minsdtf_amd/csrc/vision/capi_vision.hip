// Library-level entry points of the vision ABI (include/minsdtf_hip_vision.h).  The kernels share csrc/common.h with the core
// library; the error hook is this library's own (the shared objects share no state).
#include <stdarg.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_vision.h"

static thread_local char g_err[512] = "";

void msd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int msdv_abi_version(void) { return MSDV_ABI_VERSION; }
extern "C" const char* msdv_last_error(void) { return g_err; }
