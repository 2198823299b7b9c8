// Library-level entry points of the T2I-Adapter ABI (include/minsdtf_hip_t2i.h).  The kernels share csrc/common.h with the core
// library; the error hook is this library's own (the shared objects share no state).
#include <stdarg.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_t2i.h"

static thread_local char g_err[512] = "";

void msd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int msda_abi_version(void) { return MSDA_ABI_VERSION; }
extern "C" const char* msda_last_error(void) { return g_err; }
