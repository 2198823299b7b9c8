// Library-level entry points of the resampler ABI (include/minsdtf_hip_resampler.h).  The kernel shares csrc/common.h with the core
// library; the error hook is this library's own (the shared objects share no state).
#include <stdarg.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_resampler.h"

static thread_local char g_err[512] = "";

void msd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int msdr_abi_version(void) { return MSDR_ABI_VERSION; }
extern "C" const char* msdr_last_error(void) { return g_err; }
