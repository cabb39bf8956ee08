// Error reporting and version of the C ABI (include/x3deval.h).
#include "eval_common.h"

static thread_local char g_err[512] = "";

void x3deval_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* x3deval_last_error(void) { return g_err; }
extern "C" int x3deval_abi_version(void) { return X3DEVAL_ABI_VERSION; }
