// Error reporting and version of the C ABI (include/x3ddata.h).
#include "data_common.h"

static thread_local char g_err[512] = "";

void x3ddata_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* x3ddata_last_error(void) { return g_err; }
extern "C" int x3ddata_abi_version(void) { return X3DDATA_ABI_VERSION; }
extern "C" size_t x3ddata_label_job_bytes(void) { return sizeof(X3DDataLabelJob); }
extern "C" size_t x3ddata_clip_job_bytes(void) { return sizeof(X3DDataClipJob); }
