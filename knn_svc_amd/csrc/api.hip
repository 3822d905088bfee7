#include "common.h"
#include <stdlib.h>
thread_local char g_knnsvc_err[512] = "";
extern "C" int knnsvc_abi_version(void) { return KNNSVC_ABI_VERSION; }
extern "C" const char* knnsvc_last_error(void) { return g_knnsvc_err; }

// The dispatchers' knob record (common.h, KnKnobs).  Round 3 called getenv ~10 times per launch.
namespace {
KnKnobs g_knobs;
bool env_off(const char* name) { const char* e = getenv(name); return e && e[0] == '0'; }
void load_knobs() {
    KnKnobs k;
    const char* q = getenv("KNNSVC_QUAD");
    k.quad = q ? atoi(q) : 1;
    k.quad_epi = !env_off("KNNSVC_QUAD_EPI");
    const char* ep = getenv("KNNSVC_EPILOGUE");
    k.generic_epilogue = ep && ep[0] == 'g';
    k.win = !env_off("KNNSVC_WIN"); k.win_small = !env_off("KNNSVC_WIN_SMALL"); k.win_deep = !env_off("KNNSVC_WIN_DEEP");
    k.win_wide = !env_off("KNNSVC_WIN_WIDE");
    k.win160 = !env_off("KNNSVC_WIN160"); k.gemm_small = !env_off("KNNSVC_GEMM_SMALL");
    const char* at = getenv("KNNSVC_ATTENTION");
    k.attention = !at ? 2 : (at[0] == 'b') ? 3 : (at[0] == 'f' && at[1] == 'p') ? 0 : 2;
    const char* rp = getenv("KNNSVC_CONV0_RP");
    k.conv0_rp = rp ? atoi(rp) : 2;
    if (k.conv0_rp != 1 && k.conv0_rp != 4) k.conv0_rp = 2;
    const char* su = getenv("KNNSVC_CONV0_SUBS");
    k.conv0_subs = su ? atoi(su) : 8;
    if (k.conv0_subs < 1 || k.conv0_subs > 64) k.conv0_subs = 8;
    k.loaded = true;
    g_knobs = k;
}
}  // namespace
const KnKnobs& kn_knobs() { if (!g_knobs.loaded) load_knobs(); return g_knobs; }
extern "C" int knnsvc_reload_knobs(void) { load_knobs(); return KNNSVC_OK; }

// Stream-placement probe (knn_svc_amd/pipeline.py: streams_overlap): a launch of `blocks` one-wave workgroups that do nothing but
// spin for `spin` shader-clock ticks each — its duration is set by how fast the stream's hardware queue gets workgroups onto CUs
// beside whatever else is being dispatched, which is what two streams of a pipeline compete for.
namespace {
__global__ __launch_bounds__(64) void probe_dispatch_kernel(int spin, int* sink) {
    const long long t0 = __builtin_amdgcn_s_memtime();
    while (__builtin_amdgcn_s_memtime() - t0 < spin) {}
    if (sink && threadIdx.x == 4096) *sink = 1;
}
}  // namespace
extern "C" int knnsvc_probe_dispatch(int32_t blocks, int32_t spin, void* stream) {
    KN_REQUIRE(blocks > 0 && blocks <= (1 << 22) && spin >= 0, "probe_dispatch: bad sizes");
    hipLaunchKernelGGL(probe_dispatch_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, spin, (int*)nullptr);
    return knnsvc_check_launch("probe_dispatch");
}
