// dev_mem.cpp — the HIP backend of dev_pool: the only calls of the runtime's allocation and free
// functions in csrc/, and the live counters' export.
#include "dev_mem.h"

#include <hip/hip_runtime.h>

#include "../../include/gemma_hpc.h"

namespace ghip {

static void *hip_alloc(mem_kind k, size_t bytes) {
    void *p = nullptr;
    const hipError_t r = k == MEM_PINNED     ? hipHostMalloc(&p, bytes, hipHostMallocDefault)
                         : k == MEM_UNCACHED ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached)
                                             : hipMalloc(&p, bytes);
    if (r != hipSuccess) (void)hipGetLastError();  // the refusal is reported by the pool, not left pending
    return r == hipSuccess ? p : nullptr;
}

static void hip_free(mem_kind k, void *p) {
    if (k == MEM_PINNED) (void)hipHostFree(p);
    else (void)hipFree(p);
}

static int hip_zero(void *p, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, 0, bytes, s) == hipSuccess ? 0 : -1; }

const mem_backend *hip_backend() {
    static const mem_backend be = {hip_alloc, hip_free, hip_zero};
    return &be;
}

}  // namespace ghip

extern "C" int gemma_hip_mem_live(int64_t *allocs, int64_t *bytes) {
    if (allocs) *allocs = ghip::g_mem_live_allocs.load();
    if (bytes) *bytes = ghip::g_mem_live_bytes.load();
    return 0;
}
