// bounded.hip — the status block of the bounded window forward (include/splatraster.h): a device-resident copy the kernels of a
// bounded sequence and the gated Adam launch read, and a host-mapped coherent mirror the host reads without waiting for a stream.
// The kernels that write it live with the front end they belong to (binsort.hip: bounded_publish).
#include <string.h>

#include "common.h"

namespace sr {

// both copies, in stream order: behind it a bounded sequence has its own capacity again and the gated Adam launches run
__global__ void bounded_clear_kernel(uint32_t* __restrict__ status, uint32_t* __restrict__ mirror)
{
    const int t = threadIdx.x;
    if (t >= BOUNDED_WORDS) return;
    status[t] = 0u;
    __hip_atomic_store(mirror + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int launch_bounded_status_clear(const BoundedStatus& st, hipStream_t stream)
{
    hipLaunchKernelGGL(bounded_clear_kernel, dim3(1), dim3(WAVE), 0, stream, st.dev, st.host_dev);
    SR_LAUNCH_CHECK();
    return SPLATRASTER_OK;
}

}  // namespace sr

using namespace sr;

extern "C" {

int splatraster_bounded_status_create(void** handle)
{
    if (!handle) return SPLATRASTER_ERR_BAD_ARG;
    *handle = nullptr;
    static_assert(sizeof(splatraster_bounded_status) == BOUNDED_WORDS * sizeof(uint32_t), "the status block is 64 bytes");
    BoundedStatus st{};
    SR_HIP_CHECK(hipGetDevice(&st.device));
    SR_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&st.dev), sizeof(splatraster_bounded_status)));
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&st.host), sizeof(splatraster_bounded_status),
                                 hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&st.host_dev), st.host, 0);
    if (e == hipSuccess) e = hipMemset(st.dev, 0, sizeof(splatraster_bounded_status));
    if (e != hipSuccess) {
        set_hip_error(e, "bounded status allocation");
        if (st.host) (void)hipHostFree(st.host);
        (void)hipFree(st.dev);
        return SPLATRASTER_ERR_HIP;
    }
    memset(st.host, 0, sizeof(splatraster_bounded_status));
    *handle = new BoundedStatus(st);
    return SPLATRASTER_OK;
}

int splatraster_bounded_status_destroy(void* handle)
{
    if (!handle) return SPLATRASTER_OK;
    BoundedStatus* st = reinterpret_cast<BoundedStatus*>(handle);
    (void)hipHostFree(st->host);
    (void)hipFree(st->dev);
    delete st;
    return SPLATRASTER_OK;
}

int splatraster_bounded_status_read(const void* handle, splatraster_bounded_status* out)
{
    if (!handle || !out) return SPLATRASTER_ERR_BAD_ARG;
    const uint32_t* h = reinterpret_cast<const BoundedStatus*>(handle)->host;
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    // The order of the copy is the contract (include/splatraster.h): last_tag, THEN overflow, THEN the record.  Every sequence in
    // front of `last_tag` has finished, so a clear flag read after it says that none of them overflowed; a set flag read before
    // the record comes with its record (the device stores the flag last).
    o[BOUNDED_LAST_TAG] = __atomic_load_n(h + BOUNDED_LAST_TAG, __ATOMIC_ACQUIRE);
    o[BOUNDED_OVERFLOW] = __atomic_load_n(h + BOUNDED_OVERFLOW, __ATOMIC_ACQUIRE);
    for (int k = 0; k < BOUNDED_WORDS; ++k)
        if (k != BOUNDED_OVERFLOW && k != BOUNDED_LAST_TAG) o[k] = __atomic_load_n(h + k, __ATOMIC_RELAXED);
    return SPLATRASTER_OK;
}

int splatraster_bounded_status_clear(void* handle, void* stream)
{
    if (!handle) return SPLATRASTER_ERR_BAD_ARG;
    BoundedStatus* st = reinterpret_cast<BoundedStatus*>(handle);
    // The clear itself is the kernel, in stream order.  The host zeroes the mirror at once as well: a caller that has
    // synchronised the stream (the replay of an overflow) then reads a clear block straight away, not the old record until
    // the kernel has run; work still in front of the kernel only ever re-raises what the kernel then clears.
    for (int k = 0; k < BOUNDED_WORDS; ++k) __atomic_store_n(st->host + k, 0u, __ATOMIC_RELAXED);
    return launch_bounded_status_clear(*st, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
