// spt_staging.cpp -- the HIP half of spt_staging.h: the allocation behind a staging plan.
#include "spt_staging.h"

#include <hip/hip_runtime.h>

namespace spt_api {

bool Staging::alloc(const StagingPlan &p, void *stream_)
{
    plan = p;
    stream = stream_;
    if (hipMalloc((void **)&base, plan.total) != hipSuccess) base = nullptr;
    return base != nullptr;
}

Staging::~Staging()
{
    if (!base) return;
    if (!ok) (void)hipStreamSynchronize((hipStream_t)stream);  // the call's queued work uses the memory
    (void)hipFree(base);
}

}  // namespace spt_api
