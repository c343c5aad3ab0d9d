// What instances_shared_update.hip (the device-side instance update) and instances_shared_rebuild.hip (the device re-build of the top level)
// share: the device tables' record layouts, the status block and the entry points each has for the other.
#pragma once
#include "hr_internal.h"
#include "instance_math.h"

namespace hr {

struct MeshTab { float bounds[6], absmax[3]; uint32_t root, tri_base, pad; };
static_assert(sizeof(MeshTab) == 48, "MeshTab must be 48 bytes");

// device block, mirrored into pinned host memory on demand
struct DeviceUpdateStatus
{
    uint32_t acc_lo[3], acc_hi[3];   // ordered-uint min / max of the instance boxes, folded by the record kernel, consumed and reset by the refit
    uint32_t acc_rejected, acc_violated;
    float    bounds[6];              // of the last update: measured, or as given
    float    pad;
    uint32_t rejected, violated, any_box;
    double   area;                   // sum of the top-level nodes' half areas after the last update or re-build
    double   baseline;               // that sum after the last device re-build: what top_cost_ratio and the threshold compare against
    uint32_t rebuild_flag;           // set by an update's refit when area / baseline exceeds the threshold; cleared by the re-build's refit
    uint32_t rebuilds_done;          // counted device re-builds that ran
};
static_assert(sizeof(DeviceUpdateStatus) == 96, "DeviceUpdateStatus layout");

// modes of the top-level refit (instances_shared_update.hip)
enum { kRefitUpdate = 0,           // an update: bounds / pad from the call or the accumulators, the whole status block written
       kRefitRebuildCounted = 1,   // the tail of a device re-build: bounds / pad of the last update (status block); area becomes the baseline
       kRefitRebuildQuiet = 2 };   // the same, not counted in rebuilds_done (the re-build that only brings a scene to the fixed shape)

// instances_shared_update.hip
hr_status shared_device_work_ensure(hr_scene* s);
hr_status shared_device_refit_enqueue(hr_scene* s, hipStream_t st, int mode, bool predicated);   // over the scene's standing shared_top / shared_depth_start
hr_status shared_device_status_refresh(const hr_scene* s);                                        // status_host follows the device (waits when it lags)
bool      stream_is_capturing(hipStream_t st);
// instances_shared_rebuild.hip: the whole re-build on `st`; predicated: every launch exits at once unless the status block's rebuild_flag is set
hr_status shared_device_rebuild_enqueue(hr_scene* s, hipStream_t st, const char* call, bool counted, bool predicated);

} // namespace hr
