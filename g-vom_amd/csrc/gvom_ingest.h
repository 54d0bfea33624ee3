// gvom_ingest.h -- launcher of the range-image pre-pass (gvom_ingest.hip), called by gvom_capi.hip only.  A header of its own:
// the scan / fusion / 2-D units never see it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct UnprojectParams {
    const void   *raw;        // range image, row-major, rows row_stride bytes apart (device memory)
    int64_t       row_stride;
    const double *dir;        // [n][3] unit directions
    const double *off;        // [n][3] offsets (metres)
    const double *poses;      // [W][12] row-major 3x4 per column, or nullptr
    void         *out;        // [n][3] cloud of the cloud type, (NaN, NaN, NaN) for invalid pixels
    double        scale, min_range, max_range;
    uint32_t      W, n;       // columns per row; pixels (H * W < 2^31)
};
#define GVOM_UNPROJECT_BLOCK 256   // pixels (= lanes) per workgroup
// range_dtype: GVOM_RANGE_*, cloud_dtype: GVOM_DTYPE_*
hipError_t gvom_launch_unproject(hipStream_t s, const UnprojectParams &P, int range_dtype, int cloud_dtype);
