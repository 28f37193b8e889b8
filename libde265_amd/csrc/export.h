// export.h -- what host.hip hands k_export (k_export.hip): one launch per exported picture, all its output planes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d265 {

// One output plane.  src[0] (and src[1] for the interleaved CbCr plane) point at the window's first sample (the crop applied
// by samples on the host), rows / cols are the OUTPUT's (a semi-planar chroma row has 2 x chroma-width elements).
struct ExportPlane {
  const uint8_t* src[2];
  uint8_t* dst;
  int64_t spitch, dpitch;               // bytes
  int32_t rows, cols;
  int32_t bd;                           // bit depth of the component(s)
  int32_t semi;                         // elements alternate src[0], src[1] (Cb first)
  int32_t row_start;                    // first row of this plane in the launch's row numbering
  int32_t pad;
};

struct ExportJob {
  ExportPlane p[3];
  int32_t n_planes, total_rows;
  int32_t src16, format;                // source samples are uint16 (bit depth > 8); DE265HIP_EXPORT_*
};

// enqueues k_export on `st` with `grid` workgroups of 256 threads (grid-stride over the rows)
hipError_t launch_export(const ExportJob& J, hipStream_t st, int grid);

}  // namespace d265
