// pt_in_box.hpp -- the point-in-box test of points_in_boxes_cpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:
// 121-140), shared by gtdb_stage.hip (the ground-truth database) and gtsample_stage.hip (the scene points that ground-truth
// sampling removes).  Arithmetic and its hazards: see gtdb_stage.hip's header.
#pragma once
#include "common.hpp"

namespace {

struct BoxF {
  float cx, cy, cz, cosa, sina;
  double hz, hx, hy;          // dz/2, dx/2 + MARGIN, dy/2 + MARGIN (double, as the reference compares)
  double c64x, c64y, c64z;    // float64 centre: gt_points[:, :3] -= gt_boxes[i, :3] (kitti_dataset.py:319)
};

__device__ __forceinline__ BoxF load_box(const double *b) {
  BoxF q;
  q.c64x = b[0]; q.c64y = b[1]; q.c64z = b[2];
  q.cx = (float)b[0]; q.cy = (float)b[1]; q.cz = (float)b[2];          // boxes.float()
  const float dx = (float)b[3], dy = (float)b[4], dz = (float)b[5], rz = (float)b[6];
  const float MARGIN = 1e-2f;
  q.cosa = (float)cos((double)(-rz));
  q.sina = (float)sin((double)(-rz));
  q.hz = (double)dz / 2.0;
  q.hx = (double)dx / 2.0 + (double)MARGIN;
  q.hy = (double)dy / 2.0 + (double)MARGIN;
  return q;
}

// The same box from float32 (x, y, z, dx, dy, dz, heading) with the margin of the caller's op (roipoint_stage.hip: 1e-5f)
// and its enlargement of the dims, added in float32 as box_utils.enlarge_box3d does.  The float64 centre is the float one.
__device__ __forceinline__ BoxF load_box_f32(const float *b, float margin, float ex, float ey, float ez) {
  BoxF q;
  q.cx = b[0]; q.cy = b[1]; q.cz = b[2];
  q.c64x = (double)q.cx; q.c64y = (double)q.cy; q.c64z = (double)q.cz;
  const float dx = b[3] + ex, dy = b[4] + ey, dz = b[5] + ez, rz = b[6];
  q.cosa = (float)cos((double)(-rz));
  q.sina = (float)sin((double)(-rz));
  q.hz = (double)dz / 2.0;
  q.hx = (double)dx / 2.0 + (double)margin;
  q.hy = (double)dy / 2.0 + (double)margin;
  return q;
}

__device__ __forceinline__ bool pt_in_box(const BoxF &q, float x, float y, float z) {
  if ((double)fabsf(z - q.cz) > q.hz) return false;
  const float sx = x - q.cx, sy = y - q.cy;
  const float lx = sx * q.cosa + sy * (-q.sina);
  const float ly = sx * q.sina + sy * q.cosa;
  return ((double)fabsf(lx) < q.hx) && ((double)fabsf(ly) < q.hy);
}

}  // namespace
