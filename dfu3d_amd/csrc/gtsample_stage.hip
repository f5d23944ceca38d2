// gtsample_stage.hip -- SURVEY.md §8 row f-5: OpenPCDet's ground-truth sampling augmentor (copy-paste of database
// objects into a scene), pcdet/datasets/augmentor/database_sampler.py:364-501 (`add_sampled_boxes_to_scene`,
// `__call__`), for a batch of scenes.  The host has drawn every scene's candidates already (the RNG part does not depend
// on the collision results); what is left runs here:
//
// k_gts_collide, one workgroup per scene.  The scene's boxes -- its ground truths first, then the candidates grouped by
// class group in SAMPLE_GROUPS order -- go to LDS as Rect.  Group by group, a candidate is accepted iff its BEV overlap
// is 0 with every box in `existed` (the ground truths plus the candidates accepted in earlier groups) and with every
// other candidate of its group, accepted or not (database_sampler.py:469-480).  The pairs of a group are spread over the
// workgroup's threads and every hit ORs into the candidate's LDS flag; the accepted candidates are then appended to
// `existed` in candidate order.  The overlap is the exact area of rect_overlap.hpp (the one dfu3d_boxes_bev returns), in
// float32 from the float32-rounded boxes.  The reference's `iou1 = iou2` for an empty `existed` (:477) changes no
// decision: then valid = (2 * max iou2 == 0) = (max iou2 == 0), the same test as with no `existed` term at all.
// The workgroup also writes the scene's output boxes: all ground truths when nothing was accepted (gt_boxes_mask is not
// applied then, :498-501), else the ground truths under the mask followed by the accepted candidates (:366, :431).
//
// k_gts_count / k_gts_scan / k_gts_write: the scene's points.  Slot 0 of a scene is its pasted objects (the accepted
// candidates' rows of the resident pool, in acceptance order, xyz + float32 centre, :398-413), slots 1.. are chunks of
// PC points of the scene kept in order when they lie in none of the accepted candidates' enlarged boxes (the
// points_in_boxes_cpu test of pt_in_box.hpp, :427-430).  Count per slot, one exclusive scan over all slots of the
// batch, write: the output is one dense CSR, out_off (B+1).
#include "common.hpp"
#include "pt_in_box.hpp"
#include "rect_overlap.hpp"

namespace {

constexpr int GS_MAX = DFU3D_GT_SAMPLE_MAX_BOXES;   // boxes (ground truths + candidates) of one scene
constexpr int PT = 256;                             // threads per point workgroup
constexpr int PE = 4;                               // consecutive points per thread
constexpr int PC = PT * PE;                         // points per chunk slot

__device__ __forceinline__ void load7f(const double *b, float *f) {
#pragma unroll
  for (int k = 0; k < 7; k++) f[k] = (float)b[k];
}

__global__ __launch_bounds__(IB) void k_gts_collide(const double *__restrict__ boxes, const int *__restrict__ box_off,
                                                    const int *__restrict__ gt_cnt, const int *__restrict__ grp,
                                                    const int *__restrict__ gt_mask, int *__restrict__ accept,
                                                    double *__restrict__ out_boxes, int *__restrict__ out_src,
                                                    int *__restrict__ out_cnt, uint32_t *__restrict__ status) {
  __shared__ float s_poly[4][MAXV * IB];
  __shared__ Rect s_r[GS_MAX];
  __shared__ int s_g[GS_MAX];
  __shared__ int s_hit[GS_MAX];
  __shared__ int s_e[GS_MAX];                        // rows of `existed`, in order
  __shared__ int s_w[IB / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const int r0 = box_off[b], n = box_off[b + 1] - r0, ng = gt_cnt[b];
  if (n > GS_MAX || ng > n || ng < 0) {              // the host checks this; never index LDS beyond it
    for (int i = t; i < n; i += IB) accept[r0 + i] = 0;
    if (t == 0) { out_cnt[b] = 0; atomicOr(status, DFU3D_ST_BOX_RANGE); }
    return;
  }
  for (int i = t; i < n; i += IB) {
    float f[7];
    load7f(boxes + (size_t)(r0 + i) * 7, f);
    s_r[i] = make_rect(f, 7);
    s_g[i] = grp[r0 + i];
    s_hit[i] = 0;
    if (i < ng) s_e[i] = i;
  }
  __syncthreads();
  float *pu = s_poly[0] + t, *pv = s_poly[1] + t, *qu = s_poly[2] + t, *qv = s_poly[3] + t;
  int ne = ng;
  for (int c0 = ng; c0 < n;) {
    int c1 = c0 + 1;
    while (c1 < n && s_g[c1] == s_g[c0]) c1++;       // the group's candidates: [c0, c1)
    const int m = c1 - c0, E = ne;
    const int p1 = m * E, ptot = p1 + m * m;
    for (int p = t; p < ptot; p += IB) {
      if (p < p1) {                                   // candidate against `existed`
        const int i = c0 + p / E, k = s_e[p % E];
        if (overlap_area(s_r[i], s_r[k], pu, pv, qu, qv) > 0.0f) s_hit[i] = 1;
      } else {                                        // candidate pair of the group, each pair once
        const int q = p - p1, i = c0 + q / m, j = c0 + q % m;
        if (j > i && overlap_area(s_r[i], s_r[j], pu, pv, qu, qv) > 0.0f) { s_hit[i] = 1; s_hit[j] = 1; }
      }
    }
    __syncthreads();
    int added = 0;
    for (int i0 = c0; i0 < c1; i0 += IB) {
      const int i = i0 + t;
      const bool ok = i < c1 && !s_hit[i];
      int tot;
      const int r = block_rank<IB / 64>(ok, s_w, tot);
      if (i < c1) accept[r0 + i] = ok ? 1 : 0;
      if (ok) s_e[ne + added + r] = i;
      added += tot;
    }
    ne += added;
    __syncthreads();
    c0 = c1;
  }
  for (int i = t; i < ng; i += IB) accept[r0 + i] = 0;
  // output boxes: ground truths (under the mask iff something was accepted), then the accepted candidates
  const bool any = ne > ng;
  int kept = 0;
  for (int i0 = 0; i0 < ng; i0 += IB) {
    const int i = i0 + t;
    const bool keep = i < ng && (!any || gt_mask[r0 + i] != 0);
    int tot;
    const int r = block_rank<IB / 64>(keep, s_w, tot);
    if (keep) {
      const int d = r0 + kept + r;
      for (int k = 0; k < 7; k++) out_boxes[(size_t)d * 7 + k] = boxes[(size_t)(r0 + i) * 7 + k];
      out_src[d] = i;
    }
    kept += tot;
  }
  for (int a = t; a < ne - ng; a += IB) {
    const int i = s_e[ng + a], d = r0 + kept + a;
    for (int k = 0; k < 7; k++) out_boxes[(size_t)d * 7 + k] = boxes[(size_t)(r0 + i) * 7 + k];
    out_src[d] = i;
  }
  if (t == 0) out_cnt[b] = kept + ne - ng;
}

// The accepted candidates of scene b in acceptance order (= row order): s_row[a] = batch row; returns their number.
__device__ __forceinline__ int accepted_rows(int r0, int n, int ng, const int *__restrict__ accept, int *s_row,
                                             int *s_w) {
  int na = 0;
  for (int i0 = ng; i0 < n; i0 += PT) {
    const int i = i0 + threadIdx.x;
    const bool ok = i < n && accept[r0 + i] != 0;
    int tot;
    const int r = block_rank<PT / 64>(ok, s_w, tot);
    if (ok) s_row[na + r] = r0 + i;
    na += tot;
  }
  __syncthreads();
  return na;
}

__device__ __forceinline__ bool scene_box_ok(int n, int ng) { return n <= GS_MAX && ng >= 0 && ng <= n; }

// cnt[b * S + 0] = object points of scene b, cnt[b * S + 1 + c] = kept scene points of chunk c   (S = 1 + chunks)
__global__ __launch_bounds__(PT) void k_gts_count(const float *__restrict__ pts, int C, const long long *__restrict__ pt_off,
                                                  const int *__restrict__ box_off, const int *__restrict__ gt_cnt,
                                                  const double *__restrict__ large, const int *__restrict__ accept,
                                                  const int *__restrict__ obj_cnt, int S, int *__restrict__ cnt,
                                                  uint32_t *__restrict__ status) {
  __shared__ BoxF s_box[GS_MAX];
  __shared__ int s_row[GS_MAX];
  __shared__ int s_w[PT / 64];
  const int b = blockIdx.y, slot = blockIdx.x;
  const int r0 = box_off[b], n = box_off[b + 1] - r0, ng = gt_cnt[b];
  const long long p0 = pt_off[b];
  const long long np = pt_off[b + 1] - p0;
  if (!scene_box_ok(n, ng)) {                         // k_gts_collide flagged it; the scene comes out empty
    if (threadIdx.x == 0) cnt[(size_t)b * S + slot] = 0;
    return;
  }
  if (slot == 0 && threadIdx.x == 0 && np > (long long)(S - 1) * PC) atomicOr(status, DFU3D_ST_BOX_RANGE);
  const int na = accepted_rows(r0, n, ng, accept, s_row, s_w);
  if (slot == 0) {
    int c = 0;
    for (int a = threadIdx.x; a < na; a += PT) c += obj_cnt[s_row[a]];
    c = block_sum_i<PT / 64>(c, s_w);
    if (threadIdx.x == 0) cnt[(size_t)b * S] = c;
    return;
  }
  for (int a = threadIdx.x; a < na; a += PT) s_box[a] = load_box(large + (size_t)s_row[a] * 7);
  __syncthreads();
  const long long i0 = (long long)(slot - 1) * PC + threadIdx.x * PE;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < PE; k++) {
    if (i0 + k < np) {
      const float *p = pts + (size_t)(p0 + i0 + k) * C;
      const float x = p[0], y = p[1], z = p[2];
      bool in = false;
      for (int a = 0; a < na && !in; a++) in = pt_in_box(s_box[a], x, y, z);
      mine += in ? 0 : 1;
    }
  }
  mine = block_sum_i<PT / 64>(mine, s_w);
  if (threadIdx.x == 0) cnt[(size_t)b * S + slot] = mine;
}

// exclusive scan of the B * S slot counts -> slot_off (int64); out_off[b] = slot_off[b * S], out_off[B] = total
__global__ __launch_bounds__(1024) void k_gts_scan(int B, int S, const int *__restrict__ cnt,
                                                   long long *__restrict__ slot_off, long long *__restrict__ out_off,
                                                   long long cap, uint32_t *__restrict__ status) {
  __shared__ int s_w[16];
  const long long total = block_scan_range<1024, 1, long long, long long>(
      (long long)B * S, [&](long long s) { return cnt[s]; },
      [&](long long s, long long ex) {
        slot_off[s] = ex;
        if (s % S == 0) out_off[s / S] = ex;
      },
      s_w);
  if (threadIdx.x == 0) {
    out_off[B] = total;
    if (total > cap) atomicOr(status, DFU3D_ST_POOL_OVERFLOW);
  }
}

__global__ __launch_bounds__(PT) void k_gts_write(const float *__restrict__ pts, int C, const long long *__restrict__ pt_off,
                                                  const int *__restrict__ box_off, const int *__restrict__ gt_cnt,
                                                  const double *__restrict__ boxes, const double *__restrict__ large,
                                                  const int *__restrict__ accept, const float *__restrict__ pool,
                                                  const long long *__restrict__ obj_src, const int *__restrict__ obj_cnt,
                                                  int S, const int *__restrict__ cnt,
                                                  const long long *__restrict__ slot_off, long long cap,
                                                  float *__restrict__ out) {
  __shared__ BoxF s_box[GS_MAX];
  __shared__ int s_row[GS_MAX];
  __shared__ int s_w[PT / 64];
  const int b = blockIdx.y, slot = blockIdx.x;
  const int r0 = box_off[b], n = box_off[b + 1] - r0, ng = gt_cnt[b];
  if (!scene_box_ok(n, ng) || cnt[(size_t)b * S + slot] == 0) return;     // nothing to write in this slot
  const long long p0 = pt_off[b];
  const long long np = pt_off[b + 1] - p0;
  const long long o = slot_off[(size_t)b * S + slot];
  const int na = accepted_rows(r0, n, ng, accept, s_row, s_w);
  if (slot == 0) {
    // objects one after the other: obj_points[:, :3] += float32(box3d_lidar[:3]) in float32, all C columns
    long long d0 = o;
    for (int a = 0; a < na; a++) {
      const int row = s_row[a];
      const int m = obj_cnt[row];
      const float *src = pool + (size_t)obj_src[row] * C;
      const double *bx = boxes + (size_t)row * 7;
      const float cx = (float)bx[0], cy = (float)bx[1], cz = (float)bx[2];
      for (long long e = threadIdx.x; e < (long long)m * C; e += PT) {
        const int col = (int)(e % C);
        float v = src[e];
        v = col == 0 ? v + cx : col == 1 ? v + cy : col == 2 ? v + cz : v;
        if (d0 * C + e < cap * C) out[(size_t)(d0 * C + e)] = v;
      }
      d0 += m;
    }
    return;
  }
  for (int a = threadIdx.x; a < na; a += PT) s_box[a] = load_box(large + (size_t)s_row[a] * 7);
  __syncthreads();
  const long long i0 = (long long)(slot - 1) * PC + threadIdx.x * PE;
  bool keep[PE];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < PE; k++) {
    keep[k] = false;
    if (i0 + k < np) {
      const float *p = pts + (size_t)(p0 + i0 + k) * C;
      const float x = p[0], y = p[1], z = p[2];
      bool in = false;
      for (int a = 0; a < na && !in; a++) in = pt_in_box(s_box[a], x, y, z);
      keep[k] = !in;
    }
    mine += keep[k] ? 1 : 0;
  }
  int tot;
  int r = block_excl_scan<PT / 64>(mine, s_w, tot);
#pragma unroll
  for (int k = 0; k < PE; k++) {
    if (keep[k]) {
      const long long d = o + r;
      if (d < cap) {
        const float *p = pts + (size_t)(p0 + i0 + k) * C;
        float *q = out + (size_t)d * C;
        for (int c = 0; c < C; c++) q[c] = p[c];
      }
      r++;
    }
  }
}

}  // namespace

extern "C" int dfu3d_gt_sample_collide(const double *boxes, const int32_t *box_off, const int32_t *gt_cnt,
                                       const int32_t *grp, const int32_t *gt_mask, int32_t B, int32_t max_boxes,
                                       int32_t *accept, double *out_boxes, int32_t *out_src, int32_t *out_cnt,
                                       uint32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!boxes || !box_off || !gt_cnt || !grp || !gt_mask || !accept || !out_boxes || !out_src || !out_cnt || !status)
    return DFU3D_EINVAL;
  if (B < 0 || max_boxes < 0) return DFU3D_EINVAL;
  if (max_boxes > DFU3D_GT_SAMPLE_MAX_BOXES) return DFU3D_ERANGE;
  if (B == 0) return DFU3D_OK;
  hipLaunchKernelGGL(k_gts_collide, dim3(B), dim3(IB), 0, (hipStream_t)stream, boxes, box_off, gt_cnt, grp, gt_mask,
                     accept, out_boxes, out_src, out_cnt, status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

static int64_t gts_slots(int32_t max_scene_points) { return 1 + ((int64_t)max_scene_points + PC - 1) / PC; }

extern "C" int64_t dfu3d_gt_sample_paste_scratch_bytes(int32_t B, int32_t max_scene_points) {
  if (B < 0 || max_scene_points < 0) return -1;
  const int64_t slots = (int64_t)B * gts_slots(max_scene_points) + 1;
  return ((slots * 4 + 7) / 8) * 8 + slots * 8;
}

extern "C" int dfu3d_gt_sample_paste(const float *points, int32_t C, const int64_t *pt_off, int32_t B,
                                     int32_t max_scene_points, const int32_t *box_off, const int32_t *gt_cnt,
                                     const double *boxes, const double *large, const int32_t *accept,
                                     const float *pool, const int64_t *obj_src, const int32_t *obj_cnt,
                                     float *out, int64_t *out_off, int64_t cap_out, void *scratch, uint32_t *status,
                                     void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!points || !pt_off || !box_off || !gt_cnt || !boxes || !large || !accept || !obj_src || !obj_cnt || !out ||
      !out_off || !scratch || !status)
    return DFU3D_EINVAL;
  if (B < 0 || C < 3 || max_scene_points < 0 || cap_out < 0) return DFU3D_EINVAL;
  if ((uintptr_t)scratch & 7u) return DFU3D_EINVAL;
  if (points == out || (pool && pool == out)) return DFU3D_EINVAL;
  if (B == 0) return DFU3D_OK;
  const int64_t S = gts_slots(max_scene_points);
  if (S > 65535 || B > 65535) return DFU3D_ERANGE;
  const int64_t slots = (int64_t)B * S + 1;
  int *cnt = (int *)scratch;
  long long *slot_off = (long long *)((char *)scratch + ((slots * 4 + 7) / 8) * 8);
  hipStream_t st = (hipStream_t)stream;
  const float *pl = pool ? pool : points;            // no accepted candidate can have rows when the pool is empty
  hipLaunchKernelGGL(k_gts_count, dim3((unsigned)S, B), dim3(PT), 0, st, points, C, (const long long *)pt_off, box_off,
                     gt_cnt, large, accept, obj_cnt, (int)S, cnt, status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gts_scan, dim3(1), dim3(1024), 0, st, B, (int)S, cnt, slot_off, (long long *)out_off,
                     (long long)cap_out, status);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gts_write, dim3((unsigned)S, B), dim3(PT), 0, st, points, C, (const long long *)pt_off, box_off,
                     gt_cnt, boxes, large, accept, pl, (const long long *)obj_src, obj_cnt, (int)S, cnt, slot_off,
                     (long long)cap_out, out);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
