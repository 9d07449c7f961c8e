// hastar_smooth.h — records and launch wrappers of hastar_smooth.hip: the exact squared
// Euclidean distance transform of a planner's occupancy map (the clearance field) and the
// batched gradient path smoother that reads it.  Float planners only.
#pragma once
#include <hip/hip_runtime.h>

namespace hastar {

constexpr int EDT_ROW_NONE = 0x3fffffff;  // pass A: no occupied cell in this map row
constexpr int EDT_MAX_N = 32768;          // 2 (N - 1)^2 must fit int32
constexpr int SMOOTH_THREADS = 256;

// one map of a clearance-field launch: occupancy in, squared distances out (N x N each)
struct EdtMap {
  const float* occ;
  int* dst;
  float thr;
  int pad;
};

// one planner of a smoothing launch: its map, its clearance field and its grid frame
struct SmoothMap {
  const float* occ;
  const int* d2;
  int N;
  float res, thr;
  float rot_c, rot_s, world_goal_x, world_goal_y, goal_x, goal_y;
  float kappa_max;
};

// hastar_smooth_opts with the defaults filled in and the constants derived on the host
struct SmoothParams {
  float ws2, wo2, wf2;  // 2 x the weights (the gradients' common factor)
  float alpha;          // 1 / (32 w_smooth + 4 w_obs + 2 w_fid)
  float d_max;
  int iterations;
};

hipError_t launch_edt(const EdtMap* d_maps, int nmaps, int N, int* d_stacks, hipStream_t st);
hipError_t launch_smooth(const SmoothMap* d_maps, const int* d_map_of, const long long* d_off, int p0, int np,
                         int max_points, const float* xyh, const float* curv, const signed char* dir, float* xyh_out,
                         float* curv_out, float* g0, float* blend, int* status, const SmoothParams& sp,
                         hipStream_t st);

}  // namespace hastar
