// register_device.h -- what the kernels of the map registrations share (register.hip: dslam_register_maps, one pair per
// launch; register_graph.hip: dslam_register_graph, every pair of a pose graph in one launch): the sizes, the parameters of
// one source read against one destination, and -- in register_body.h -- the evaluation itself.
#pragma once
#include "mesh_device.h"
#include "multimap_device.h"

namespace dslam {

// (kRegSums, the 33 sums of an evaluation: register_host.h)
constexpr int kRegGrid = 512;      // workgroups of the registration kernels: two per CU of an MI355X
constexpr int kRegThreads = 256;   // lane t takes voxels t and t + 256 of a block
constexpr int kRegWaves = kRegThreads / 64;
// the depth-to-SDF tracker's kernels (track_sdf.hip, track_sdf_starts.hip; the body of both is track_sdf_device.h)
constexpr int kTrackSdfGrid = 512;      // workgroups: two per CU of an MI355X.  512 x 256 = 131072 lanes, so a level of
                                        // more than 131072 pixels (640 x 480 has 307200) takes further trips of the loop
constexpr int kTrackSdfThreads = kRegThreads;

struct RegisterParams {
  const HashEntry *hash;     // the source
  const uint2 *voxels;
  const int *live_list;      // its resident entries, ascending
  const int *live_count;
  MultiMap dst;              // the destination read from the source's voxel frame: T = X~
  int band_raw;              // (int)(band * 32767)
  float residual_gate;
  double *partials;          // [gridDim.x][kRegSums]
};

}  // namespace dslam
