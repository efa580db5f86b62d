// dslam_internal.h -- host-side objects behind the opaque handles of include/dslam_fusion.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dslam_fusion.h"
#include "dslam_device.h"
#include "dslam_memory.h"
#include "register_host.h"

namespace dslam {

void set_last_error(const std::string &msg);

#define DSLAM_HIP(call)                                                       \
  do {                                                                        \
    hipError_t _e = (call);                                                   \
    if (_e != hipSuccess) return ::dslam::hip_fail(_e, #call, __FILE__, __LINE__); \
  } while (0)

#define DSLAM_REQUIRE(cond, msg)                 \
  do {                                           \
    if (!(cond)) {                               \
      ::dslam::set_last_error(msg);              \
      return DSLAM_ERR_INVALID;                  \
    }                                            \
  } while (0)

// host inverse of a column-major 4x4 (ORUtils::Matrix4::inv); used for invM_d = pose_d->GetInvM()
bool invert_matrix(const float *m, float *dst);

// The re-integration batch (integrate.hip) as the host builds it (capi.hip) and the kernels read it: one BatchOp per
// operation -- [2k] the de-integration of keyframe k at its old pose, [2k + 1] its re-fusion at the new one ...
struct BatchOp {
  Mat4 M;                // world -> camera of this operation
  const float *depth;    // the keyframe's depth image in metres: written by the allocation pass of its re-fusion (k_mark derives
                         // it from the int16 image exactly as UpdateView does) into the batch's scratch, one image per keyframe
  const uchar4 *rgba;
  int push_bit, push_frame;  // re-fusions: the ring bit and frame stamp ProcessFrame(isDefusion) queues the block with
  int pad[2];
};
// ... and one list per operation (k_batch_mark), plus the lists whose block positions k_store_list_positions fills in
struct BatchListRef {
  const RenderCounters *count;   // header of the list (no_visible = its length)
  const int *ids;
  const short4 *pos;             // stored lists: the block each entry held at fusion time; null: a fresh list
};

// scratch shared by all scenes of an engine, sized for the largest scene seen (ensure_scratch builds a new set aside and
// move-assigns it: buffers and sizes change together)
struct EngineScratch {
  int scratch_entries = 0;
  int scratch_local_blocks = 0;
  DeviceBuffer<unsigned> order_keys;     // [entries] mark-phase order keys; ALL ZERO between allocation passes (the pass that
                                      // sets a key clears it again, so no pass starts with a 4.7 MB memset)
  DeviceBuffer<unsigned char> alloc_type;  // [entries] entriesAllocType of the last pass (kept for the parity tests)
  DeviceBuffer<short4> block_coords;     // [entries] blockCoords
  // bit-packed summaries of an allocation pass (dslam_device.h): requests on empty bucket heads (q1) / chain ends (q2),
  // entries a pixel's walk found (mark).  Two sets used alternately: pass k sets bits in set k & 1 and zeroes set
  // (k + 1) & 1 -- the set of the pass before it -- so no pass starts with a memset; bits_dirty[s] = words of set s that
  // may be non-zero (scenes of different sizes share the sets).  retest: outcome of the frustum re-test of the entries
  // that were visible before the pass (every word is written by every pass).
  DeviceBuffer<unsigned> bits_q1[2], bits_q2[2], bits_mark[2];
  DeviceBuffer<unsigned> bits_retest;
  int bits_words = 0;                 // words per bitmap (whole tiles)
  int bits_dirty[2] = {0, 0};
  // single-pass ordered compactions: per-tile aggregates published inside one launch ({epoch, counts} in one 8-byte
  // word per tile; three channels: allocation requests, commit results, visible counts) and the launch counter that
  // tags them, so the arrays never need clearing
  DeviceBuffer<unsigned long long> agg;  // [3][agg_tiles]
  int agg_tiles = 0;
  // table writes of an allocation sweep that ran beside the previous GetImage's march, until k_publish_entries scatters them
  // (DESIGN.md 4h).  Every committed request takes one voxel-block slot and names one table entry, so a pass appends at
  // most min(local_blocks, entries) records of each kind: the lists hold that many.  pend_count: [2][2] record counts, the
  // pair of overlapped pass k at [k & 1]; the publish kernel of a pass zeroes the other pair for the next one.
  DeviceBuffer<uint4> pend_entry;        // [pend_cap] whole entries ...
  DeviceBuffer<int> pend_entry_idx;      // [pend_cap] ... and where they go
  DeviceBuffer<int2> pend_offset;        // [pend_cap] {entry, its new offset field}
  DeviceBuffer<unsigned> pend_count;     // [4], all zero between passes
  int pend_cap = 0;
  // ... and, by table entry, the block position of every entry such a sweep creates (bucket and excess alike): what a
  // selection that runs before k_publish_entries reads in place of the still empty table entry.  Only the
  // slots of entries created by the pass in flight mean anything.
  DeviceBuffer<short4> hidden_pos;       // [entries]
  DeviceBuffer<int> list_d;              // [max(local_blocks, entries)] general purpose scratch (bucket leaders, live flags)
  // release pipeline (decay / sliding window): flags that are ALL ZERO between passes (the kernels that consume a flag
  // clear it), so no pass starts with a memset
  DeviceBuffer<unsigned char> rem_flags;    // [entries] entry is being released
  DeviceBuffer<unsigned char> freed_flags;  // [entries] excess slot came free
  DeviceBuffer<unsigned char> rem_cand;     // [local_blocks] candidate i of the decay pass lost its last measured voxel
  DeviceBuffer<int> maint_flags;            // device [4]: [0] the pass took something out of a visible list
  DeviceBuffer<int> tile_counts;         // [2 * tiles] per-tile counts of the ordered compactions
  DeviceBuffer<int> tile_offsets;        // [2 * tiles]
  DeviceBuffer<int> list_a;              // [max(local_blocks, entries)] general purpose int lists
  DeviceBuffer<int> list_b;
  DeviceBuffer<int> list_c;
  DeviceBuffer<short4> pos_scratch;      // [local_blocks]
};

// dslam_merge_maps (merge.hip): what its kernels count for the host, and its own scratch -- allocated by the first call,
// grown as a whole (built aside, move-assigned), so the alternating bitmap sets of the allocation pass are left alone
struct MergeCounters {
  int live;                 // resident entries of the source
  int requests;             // slots asked for in the current pass
  int served1, served2;     // ... of them served (empty bucket heads / chain ends)
  int touched;              // destination entries to fuse into
  int pad[3];
  unsigned long long candidates, out_of_range;
  unsigned long long without_block;   // dslam_unmerge_maps: candidates whose target block the destination does not hold
};
struct MergeScratch {
  int src_entries = 0, dst_entries = 0, words = 0;
  DeviceBuffer<unsigned> keys;           // [dst_entries] order keys; ALL ZERO between calls (the serve step clears what it reads)
  DeviceBuffer<unsigned> bits;           // [4][words]: requests on empty heads, on chain ends, either; touched entries
  DeviceBuffer<int> ranks;               // [dst_entries] rank of a request among those of its type
  DeviceBuffer<int> touched_list;        // [dst_entries]
  DeviceBuffer<int> live_list;           // [src_entries]
  DeviceBuffer<MergeCounters> counters;
  PinnedBuffer<MergeCounters> counters_host;   // [2]: the merge's read-backs, the unmerge's
  PinnedBuffer<unsigned long long> changed;   // mapped: [workgroups] voxels changed, one count per workgroup of the merge's
                                              // block kernel; then [workgroups][3], one row per workgroup of the unmerge's
};
// The resident entries of several maps of one call (fill_live_lists, live_list.hip: dslam_register_graph's distinct sources,
// dslam_survey_overlaps' maps), one range of live_list per map -- allocated by the first call, grown as a whole (built
// aside, move-assigned); the list and counter slots other calls use are left alone.  One set per engine: both calls
// enqueue on the engine's one stream and wait for it before they return, so neither sees the other's lists in flight.
struct LiveLists {
  int entries = 0;                       // capacity of live_list
  DeviceBuffer<int> live_list;
  DeviceBuffer<int> live_counts;         // [DSLAM_MAX_RENDER_MAPS] entries in each range
  PinnedBuffer<int> live_counts_host;
};
// dslam_register_graph (register_graph.hip): its own scratch, allocated by the first call
struct RegisterGraphScratch {
  PinnedBuffer<double> partials;         // mapped: [workgroups][33], one row per workgroup of k_register_graph
  PinnedBuffer<void> jobs;               // mapped: the pair table and the workgroup -> pair table the kernel reads
};
// dslam_survey_overlaps (overlap.hip): its own scratch, allocated by the first call
struct OverlapScratch {
  PinnedBuffer<int> rows;                // mapped: [workgroups][2 N], one row per workgroup of k_survey_overlaps
  PinnedBuffer<void> tables_host;        // the tables of a call on their way to the device:
  DeviceBuffer<void> tables;             // workgroup -> source map, the map descriptors, the N x N pair transforms
};
// dslam_survey_views (view_survey.hip): its own scratch, allocated by the first call
struct ViewSurveyScratch {
  PinnedBuffer<void> tables_host;        // the tables of a call on their way to the device:
  DeviceBuffer<void> tables;             // first tile of each map, the map descriptors, the views' planes
  DeviceBuffer<int> results;             // live [N], reach [V][N], nearest and farthest [V][N] (encoded): zeroed per call
  PinnedBuffer<int> results_host;
};
// The reduction channel of an SDF optimiser (dslam_register_maps, dslam_track_camera_sdf): one row of 33 partial sums per
// workgroup in mapped page-locked memory (kernels: partials.device()), added by the host in index order
struct SumChannel {
  PinnedBuffer<double> partials;         // [rows][33], allocated by the first call
  double last_sums[kRegSums] = {0};      // the totals of the most recent evaluation (dslam_debug_*_sums; test hook)
  bool have_sums = false;
  int ensure(int rows) { return partials ? 0 : partials.alloc((size_t)rows * kRegSums, hipHostMallocMapped); }
  void collect(int rows, Evaluation33 &ev) {
    ev.sum_rows(partials, 0, rows);
    memcpy(last_sums, ev.sums, sizeof last_sums);
    have_sums = true;
  }
};
// The reduction channel of dslam_track_camera_sdf_rgb (track_sdf_rgb.hip): SumChannel's with 35 sums per row
constexpr int kTrackSdfRgbSums = 35;
struct RgbSumChannel {
  PinnedBuffer<double> partials;         // mapped: [rows][35], allocated by the first call
  double last_sums[kTrackSdfRgbSums] = {0};   // the totals of the most recent evaluation (dslam_debug_track_sdf_rgb_sums; test hook)
  bool have_sums = false;
  int ensure(int rows) { return partials ? 0 : partials.alloc((size_t)rows * kTrackSdfRgbSums, hipHostMallocMapped); }
  // rows 0 .. rows of the per-workgroup partials, added in index order
  void collect(int rows) {
    const double *row = partials;
    for (int i = 0; i < kTrackSdfRgbSums; i++) last_sums[i] = 0.0;
    for (int g = 0; g < rows; g++, row += kTrackSdfRgbSums)
      for (int i = 0; i < kTrackSdfRgbSums; i++) last_sums[i] += row[i];
    have_sums = true;
  }
};
// dslam_score_camera_poses / dslam_track_camera_sdf_starts (track_sdf_starts.hip): their own scratch.  The tables exist
// from the first call on; the rows grow on demand (a larger level or more poses in a round) and are never allocated per call.
struct TrackStartsScratch {
  DeviceBuffer<double> rows;             // [poses of a round][workgroups per pose][33], one row per workgroup of k_track_sdf_starts
  size_t rows_capacity = 0;              // ... in doubles
  PinnedBuffer<double> rows_host;        // mapped: the same rows when the host adds them (DSLAM_TRACK_STARTS_ROWS=host, a
  size_t rows_host_capacity = 0;         // measurement's switch); never allocated otherwise
  PinnedBuffer<float> poses_host;        // [DSLAM_MAX_TRACK_STARTS][12]: the P~ of a round on their way to the device
  DeviceBuffer<float> poses;             // ... where the kernel reads them by scalar loads
  PinnedBuffer<double> sums;             // mapped: [DSLAM_MAX_TRACK_STARTS][33], the totals k_track_sdf_row_sum writes
  std::vector<double> last_sums;         // [starts][33]: each start's most recent evaluation in the most recent _starts call
                                         // (dslam_debug_track_sdf_start_sums; test hook)
};
// dslam_query_points / dslam_cast_rays (query.hip): what the host forms stage a chunk of elements through; grown on demand
// (to one chunk of 2^20 elements at the most) and released with the engine
struct QueryScratch {
  DeviceBuffer<void> in, out;            // a chunk's points or rays, and its 48-byte results
  size_t in_bytes = 0, out_bytes = 0;    // their capacities
};
// dslam_mark_occupancy / dslam_distance_transform / dslam_distance_field (distance_field.hip): the packed states of a grid,
// its int32 line distances, what the host forms stage state bytes through, and the call's map table; each grown on demand
// and released with the engine
struct DistanceFieldScratch {
  DeviceBuffer<unsigned> packed;         // [dims2][dims1][ceil(dims0 / 16)]: 2 bits per cell, 16 cells along x per word
  DeviceBuffer<int> lines;               // [cells]: the passes work in place; the host forms' distances leave from here
  DeviceBuffer<unsigned char> bytes;     // [cells]: the host forms' state bytes, in or out
  DeviceBuffer<void> maps;               // [DSLAM_MAX_RENDER_MAPS] map descriptors of a marking call
  size_t packed_words = 0, lines_cells = 0, bytes_cells = 0;   // their capacities
  // dslam_debug_distance_field_phases (bench hook): events recorded at the phase boundaries of a call while `timing` is set
  bool timing = false;
  Event events[5];
  unsigned recorded = 0;                 // bit k: events[k] was recorded by the most recent call
};
// bytes of one map descriptor (MultiMap, multimap_device.h) in dslam_engine::map_table
constexpr size_t kMapDescriptorBytes = 80;
}  // namespace dslam

// (the handles' destructors free memory now: they are not part of the library's exported names)
#define DSLAM_INTERNAL __attribute__((visibility("hidden")))

using dslam::DeviceBuffer, dslam::Event, dslam::PinnedBuffer;

// The engine's compute stream, and with it the permission to run the next allocation pass' k_mark beside what the stream still
// holds.  dslam_get_image grants it once its stamped range pass and everything behind it are enqueued; whoever
// takes the stream to enqueue anything else -- a launch, a copy, a memset, the caller through dslam_engine_stream -- withdraws
// it by the act of taking it, so no launch site has to remember to.  Waits and event records, which touch no buffer, look at
// the stream through peek() and leave the permission alone.
class EngineStream {
 public:
  EngineStream() = default;
  EngineStream(const EngineStream &) = delete;
  EngineStream &operator=(const EngineStream &) = delete;
  operator hipStream_t() const { settle(); stamped_last_ = false; return s_; }
  hipStream_t peek() const { settle(); return s_; }
  hipStream_t *create_into() { return &s_; }
  // Calls whose bodies are still held back (dslam_engine::deferred) come first, whoever asks for the stream and
  // for whatever: the engine arms the hook while it holds any, and the bodies themselves run with it disarmed.
  void arm(void (*run)(void *), void *owner) { run_held_ = run; owner_ = owner; }
  void disarm() { run_held_ = nullptr; }
  void grant() { stamped_last_ = true; }
  bool take() { const bool had = stamped_last_; stamped_last_ = false; return had; }   // (the permission is good for one pass)

 private:
  void settle() const { if (run_held_) run_held_(owner_); }
  hipStream_t s_ = nullptr;
  void (*run_held_)(void *) = nullptr;
  void *owner_ = nullptr;
  mutable bool stamped_last_ = false;   // the last thing enqueued that k_mark could collide with is a stamped GetImage
};

struct DSLAM_INTERNAL dslam_engine : dslam::EngineScratch {
  int device = 0;
  EngineStream stream;
  // k_mark beside the previous GetImage's march; DSLAM_OVERLAP_MARK=0 turns it off
  hipStream_t aux_stream = nullptr;   // holds nothing but that k_mark and, behind it, the pass' deferring sweep (4h) and GetImage's front
                                      // end for the pass' pose (4i); the host waits for it before anything that reads what they wrote is enqueued
  bool overlap_mark = true;
  bool stream_lent = false;           // dslam_engine_stream handed the compute stream out: the caller may order its own work by it
  PinnedBuffer<unsigned> start_stamp; // page-locked, fine-grained: the stamp of the last stamped range pass that has STARTED
  unsigned stamp_seq = 0;             // the stamp given to the last range pass enqueued with one (0: none yet)
  long long mark_overlapped = 0, mark_in_stream = 0;   // allocation passes whose k_mark ran on aux_stream / in the stream (test hook)
  // ... and the pass' sweep behind it on aux_stream, its table writes deferred to k_publish_entries;
  // DSLAM_OVERLAP_SWEEP=0 keeps the sweep in the stream
  bool overlap_sweep = true;
  long long sweep_overlapped = 0, sweep_in_stream = 0;   // (test hook)
  unsigned pend_pass = 0;             // overlapped sweeps so far: which pair of pend_count the next one appends through
  bool publish_due = false;           // aux_stream holds a deferring sweep whose k_publish_entries is not enqueued yet
  // ... and behind the sweep GetImage's front end for the pass' pose -- selection and range pass -- on aux_stream as well,
  // beside the publish kernel and the plain fusion launch; DSLAM_OVERLAP_FRONT=0 keeps it in the fusion launch
  bool overlap_front = true;
  long long front_on_aux = 0, front_in_launch = 0;   // front ends computed on aux_stream / in the fusion launch (test hook)
  bool front_pending = false;         // aux_stream holds such a front end the host has not waited for yet (settle_front)
  // Host order ("Host order"): the front end is launched at ProcessFrame time directly behind the sweep, and the
  // held tail waits for the sweep alone, not for the whole stream, so that the publish kernel and the fusion launch are
  // enqueued as soon as the sweep is complete.  What tells it is the selection's own start: one lane stores the pass' number
  // into start_stamp[1] (a stream runs its launches in order), and the host polls the word as it polls the start stamp.
  // DSLAM_SWEEP_DONE_EVENT=1, a measurement's switch, records an event between the two kernels and waits for that instead.
  // DSLAM_FRONT_BEHIND_TAIL=1, another, launches the front end from the tail, behind the fusion launch (the order that lost).
  bool front_behind_tail = false;
  bool sweep_done_by_event = false;
  Event sweep_done;
  bool sweep_done_recorded = false;   // the sweep in flight has sweep_done behind it (the event, or:)
  unsigned sweep_done_seq = 0;        // ... the value start_stamp[1] takes when the selection behind the sweep has started (0: none)
  unsigned front_seq = 0;             // front ends launched behind a sweep so far
  bool front_at_pass = false;         // the pass in flight launched its front end itself (frame_tail: nothing left to launch)
  bool stamp_due = false;             // GetImage adopted a complete record: its march carries the start stamp (raycast.hip)
  // The pipelined upload enqueues its copy between the held calls: behind a ProcessFrame tail that left a front end on
  // aux_stream, in front of the GetImage that has to sit that stream out (capi.hip upload_view_pipelined).  Called once.
  std::function<void()> after_tail;
  // Calls whose body the caller's thread runs later: the tail of a ProcessFrame whose sweep runs on aux_stream,
  // and a GetImage / fence record behind it.  Run in order by flush_deferred() -- from the pipelined upload while its copy is
  // in flight, and otherwise by whatever touches the engine next (every entry point; EngineStream as the backstop).
  std::vector<std::function<int()>> deferred;
  bool flushing = false;
  int deferred_rc = 0;                // first failure of a deferred body, told once by device_errors()
  std::string deferred_error;
  // What a stamp that has arrived proves about the views: view_reads when the stamped range pass was enqueued (every kernel
  // that read a view and was counted by then is complete), and the newest such figure the host has seen arrive.
  unsigned long long stamp_view_reads = 0, view_reads_done = 0;
  // Handles made from this engine that still exist (scenes, render states, views, frame stores: everything that keeps a
  // pointer to it and reads it in its destroy call).  dslam_engine_destroy with children left only closes the engine:
  // object and streams stay until the last child's destroy call (capi.hip engine_adopt / engine_release).
  int children = 0;
  bool closed = false;
  // A caller's fence recorded behind the last call that read a view is also that view's "consumed" mark: the pipelined
  // upload then records no event of its own (an event record costs the compute stream ~3.5 us per frame, measured).
  unsigned long long view_reads = 0;   // calls that enqueued kernels reading a view's images, so far
  dslam_fence *last_fence = nullptr;   // most recently recorded fence
  std::vector<dslam_fence *> fences;   // every fence of this engine that still exists: live ones, and destroyed ones whose
                                       // event a view still waits on (they go when the last such view lets go)
  hipStream_t copy_stream = nullptr;  // pipelined uploads (async mode, page-locked sources): H2D of frame i + 1 under frame i's kernels
  bool async_mode = false;
  // ProcessFrame computes GetImage's front end for its own pose (FrontEndRecord); DSLAM_SPECULATIVE_FRONT_END=0 turns it off
  bool speculate_front = true;
  dslam_weight_params wp{0, 1, 1.0f};
  unsigned alloc_pass = 0;
  // tickets of the single-pass ordered compactions (dslam_device.h take_ticket): one ever-growing device counter and
  // the value the host knows it has
  DeviceBuffer<unsigned> ticket;         // device [16]: counter k is ticket + k
  unsigned ticket_base = 0;           // counter 0
  unsigned ticket_base2 = 0;          // counter 1 (a second, independent chain inside the same launch)
  unsigned ticket_base3 = 0;          // counter 2: the allocation sweep that runs on aux_stream
  unsigned long long hip_failures_seen = 0;  // ... which is only as good as the launches that were accepted: after any HIP
                                      // failure of the process the bases are read back from the device (tickets_resync)
  // what kernels could not tell anybody (report_error, dslam_device.h): one page-locked word, looked at by every entry
  // point that waits for the stream (sync_check).  Sticky per scene in SceneCounters::error_flags; here: told once.
  PinnedBuffer<int> err_host;
  unsigned epoch = 0;
  int sweep_grid_cap = 0;             // workgroups of the sweep kernels that are certainly co-resident on this device
  // pinned staging
  PinnedBuffer<void> pinned;             // small host mirror for counters / stats
  size_t pinned_bytes = 0;
  DeviceBuffer<char> staging_dev;        // H2D staging for view uploads (rgba + depth)
  size_t staging_bytes = 0;
  PinnedBuffer<char> staging_host;
  // kernel timer (bench roofline): HIP events around the integrate kernel on the engine stream
  bool timer_enabled = false;
  std::vector<Event> ev_pool;
  size_t ev_used = 0;
  double timer_ms = 0;
  long long timer_launches = 0;
  long long timer_blocks = 0;
  DeviceBuffer<int> timer_counts_dev;    // visible-block count of each timed launch (written by the kernel)
  int sm_count = 256;
  // visible blocks from which on a fusion launch counts as larger than the Infinity Cache (65536 x 4 KiB = 256 MiB): trailing
  // push workgroups (integrate.hip kPushJobMin, decided on the device) and streaming cache policy (decided by the host from
  // dslam_render_state::vis_hint).  Lowered only by the parity test of those paths.
  int push_job_min = 65536;
  long long stream_launches = 0;      // fusion / de-integration launches that took the streaming instantiation (test hook)
  long long front_launches = 0;       // fusion launches that computed GetImage's front end (FrontEndRecord; test hook)
  long long front_adoptions = 0;      // GetImage front ends taken from such a record instead of computed (test hook)
  int render_tile_budget = DSLAM_MAX_RENDERING_BLOCKS;  // MAX_RENDERING_BLOCKS; lowered only by the budget test
  PinnedBuffer<double> icp_partials;  // depth tracker: per-workgroup partial sums in mapped page-locked memory (kernels: device())
  double icp_last_sums[29] = {0};     // the totals of the most recent ComputeGandH evaluation (dslam_debug_icp_sums; test hook)
  bool icp_have_sums = false;
  DeviceBuffer<int> misc_counter;        // device: small result counters of one-off kernels (depthPostProcessing)
  // the last mesh dslam_mesh_scene produced (ITMMesh: triangles as 3 x Vector3f, metres)
  DeviceBuffer<float> mesh_positions;    // device [mesh_triangles][3][3]
  DeviceBuffer<float> mesh_colours;      // device [mesh_triangles][3][3], only if asked for
  size_t mesh_bytes = 0;              // capacity of each of the two buffers
  int mesh_triangles = 0;
  bool mesh_has_colour = false;
  bool mesh_table_ready = false;      // the case table sits in this device's constant memory
  bool multimesh_table_ready = false; // dslam_mesh_scene_multi (multimesh.hip): its copy of the case table is in place
  // The map descriptors of one multi-map call (dslam_get_image_multi, dslam_mesh_scene_multi per map pass,
  // dslam_track_camera_sdf): DSLAM_MAX_RENDER_MAPS x MultiMap, device.  One table serves all three: every upload to it
  // and every kernel that reads it is enqueued on this engine's one stream, so a call's kernels have read the table
  // before the next call's upload overwrites it.
  DeviceBuffer<void> map_table;
  dslam::SumChannel reg_sums;         // dslam_register_maps (register.hip)
  dslam::SumChannel track_sdf_sums;   // dslam_track_camera_sdf (track_sdf.hip)
  dslam::RgbSumChannel track_sdf_rgb_sums;   // dslam_track_camera_sdf_rgb (track_sdf_rgb.hip)
  dslam::TrackStartsScratch track_starts;   // dslam_score_camera_poses, dslam_track_camera_sdf_starts (track_sdf_starts.hip)
  dslam::MergeScratch merge;          // dslam_merge_maps (merge.hip)
  dslam::LiveLists live_lists;        // dslam_register_graph, dslam_survey_overlaps
  dslam::RegisterGraphScratch reg_graph;   // dslam_register_graph (register_graph.hip)
  dslam::OverlapScratch overlap;      // dslam_survey_overlaps (overlap.hip)
  dslam::ViewSurveyScratch view_survey;   // dslam_survey_views (view_survey.hip)
  long long view_survey_launches = 0; // kernel launches dslam_survey_views has enqueued (test hook)
  dslam::QueryScratch query;          // dslam_query_points, dslam_cast_rays (query.hip)
  dslam::DistanceFieldScratch distance_field;   // dslam_mark_occupancy, dslam_distance_transform, dslam_distance_field
  std::vector<double> reg_graph_sums; // [pairs][33]: each pair's totals at the most recent joint evaluation it took part
                                      // in (dslam_debug_register_graph_sums; test hook)
  // dslam_debug_merge_phases (bench hook): wall clock of the last merge's phases, each closed by a wait for the stream --
  // [0] the source's live list, [1] mark kernels, [2] ordered selections (ranks, serve, touched list), [3] block kernel,
  // [4] read-backs
  bool merge_phases_on = false;
  double merge_phase_ms[5] = {0, 0, 0, 0, 0};
};

// GetImage's front end for the pose of the last ProcessFrame: FindVisibleBlocks with the projections of its blocks and a reset
// range image, computed by workgroups at the front of that ProcessFrame's fusion launch (they read the table, not the
// voxels) -- or, where the pass' sweep ran on aux_stream, behind that sweep with the range pass as well.
// A GetImage of the same scene version, pose, intrinsics and image size adopts the buffers -- their pointers are exchanged
// with the render state's -- and runs only the range pass and the march, or the march alone (raycast.hip).
struct FrontEndRecord {
  bool valid = false;
  bool range_filled = false;          // computed on aux_stream, range pass included: GetImage runs the march alone
  unsigned long long version = 0;     // the scene's version after the ProcessFrame
  float M[16] = {0}, intr[4] = {0};
  int w = 0, h = 0, n_local = 0, n_entries = 0;   // the sizes of the buffers (= those of the render states they may go to)
  DeviceBuffer<int> visible_ids, proj_req, proj_wg_tiles;
  DeviceBuffer<int4> proj_boxes;
  DeviceBuffer<float2> proj_z, range;
  DeviceBuffer<dslam::RenderCounters> counters;
};

// The lazily allocated groups of a scene: each exists whole or not at all (built aside, move-assigned when complete).
struct SceneDirty {
  // sharded re-integration: per voxel-block slot "a (de-)integration pass visited this block since tracking began"
  DeviceBuffer<unsigned char> dirty;       // device [num_local_blocks], allocated by dslam_scene_track_dirty
  DeviceBuffer<int> dirty_list;            // device [num_local_blocks]: the dirty slots in virtual (shard-major) order
  DeviceBuffer<int> dirty_counts;          // device [128]: per shard its number of dirty slots (+ scratch)
};
struct SceneBatch {
  // block-major re-integration batch (dslam_reintegrate_batch): per voxel-block slot the re-fusion pass of the batch that
  // allocated it (0: it existed before), which operations of the batch touch it, an entry that holds it; the list of
  // touched slots; [0] its length, [1] the work cursor.  alloc_born / alloc_born_stamp: the allocation sweep stamps the
  // blocks it commits while a batch is being planned
  DeviceBuffer<int> batch_born;
  DeviceBuffer<unsigned long long> batch_opmask;
  DeviceBuffer<int> batch_slot_entry, batch_order, batch_counters;   // (batch_order: 8 class lists)
  DeviceBuffer<unsigned char> batch_marks;   // [num_local_blocks][64]: operation k of the batch touches the block (zero between batches)
  DeviceBuffer<dslam::BatchOp> batch_ops_dev;
  DeviceBuffer<dslam::BatchListRef> batch_lists_dev;
  PinnedBuffer<void> batch_staging;          // page-locked: the operations and list references of a batch on their way to the device
  Event batch_staging_ev;                 // ... the copies out of it have been made
};

struct DSLAM_INTERNAL dslam_scene : SceneDirty, SceneBatch {
  dslam_engine *engine = nullptr;
  dslam_scene_params p{};
  int n_entries = 0;
  DeviceBuffer<dslam::HashEntry> hash;
  uint2 *voxels = nullptr;            // what the kernels use: voxels_own, or the caller's buffer (borrowed, never freed here)
  DeviceBuffer<uint2> voxels_own;     // empty when the voxels are the caller's
  DeviceBuffer<int> alloc_list;
  DeviceBuffer<int> excess_list;
  DeviceBuffer<int> last_seen;           // per voxel-block slot
  DeviceBuffer<dslam::SceneCounters> counters;  // device
  // visible-list history: per voxel-block slot two bit rings (0 fusion, 1 defusion); list k of ring q
  // owns bit k % (64*history_words) of masks[(slot*2+q)*history_words ...]
  int history_words = 4;
  DeviceBuffer<unsigned long long> masks;  // device
  int ring_head[2] = {0, 0}, ring_next[2] = {0, 0}, decay_cursor[2] = {0, 0};
  int frame_counter = 0;
  // ITMGlobalCache
  DeviceBuffer<unsigned char> swap_state;  // device [entries]
  DeviceBuffer<unsigned> alloc_bits;       // device [bit tiles]: bit t = entry t holds a resident block (ptr >= 0)
  DeviceBuffer<unsigned> swap1_bits;       // device [bit tiles], swapping only: bit t = swap_state[t] == 1 (host copy to be merged)
  // host store of swapped-out blocks: page-locked slabs the kernels read and write directly over PCIe (no staging
  // copy, no host memcpy); an entry's block lives in slot slot_dev[entry]; slots are handed out by an atomic counter
  std::vector<PinnedBuffer<uint4>> slabs;          // pinned, kSlabBlocks blocks each, allocated as the store grows
  DeviceBuffer<uint4 *> slab_ptrs_dev;     // device [kMaxSlabs]: the same pointers for the kernels
  DeviceBuffer<int> slot_dev;              // device [entries]: slot of the entry's stored block, -1 = none.  The table and
                                        // the slot counter (SceneCounters::next_slot) live on the device: a swap batch
                                        // needs no host round trip (round 1: two per ProcessFrame)
  PinnedBuffer<int> next_slot_host;        // pinned: copy of next_slot queued behind every batch that may hand out slots
  long long slot_bound = 0;             // upper bound of next_slot the host can prove (slabs exist for all of it)
  int shard = 0, num_shards = 1, chunk_blocks = 256;
  unsigned long long version = 0;       // bumped by every call that can change the map (GetImage memo key)
  int shard_first = 0, shard_count = -1;  // contiguous slot range (count < 0: off)
  DeviceBuffer<float> batch_depth;           // one float depth image per keyframe of a batch (written by its allocation pass, read by
  size_t batch_depth_pixels = 0;          // both of its operations in the block launch); pixels per image it was sized for
  bool dirty_tracking = false;
  int *alloc_born = nullptr;               // = batch_born while a batch is being planned
  int alloc_born_stamp = 0;
  int dirty_shards = 0, dirty_chunk = 0;  // the layout of the last dslam_shard_dirty_plan
  std::unique_ptr<FrontEndRecord> front;  // allocated by the first ProcessFrame that computes it
};

// The lazily allocated groups of a render state (whole or not at all, as a scene's).  CreateICPMaps:
struct RenderIcpMaps {
  DeviceBuffer<float4> icp_points, icp_normals;
  DeviceBuffer<uchar4> raycast_image;  // ITMRenderState::raycastImage: the grey tracking raycast CreateICPMaps draws (with the maps)
};
struct RenderMulti {
  // dslam_get_image_multi (multimap.hip), allocated by its first call: per range cell the maps whose blocks project into
  // it (bit i = map i), per map its visible-block count (the descriptors go to dslam_engine::map_table)
  DeviceBuffer<unsigned long long> multi_mask;
  DeviceBuffer<int> multi_counts;
};

struct DSLAM_INTERNAL dslam_render_state : RenderIcpMaps, RenderMulti {
  dslam_engine *engine = nullptr;
  int w = 0, h = 0, n_entries = 0, n_local = 0;
  DeviceBuffer<int> visible_ids;
  DeviceBuffer<unsigned char> visible_type;
  DeviceBuffer<unsigned> vis_bits;   // bit t = visible_type[t] != 0 (kept by every kernel that writes a type)
  DeviceBuffer<float2> range;      // renderingRangeImage (full image stride)
  DeviceBuffer<float4> raycast;    // raycastResult
  DeviceBuffer<uchar4> image_rgba; // RenderImage's outputImage (rgba types)
  DeviceBuffer<float> image_float;
  DeviceBuffer<int4> proj_boxes;   // per visible block: render bbox (ul.x, ul.y, lr.x, lr.y)
  DeviceBuffer<float2> proj_z;     // per visible block: z range
  DeviceBuffer<int> proj_req;      // per visible block: render tiles required (0 = invalid projection)
  DeviceBuffer<int> proj_wg_tiles; // render tiles requested per workgroup of the projection pass (summed by the next kernel)
  DeviceBuffer<dslam::RenderCounters> counters;  // device
  // One page-locked word: the length of the visible list as an allocation pass that RAN left it -- k_alloc_sweep rewrites it
  // whenever the answer to "at least push_job_min blocks?" would change, an uploaded list sets it.  The
  // host looks at it -- without waiting for anything, so on an asynchronous engine it is a frame or two late -- to choose the
  // fusion kernel's cache policy (launch_integrate): a hint, both policies compute the same bytes.
  PinnedBuffer<int> vis_hint;
  // entriesVisibleType carries a generation bit (0x80): an allocation pass writes its marks with the pass' bit, so a
  // non-zero byte with the OTHER bit is "visible in the previous pass" (upstream's re-arming of the previous visible
  // list as type 3) without a pass over that list.  The C ABI hands out the plain types (bit masked off).
  unsigned char gen = 0;
  // the visible list was replaced behind the types' back (FindVisibleBlocks on this render state, an uploaded list):
  // the next allocation pass re-derives the "previously visible" marks from the list first
  bool types_follow_list = true;
  // GetImage memo: raycastResult (and the visible list / range image behind it) is still that of this scene version,
  // pose and intrinsics, so another image type of the same view only has to be shaded (the reference's GUI asks for
  // a depth and a colour image of the same free pose every tick, DenseSlam.h:146-164)
  bool memo_valid = false;
  const dslam_scene *memo_scene = nullptr;
  unsigned long long memo_version = 0;
  int memo_budget = 0;
  float memo_M[16] = {0}, memo_intr[4] = {0};
};

struct ViewLanding {
  // pipelined uploads (async engine + page-locked caller images): two landing buffers, filled on the engine's copy
  // stream while the compute stream still reads the other one
  DeviceBuffer<uchar4> up_rgba[2];
  Event up_done[2];      // copy stream: buffer b has landed
  Event up_consumed[2];  // compute stream: every kernel that reads buffer b has been passed
};

struct DSLAM_INTERNAL dslam_view : ViewLanding {
  dslam_engine *engine = nullptr;
  int w_rgb = 0, h_rgb = 0, w_d = 0, h_d = 0;
  DeviceBuffer<uchar4> rgba;       // own buffers (host uploads land here)
  float *depth = nullptr;       // what the kernels use: depth_own, or (inside a re-integration batch) one of the batch's images
  DeviceBuffer<float> depth_own;
  short *raw_depth = nullptr;   // (inside rgba's allocation, behind the RGBA image)
  mutable DeviceBuffer<float> pyramid;  // depth tracker: levels 1.. of the depth pyramid (scratch, allocated on first use)
  mutable DeviceBuffer<float> grey;     // photometric tracker: the grey pyramid of rgba_src (scratch, allocated on first use)
  mutable int grey_levels = 0;          // ... the levels the most recent dslam_track_camera_sdf_rgb built
  // what the kernels read: own buffers, or the caller's resident frame (dslam_view_update_device: no copy)
  const uchar4 *rgba_src = nullptr;
  const short *raw_src = nullptr;
  short *up_raw[2] = {nullptr, nullptr};  // (inside up_rgba[b]'s allocation, behind the RGBA image)
  hipEvent_t up_consumed_by[2] = {nullptr, nullptr};  // the event that says so for the current contents: up_consumed[b] or a caller's fence
  dslam_fence *up_lender[2] = {nullptr, nullptr};     // ... the fence that event belongs to, if it is a caller's
  bool up_used[2] = {false, false};
  unsigned long long up_reads[2] = {0, 0};   // engine->view_reads when buffer b's last reader had been called (see dslam_engine::view_reads_done)
  int up_next = 0;
  float affine_a = 0.001f, affine_b = 0.0f;
  mutable bool depth_dirty = false;  // float depth not yet derived from raw_src (done by the next consumer)
  double timestamp = 0;
  bool updated = false;         // an UpdateView has given the view a frame (dslam_track_camera_sdf refuses a view without one)
};

// a marker in the engine's stream (dslam_fence_*): lets a pipelining caller learn when a frame's results have landed
struct DSLAM_INTERNAL dslam_fence {
  dslam_engine *engine = nullptr;
  Event ev;
  bool recorded = false;
  unsigned long long view_reads_at_record = 0;  // engine->view_reads when it was recorded
  int lent_count = 0;   // views that wait on `ev` as their "landing buffer consumed" mark at the moment
  bool record_held = false;   // dslam_fence_record was called, the record itself waits in dslam_engine::deferred
  bool zombie = false;  // destroyed by the caller while lent: the object and its event live until the last view lets go
};

// mfusionFrameDataBase's image payload (fusionFrameInfo::rgbinfo / depthinfo, DenseSlam.h:431-433) kept in HBM:
// `capacity` slots of one RGBA image + one int16 depth image each, in two contiguous arrays
struct DSLAM_INTERNAL dslam_frame_store {
  dslam_engine *engine = nullptr;
  int w_rgb = 0, h_rgb = 0, w_d = 0, h_d = 0, capacity = 0;
  size_t rgba_bytes = 0, depth_bytes = 0;  // per slot
  DeviceBuffer<unsigned char> rgba;
  DeviceBuffer<unsigned char> depth;
  // optional: per slot the visible list of the keyframe's fusion (dslam_frame_store_enable_lists):
  // [RenderCounters-sized header: count][int ids[list_cap]][short4 pos[list_cap]]
  DeviceBuffer<unsigned char> lists;
  int list_cap = 0;
  int list_entries = 0;   // hash-table size (entries) of the scene the lists were enabled for: their ids index that table
  size_t list_bytes = 0;  // per slot
  std::vector<unsigned char> has_list;
  // where each slot's list lives: a buffer of `lists`, or -- after a re-integration batch, which writes the lists of its
  // re-fusions to scratch buffers and then trades buffers instead of copying -- one of `batch_lists`
  std::vector<unsigned char *> list_ptr;
  DeviceBuffer<unsigned char> batch_lists;          // 32 more list buffers (allocated by the first batch)
  std::vector<unsigned char *> batch_list_ptr;
};

// The fern keyframe index (fern.hip): the codes of all keyframes, the fern table and the index's own
// scratch.  The scratch groups exist whole or not at all (built aside, move-assigned).
struct FernThumbs {
  DeviceBuffer<unsigned short> thumbs;   // [thumb_slots][2][TW TH]: D and G of the images being encoded
  int thumb_slots = 0;
};
struct FernRows {
  DeviceBuffer<unsigned short> dist;     // [rows][dist_stride]: the dissimilarity of query q to stored id i at [q][i]
  DeviceBuffer<unsigned> partial;        // [rows][kFernMaxSlices][64]: the best keys of each slice of the window
  int rows = 0;                          // 1, or DSLAM_FERN_MAX_QUERIES from the first dslam_fern_query_stored with more than one
};
struct DSLAM_INTERNAL dslam_fern_index : FernThumbs, FernRows {
  dslam_engine *engine = nullptr;
  int w = 0, h = 0, tw = 0, th = 0, capacity = 0, count = 0;
  dslam_fern_params p{};                 // defaults filled in
  std::vector<int32_t> table;            // [F][4][3] as dslam_fern_index_table gives it
  DeviceBuffer<int2> table_dev;          // [F][4] {2 cell + channel, threshold}
  DeviceBuffer<unsigned> codes;          // [capacity][64]
  DeviceBuffer<unsigned> qcode;          // [64]: the code of the view a call encodes
  size_t dist_stride = 0;                // capacity rounded up to 64
  DeviceBuffer<unsigned> result;         // what a call reads back (fern.hip FernResult) ...
  PinnedBuffer<unsigned> result_host;    // ... and where
  PinnedBuffer<int> query_ids;           // mapped: [DSLAM_FERN_MAX_QUERIES] the stored codes a scan compares against
};

// The semi-global stereo matcher (stereo.hip): everything a match of one image size needs.  The
// buffers exist whole or not at all (built aside, move-assigned).
struct StereoBuffers {
  DeviceBuffer<unsigned long long> census;   // [2][H W]: left, right
  DeviceBuffer<unsigned short> S;            // [H][W][D]: the sum of the eight path costs (D innermost)
  DeviceBuffer<unsigned> rkey;               // [H W]: min over d of S(y, xr + d, d) << 8 | d
  DeviceBuffer<unsigned> cand;               // [H W]: d* << 16 | d16 of the left selection, ~0 where rejected
  DeviceBuffer<unsigned char> images;        // [2][H W channels]: where the host forms' images land
  DeviceBuffer<unsigned short> disp;         // [H W]: the disparity of the host forms and of a depth call without disp_out
  DeviceBuffer<short> depth;                 // [H W]: the host forms' depth
};
struct DSLAM_INTERNAL dslam_stereo : StereoBuffers {
  dslam_engine *engine = nullptr;
  int w = 0, h = 0;
  dslam_stereo_params p{};                   // as dslam_stereo_get_params gives it
  int D = 0, p1 = 0, p2 = 0, uniq = 0, lr_max = 0, channels = 0;   // what the kernels take (lr_max < 0: check off)
  bool matched = false;                      // census and S hold a match (dslam_debug_stereo_download)
  // dslam_debug_stereo_phases (bench hook): events recorded at the phase boundaries of a call while `timing` is set
  bool timing = false;
  Event events[6];
  int recorded = 0;
};
// one call of the dslam_stereo_* family, already checked by its entry point (capi.hip)
struct StereoCall {
  const void *left, *right;                  // NULL: no match (conversion alone, or selection on S_host)
  const unsigned short *S_host;              // dslam_debug_stereo_select
  const void *disp_in;                       // dslam_disparity_to_depth*
  const dslam_stereo_calib *calib;           // NULL: no conversion
  void *disp_out, *depth_out;
  bool host;
};

// The sparse scene-flow matcher (sflow.hip).  A "list" is one feature set: l = (slot * 2 + side) * 2 +
// set, slot one of the two frames of the ring, side 0 left / 1 right, set 0 sparse / 1 dense.  Every list has its worst-case
// capacity (4 features per cell) from creation, so nothing can overflow.  The buffers exist whole or not at all.
struct SflowBuffers {
  DeviceBuffer<unsigned char> images;        // [2][H W channels]: where the host form's images land
  DeviceBuffer<unsigned char> sobel;         // [2 sides][du, dv][h w] of the current frame
  DeviceBuffer<short> corner;                // [2 sides][f1, f2][h w]
  DeviceBuffer<int4> cell_feat;              // [2 sides][2 sets][cells of the dense set]: u | v << 16 per class, -1 = none
  DeviceBuffer<int> cell_count, cell_offset; // the same shape: accepted extrema per cell and their exclusive scan
  DeviceBuffer<int4> feats;                  // [8 lists][capacity of the set][3]: the 48-byte records
  DeviceBuffer<int> counts;                  // [8 lists] (+ pad): features per list
  DeviceBuffer<int> bin_fill, bin_start;     // [8 lists][bins], [8 lists][bins + 1]
  DeviceBuffer<unsigned long long> bin_list; // [8 lists][capacity]: (u_bin VB + v_bin) << 32 | index, grouped by bin
  DeviceBuffer<int4> stage, packed;          // [dense capacity][3]: a match per driving feature; the matches compacted
  DeviceBuffer<int> flags, keep, match_offset;   // [dense capacity]
  DeviceBuffer<int> match_count;             // [4]: the count of the most recent match (16-byte aligned)
};
struct DSLAM_INTERNAL dslam_sflow : SflowBuffers {
  dslam_engine *engine = nullptr;
  int w = 0, h = 0;                          // the caller's image size
  dslam_sflow_params p{};                    // as dslam_sflow_get_params gives it
  int s = 1, mw = 0, mh = 0;                 // scale, matching image size
  int n[2] = {0, 0}, cx[2] = {0, 0}, cy[2] = {0, 0}, cap[2] = {0, 0};   // per set: nms distance, cells along x / y, capacity
  int tau = 0, binsize = 0, radius = 0, vtol = 0, channels = 0, ub = 0, vb = 0;
  int cur = 0, pushes = 0;                   // the ring: slot of the current frame; pushes so far
  bool timing = false;
  Event events[8];                           // push: 0 .. 4, match: 5 .. 7
  int recorded = 0;
};
struct SflowPush { const void *left, *right; bool replace, host; };
struct SflowMatch { int method, set; void *out, *count; int capacity; bool host; };

namespace dslam {
// dslam_sflow_* (sflow.hip); everything already checked by the entry points (capi.hip).  The launches enqueue only; the host
// forms of match / features wait for the stream themselves because the number of records to copy is a device result.
int sflow_resolve_params(const dslam_sflow_params *params, int width, int height, dslam_sflow *sf);
int sflow_allocate(dslam_engine *e, dslam_sflow *sf);
int launch_sflow_push(dslam_engine *e, dslam_sflow *sf, const SflowPush &c);
int launch_sflow_match(dslam_engine *e, dslam_sflow *sf, const SflowMatch &c);
int sflow_features(dslam_engine *e, dslam_sflow *sf, int image, int set, void *out_host, int capacity, int32_t *count_out);
int sflow_download(dslam_engine *e, dslam_sflow *sf, int side, int filter, void *out_host);
int sflow_phases(dslam_engine *e, dslam_sflow *sf, int enable, float *ms_out);

// dslam_stereo_* (stereo.hip); stereo_resolve_params fills st->p and the kernels' values from a caller's block (or NULL).
// launch_stereo enqueues only (the host forms' copies included).
int stereo_resolve_params(const dslam_stereo_params *params, dslam_stereo *st);
int stereo_allocate(dslam_engine *e, dslam_stereo *st);
int launch_stereo(dslam_engine *e, dslam_stereo *st, const StereoCall &c);
int stereo_download(dslam_engine *e, dslam_stereo *st, int what, void *out_host);
int stereo_phases(dslam_engine *e, dslam_stereo *st, int enable, float *ms_out);

// dslam_fern_* (fern.hip); everything already checked by the entry points (capi.hip).  All wait for the stream; the
// outputs are written only when everything has succeeded.
void fern_build_table(const dslam_fern_params &p, int tw, int th, std::vector<int32_t> &table);
int fern_index_allocate(dslam_engine *e, dslam_fern_index *idx);
int fern_encode_view(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, uint32_t *code_out);
// harvest < 0: the query alone; otherwise dslam_fern_process (*added_out: the new id or -1; DSLAM_ERR_UNSUPPORTED: full)
int fern_query_view(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int harvest, int first_id, int last_id, int k,
                    dslam_fern_match *matches_out, int32_t *num_out, int32_t *added_out);
int fern_add_from_store(dslam_engine *e, dslam_fern_index *idx, const dslam_frame_store *fs, int first_slot, int num_slots);
int fern_query_stored(dslam_engine *e, dslam_fern_index *idx, const int32_t *query_ids, int num_queries, int first_id, int last_id,
                      int k, dslam_fern_match *matches_out, int32_t *num_out);

// diagnostics (DSLAM_DEBUG_SYNC=1): wait for the stream after a launch and say which one it was -- finds the kernel that
// hangs or faults without a profiler
inline bool dbg_sync_on() {
  static const bool on = getenv("DSLAM_DEBUG_SYNC") != nullptr;
  return on;
}
inline void dbg_sync(dslam_engine *e, const char *what) {
  if (!dbg_sync_on()) return;
  fprintf(stderr, "[dslam] %s ...", what);
  fflush(stderr);
  const hipError_t err = hipStreamSynchronize(e->stream.peek());
  fprintf(stderr, " %s\n", err == hipSuccess ? "ok" : hipGetErrorString(err));
  fflush(stderr);
}
// diagnostics (<env>=<file>): the per-wave / per-tile records ONE launch of a site leaves -- its `ordinal`-th, well into the
// run -- in a zeroed page-locked buffer, written to the file as they are.  One static object per site:
//   static DiagDump dump("DSLAM_DBG_X", 60);
//   params.dbg = dump.arm(records, bytes_per_record);   // null on every launch but that one
//   <launch>
//   DSLAM_TRY(dump.write(e));                           // nothing unless armed
class DiagDump {
 public:
  DiagDump(const char *env, int ordinal) : file_(getenv(env)), ordinal_(ordinal) {}
  bool enabled() const { return file_ != nullptr; }
  // the pointer the kernel stores its records through, or null: not this launch (or the allocation failed: write says so)
  unsigned long long *arm(size_t records, size_t bytes_per_record) {
    if (!file_ || ++calls_ != ordinal_) return nullptr;
    bytes_ = records * bytes_per_record;
    if ((rc_ = buf_.alloc(bytes_)) != DSLAM_OK) return nullptr;
    memset(buf_, 0, bytes_);
    return static_cast<unsigned long long *>(buf_.get());
  }
  // after the launch: wait for it and write the file; the code of a failed arm or of the wait otherwise
  int write(dslam_engine *e) {
    if (const int rc = rc_) { rc_ = DSLAM_OK; return rc; }
    if (!buf_) return DSLAM_OK;
    PinnedBuffer<void> buf = std::move(buf_);   // (armed once: the buffer goes with this call)
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    if (FILE *f = fopen(file_, "wb")) { fwrite(buf, 1, bytes_, f); fclose(f); }
    return DSLAM_OK;
  }

 private:
  const char *file_;
  int ordinal_, calls_ = 0, rc_ = DSLAM_OK;
  size_t bytes_ = 0;
  PinnedBuffer<void> buf_;
};
// kernels' host launchers (one translation unit per subsystem)
int launch_scene_reset(dslam_engine *e, dslam_scene *s);
int launch_scene_reset_tables(dslam_engine *e, dslam_scene *s);   // ... without the voxel pool
// packed maps (pack.hip); the scene already checked by the entry point.  buf: the caller's pointer (pack: null = size query)
int pack_buffer_address(dslam_engine *e, const void *p, int64_t bytes, void **dev_out);
int launch_pack_scene(dslam_engine *e, const dslam_scene *s, void *buf, int64_t capacity, dslam_pack_info *info);
int launch_unpack_validate(dslam_engine *e, const dslam_scene *s, const void *buf_dev, const dslam_pack_info *h);
int launch_unpack_write(dslam_engine *e, dslam_scene *s, const void *buf_dev, const dslam_pack_info *h);   // enqueues only
int launch_inject_error(dslam_engine *e, dslam_scene *s, int bits);
int launch_build_alloc_bits(dslam_engine *e, dslam_scene *s);  // alloc_bits from an uploaded table
int launch_view_convert(dslam_engine *e, dslam_view *v, const void *rgba_dev, const void *depth_dev, float a, float b);
int launch_bgr_to_rgba(dslam_engine *e, const void *bgr_dev, uchar4 *rgba_dev, int npix);
int launch_bilateral(dslam_engine *e, dslam_view *v);
int launch_dataset_depth(dslam_engine *e, short *depth_dev, int n, int format, float max_depth_m);
int launch_depth_to_int16(dslam_engine *e, const float *depth_dev, short *out_dev, int n, int scale);
int launch_depth_post(dslam_engine *e, short *curr_dev, const unsigned short *prev_dev, int cols, int rows,
                      const float *Tpc, const float *intr, float threshold, float area, int *count_dev);
// list_out / count_out: write the pass' visible list there instead of into the render state's own list (whose bitmap and
// types follow the pass either way; the re-integration batch keeps the lists of all its passes)
int launch_allocate(dslam_engine *e, dslam_scene *s, const dslam_view *v, dslam_render_state *r, const float *M_d,
                    const float *intr, int only_update_visible_list, int *list_out = nullptr, void *count_out = nullptr,
                    bool *publish_left = nullptr, FrontEndRecord *front_aux = nullptr);
// (front_aux: where the sweep goes to aux_stream and the caller finishes the pass later, GetImage's front end for this pose
// follows the sweep there, into this record -- DESIGN.md 4i; dslam_engine::front_at_pass says whether it did)
// (publish_left: the caller finishes an overlapped pass itself, later -- finish_overlapped_allocate -- and learns here
// whether there is one to finish; null: launch_allocate does before it returns)
// push_ring >= 0: also queue the frame's visible list on that ring (fused into the integrate kernel)
// front: also compute GetImage's front end for (M_d, intr_d, r's image size) into it, in the same launch, if the fusion
// runs the plain one-camera kernel (front->valid says whether it did; its buffers are sized for r beforehand)
int launch_integrate(dslam_engine *e, dslam_scene *s, const dslam_view *v, const dslam_render_state *r,
                     const float *M_d, const float *intr_d, const float *M_rgb, const float *intr_rgb,
                     bool deintegrate, int push_ring = -1, FrontEndRecord *front = nullptr, int front_on_aux = 0);
// (front_on_aux, DESIGN.md 4i: the front end belongs on aux_stream behind the pass' deferring sweep and the fusion launch
// stays the plain one -- 1: launch it there now, behind this launch (launch_front_end_aux); 2: the pass has launched it)
// the same kernel over a stored list (count header, ids, expected block positions) instead of a render state's
int launch_integrate_list(dslam_engine *e, dslam_scene *s, const dslam_view *v, const void *count_header, const int *ids,
                          const short4 *expect_pos, const float *M_d, const float *intr_d, const float *M_rgb,
                          const float *intr_rgb, bool deintegrate);
int launch_store_visible_list(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, void *header, int *ids,
                              short4 *pos, int capacity);
int launch_store_list_positions(dslam_engine *e, const dslam_scene *s, const BatchListRef *jobs_dev, int n_jobs);
int launch_batch_ops(dslam_engine *e, const BatchListRef *lists_dev, int n_ops, const dslam_scene *s, const int *born, unsigned char *marks,
                     unsigned long long *opmask, int *slot_entry, int *cls_list, int *cls_count);
int launch_reintegrate_blocks(dslam_engine *e, dslam_scene *s, int w_d, int h_d, int w_rgb, int h_rgb, const float *intr,
                              const BatchOp *ops_dev, const unsigned long long *opmask, const int *slot_entry,
                              const int *cls_list, const int *cls_count, int push_ring, int n_ops);
int alloc_step_cap(const dslam_scene *s, int W, int H, int *cap_out);
int ensure_view_depth(dslam_engine *e, const dslam_view *v);
int launch_selftest_division(dslam_engine *e, long long samples, unsigned long long *mismatches_dev);
int prepare_push_visible_list(dslam_engine *e, dslam_scene *s, int q, int *bit_out, int *frame_out);
int launch_find_visible(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                        const float *intr);
int launch_count_visible(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, int min_id, int max_id,
                         int *out);
int launch_expected_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                           const float *intr);
int launch_find_visible_and_depths(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M,
                                   const float *intr);
int launch_track_camera(dslam_engine *e, const dslam_view *v, dslam_render_state *r, const float *scenePose, float *pose_M,
                        const float *intr, const dslam_tracker_params *tp, dslam_tracker_result *res);
// the depth pyramid of a view whose float depth is current: level pointers and sizes for `levels` levels (track.hip)
int build_depth_pyramid(dslam_engine *e, const dslam_view *v, int levels, const float **ldepth, int *lw, int *lh);
// everything already checked (and params defaulted) by dslam_track_camera_sdf; pose_M: in the start, out the estimate
int launch_track_camera_sdf(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                            int num_maps, float *pose_M, const float *intr, const dslam_track_sdf_params *params,
                            dslam_track_sdf_result *result);
// everything already checked (and params defaulted) by dslam_track_camera_sdf_rgb (track_sdf_rgb.hip)
int launch_track_camera_sdf_rgb(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                                int num_maps, float *pose_M, const float *intr, const dslam_track_sdf_rgb_params *params,
                                dslam_track_sdf_rgb_result *result);
// level `level` of the grey pyramid the most recent dslam_track_camera_sdf_rgb built on this view, to host memory
int download_track_sdf_rgb_grey(dslam_engine *e, const dslam_view *v, int level, float *out_host);
// arguments already checked by dslam_select_start_poses / dslam_camera_pose_lattice (host only)
void select_start_poses(const dslam_pose_score *scores, int num, int min_valid, int max_keep, int32_t *kept_out, int32_t *num_kept_out);
void camera_pose_lattice(const float pose_M[16], const dslam_pose_lattice &l, float *poses_out);
bool track_sdf_pixels_in_tiles();   // which pixel takes which lane in the tracker's kernels (track_sdf.hip)
// everything already checked (and params defaulted) by dslam_score_camera_poses / dslam_track_camera_sdf_starts; outputs are
// written only by a call that succeeds
int launch_score_camera_poses(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes, const float *T_map_from_world,
                              int num_maps, const float *poses_M, int num_poses, const float *intr, int level, float residual_gate,
                              dslam_pose_score *scores_out);
int launch_track_camera_sdf_starts(dslam_engine *e, const dslam_view *v, const dslam_scene *const *scenes,
                                   const float *T_map_from_world, int num_maps, float *poses_M, int num_starts, const float *intr,
                                   const dslam_track_sdf_params *params, dslam_track_sdf_result *results);
int launch_render(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M, const float *intr,
                  int type, bool reuse_raycast = false, void *image_out_override = nullptr);
// scenes / T (N x 16, world -> map) already checked by dslam_get_image_multi
int launch_render_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int n, dslam_render_state *r,
                        const float *M, const float *intr, int type, void *image_out_override = nullptr);
int launch_icp_maps(dslam_engine *e, const dslam_scene *s, dslam_render_state *r, const float *M, const float *intr);
int launch_mesh_scene(dslam_engine *e, const dslam_scene *s, int max_triangles, int with_colour, int *out_num);
// scenes / T (N x 16, world -> map) already checked by dslam_mesh_scene_multi; out_map: [n] triangles per map, or null
int launch_mesh_scene_multi(dslam_engine *e, const dslam_scene *const *scenes, const float *T, int n, int max_triangles,
                            int with_colour, int *out_num, int32_t *out_map);
// src / dst / X / params already checked (and defaulted) by dslam_register_maps; X: in the start, out the estimate
int launch_register_maps(dslam_engine *e, const dslam_scene *src, const dslam_scene *dst, float *X,
                         const dslam_register_params *params, dslam_register_result *result);
// everything already checked (and params defaulted) by dslam_register_graph; T: in the starts, out the estimates
int launch_register_graph(dslam_engine *e, const dslam_scene *const *scenes, float *T_map_from_world, int num_maps,
                          const int32_t *pairs, int num_pairs, int anchor, const dslam_register_params *params,
                          dslam_register_graph_result *result, dslam_register_pair_result *pair_results);
// scenes / T already checked by dslam_survey_overlaps; the outputs are written only when everything has succeeded
int launch_survey_overlaps(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                           int32_t *live_blocks_out, int32_t *shared_blocks_out, int32_t *shared_octants_out);
// arguments already checked (and params defaulted) by dslam_select_register_pairs: the selection law of DESIGN.md section 16
void select_register_pairs(const int32_t *live_blocks, const int32_t *shared_octants, int num_maps,
                           const dslam_pair_select_params &params, int32_t *pairs_out, int32_t *component_out,
                           dslam_pair_select_result *result);
// the law of dslam_view_frustum_planes; the view already checked
void view_frustum_planes(const dslam_survey_view &view, float voxel_size, float out[28]);
// everything already checked by dslam_survey_views (planes: [num_views][28], rho: the loosened radius); the outputs are
// written only when everything has succeeded
int launch_survey_views(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps,
                        const float *planes, int num_views, float rho, int32_t *live_blocks_out, int32_t *reach_blocks_out,
                        int32_t *nearest_out, int32_t *farthest_out);
// query.hip: dslam_query_points (rays false) / dslam_cast_rays over n elements, everything already checked (max_range
// defaulted); host: in / out are host arrays staged in chunks, else device arrays.  Enqueues only
int launch_query(dslam_engine *e, const dslam_scene *const *scenes, const float *T_map_from_world, int num_maps, bool rays,
                 const void *in, int n, float max_range, int what, void *out, bool host);
// distance_field.hip.  grid_ok: a dslam_grid within the limits of include/dslam_fusion.h (host only).  launch_distance_field:
// everything already checked; scenes NULL: no marking, the states come from states_in (bytes); dist_out / states_out NULL: not
// wanted; host: the arrays are host arrays, staged through dslam_engine::distance_field, else device arrays.  Enqueues only
// (the marking waits once for the live counts)
bool grid_ok(const dslam_grid &g);
struct DistanceFieldCall {
  const dslam_scene *const *scenes;   // NULL: transform only
  const float *T;
  int num_maps;
  dslam_grid grid;
  int min_weight;                     // already defaulted: 1 .. 255
  int thr;                            // occupied: (int16)sdf <= thr
  const void *states_in;              // transform only
  bool transform;
  int seeds, max_cells, format;
  float voxel_size;
  void *states_out, *dist_out;
  bool host;
};
int launch_distance_field(dslam_engine *e, const DistanceFieldCall &c);
int distance_field_phases(dslam_engine *e, int enable, float *ms_out);   // dslam_debug_distance_field_phases
// arguments already checked (and params defaulted) by dslam_select_view_maps: the selection law of DESIGN.md section 20
void select_view_maps(const int32_t *reach_blocks, const int32_t *nearest, int num_views, int num_maps,
                      const dslam_view_select_params &params, int32_t *maps_out, dslam_view_select_result *result);
// live_list.hip: a bitmap of the hash table as an ordered list (one launch of k_bits_select each; enqueue only).
// list_out[0 .. *count_out) = the entries of s with ptr >= 0, ascending; capacity s->n_entries, errors to s->counters
int launch_live_list(dslam_engine *e, const dslam_scene *s, int *list_out, int *count_out);
// list_out[0 .. *count_out) = the set bits of `bits`, ascending; capacity n_entries
int launch_bits_list(dslam_engine *e, const unsigned *bits, int n_entries, int *list_out, int *count_out, SceneCounters *err_cnt);
// The live lists of several maps of one call, in dslam_engine::live_lists: for every map of `wanted`, in that order, one
// launch_live_list into a range of its own.  list_offset[i]: where map i's range begins (-1: not wanted); live[i]: how
// many entries it holds -- read back behind a wait for the stream and clamped to [0, n_entries].
int fill_live_lists(dslam_engine *e, const dslam_scene *const *scenes, int n, const std::vector<int> &wanted,
                    std::vector<int> &list_offset, std::vector<int> &live);
// src / dst / X / params already checked (and defaulted) by dslam_merge_maps
int launch_merge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float *X,
                      const dslam_merge_params *params, dslam_merge_result *result, bool reuse_live = false);
int ensure_merge_scratch(dslam_engine *e, int src_entries, int dst_entries);
// dslam_unmerge_maps / dslam_remerge_maps (unmerge.hip), arguments already checked.  defer: enqueue only -- the caller
// collects the result (collect_unmerge_result) after a later wait for the stream
int launch_unmerge_maps(dslam_engine *e, const dslam_scene *src, dslam_scene *dst, const float *X, int with_colour,
                        dslam_unmerge_result *result, bool defer);
void collect_unmerge_result(dslam_engine *e, dslam_unmerge_result *result);
int launch_decay(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int max_weight, int min_age, int force_all,
                 int which);
int launch_slide_pop(dslam_engine *e, dslam_scene *s, dslam_render_state *r, int which);
int launch_swap_in(dslam_engine *e, dslam_scene *s, dslam_render_state *r);
int launch_swap_out(dslam_engine *e, dslam_scene *s, dslam_render_state *r, bool ignore_visibility);
int launch_save_to_global(dslam_engine *e, dslam_scene *s);
int launch_dirty_plan(dslam_engine *e, dslam_scene *s, int num_shards, int chunk_blocks, int *counts_host);
int launch_dirty_pack(dslam_engine *e, const dslam_scene *s, int shard, void *send_dev, int capacity_blocks);
int launch_dirty_unpack(dslam_engine *e, dslam_scene *s, int skip_shard, const void *recv_dev, int stride_blocks);
int ensure_scratch(dslam_engine *e, int entries, int local_blocks);
int finish_call(dslam_engine *e);  // synchronise unless the engine is in async mode
int flush_deferred(dslam_engine *e);   // run the calls the engine holds back (dslam_engine::deferred), in order; failures are kept for device_errors()
void defer_call(dslam_engine *e, std::function<int()> body);
int finish_overlapped_allocate(dslam_engine *e, dslam_scene *s);   // alloc.hip: wait for aux_stream, enqueue k_publish_entries
// raycast.hip: GetImage's front end for (M, intr, r's image size) into `front` on aux_stream -- selection over alloc_bits that
// sees the entries the deferring sweep created (hidden_pos), then the range pass -- and the wait that ends it
int launch_front_end_aux(dslam_engine *e, const dslam_scene *s, const dslam_render_state *r, const float *M, const float *intr,
                         FrontEndRecord *front);
int settle_front(dslam_engine *e);
int device_errors(dslam_engine *e);  // report (once) what kernels left in dslam_engine::err_host
int sync_check(dslam_engine *e);   // wait for the engine's stream, then report what kernels left in dslam_engine::err_host
// The host advances its copy of the ticket counters when it enqueues a launch.  A launch the runtime rejected never moves the
// device counters, and every later ticket would then lie in front of its base (the kernels compare unsigned, so such a
// launch does nothing instead of indexing with a negative tile -- but it does nothing).  Any HIP failure bumps a process-
// wide count (hip_fail); an engine that sees a new value drains its stream and reads the counters back.
unsigned long long hip_failure_count();
int tickets_resync(dslam_engine *e);
inline int tickets_ok(dslam_engine *e) { return e->hip_failures_seen == hip_failure_count() ? DSLAM_OK : tickets_resync(e); }
inline int num_tiles(int entries) { return (entries + kTileEntries - 1) / kTileEntries; }
}  // namespace dslam
