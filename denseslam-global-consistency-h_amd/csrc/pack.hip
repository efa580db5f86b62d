// pack.hip -- the device half of the packed-map law (dslam_pack_scene, dslam_unpack_scene; DESIGN.md section 21;
// include/dslam_fusion.h states the layout, pack_host.h the two layout functions and the header's validity).
//
// Reference: none; the law is this project's own.  Every value moved is an integer or a bit pattern.
//
// Pack, all on the engine's stream:
//   ranks     the live list (launch_live_list, live_list.hip): list_a[k] = hash index of the k-th
//             resident entry, its length n read back together with the scene's counters (f = last_free_ex + 1) -- the one
//             wait of a size query, and what a pack needs before it can name blocks_offset;
//   records   k_pack_records: record k = the entry's pos and offset with ptr = its hash index (one 16-byte store per lane),
//             the free excess list verbatim, zeros up to blocks_offset, and the bounding box of the packed positions:
//             per-lane min / max, wave shuffles, the four wave partials through LDS, one integer atomicMin / atomicMax per
//             component and workgroup (integer minima do not depend on the order);
//   header    k_pack_header: 64 bytes by 16 lanes, behind the records kernel (it reads the box);
//   blocks    k_pack_blocks on a fixed grid of kPackGrid workgroups: workgroup w moves blocks w, w + kPackGrid, ...; one
//             256-lane workgroup moves one 4096-byte block per trip, lane t bytes [16 t, 16 t + 16); the pool side is read
//             with the non-temporal policy (nobody comes back for a parked map's blocks), the buffer side -- device or
//             page-locked host memory, written over the fabric as it is -- with plain stores.
// Unpack: the header is read and judged by the host; k_unpack_validate reads records and free list and leaves a verdict
// that the host reads back BEFORE the first write; then the tables are reset (launch_scene_reset_tables), k_unpack_records
// writes entries, free list and the two stack pointers, k_unpack_blocks fills every slot of the pool -- slot N-1-k from
// block k, the other N - n with empty voxels -- and alloc_bits is rebuilt from the table.  The kernels that write bound
// every index they take from the buffer again: a buffer that changes under the call cannot make them write elsewhere.
// Bound: bytes.  2 to 37 VGPRs, no scratch (the compiler's table).
#include <cstring>

#include "dslam_internal.h"
#include "mesh_device.h"
#include "pack_host.h"

namespace dslam {


constexpr int kPackGrid = 512;       // workgroups of the block kernels (two per CU: 128 KiB in flight per trip and CU)
constexpr int kPackThreads = 256;    // one 4096-byte block = 256 lanes x 16 bytes
constexpr int kPackRecordGrid = 256; // workgroups of the record kernels at most (grid-stride beyond)

static inline int record_grid(long long items) {
  const long long wgs = (items + kPackThreads - 1) / kPackThreads;
  return (int)std::min<long long>(std::max<long long>(wgs, 1), kPackRecordGrid);
}

// ---- pack ------------------------------------------------------------------------------------------------------------
__global__ void k_pack_begin(int *bbox) {
  if (threadIdx.x < 3) bbox[threadIdx.x] = 32767;
  else if (threadIdx.x < 6) bbox[threadIdx.x] = -32768;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_records(const HashEntry *__restrict__ hash, const int *__restrict__ ranks,
                                                               const int *__restrict__ excess_list, unsigned char *__restrict__ buf,
                                                               int n, int f, long long blocks_offset, int *bbox) {
  __shared__ int s_box[kPackThreads / 64][6];
  const int gtid = blockIdx.x * kPackThreads + threadIdx.x, stride = gridDim.x * kPackThreads;
  int lo0 = 32767, lo1 = 32767, lo2 = 32767, hi0 = -32768, hi1 = -32768, hi2 = -32768;
  u32x4 *rec = reinterpret_cast<u32x4 *>(buf + kPackHeaderBytes);
  for (int k = gtid; k < n; k += stride) {
    const int t = ranks[k];
    const HashEntry he = load_entry(hash, t);
    u32x4 r;
    r.x = ((unsigned)he.pos[0] & 0xffffu) | ((unsigned)he.pos[1] << 16);
    r.y = (unsigned)he.pos[2] & 0xffffu;   // (_pad = 0)
    r.z = (unsigned)he.offset;
    r.w = (unsigned)t;                     // ptr = the entry's hash index
    if (buf) rec[k] = r;                   // (uniform; no buffer: only the box is taken)
    lo0 = min(lo0, (int)he.pos[0]); lo1 = min(lo1, (int)he.pos[1]); lo2 = min(lo2, (int)he.pos[2]);
    hi0 = max(hi0, (int)he.pos[0]); hi1 = max(hi1, (int)he.pos[1]); hi2 = max(hi2, (int)he.pos[2]);
  }
  // the free excess list verbatim, then zeros up to blocks_offset (the section starts and ends on a 4-byte boundary)
  int *words = reinterpret_cast<int *>(buf + kPackHeaderBytes + kPackRecordBytes * (long long)n);
  const int n_words = (int)((blocks_offset - kPackHeaderBytes - kPackRecordBytes * (long long)n) / 4);   // (f + at most 1023)
  for (int i = gtid; buf && i < n_words; i += stride) words[i] = i < f ? excess_list[i] : 0;
  // bounding box: wave shuffles, wave partials through LDS, one atomic per component and workgroup
  lo0 = wave_min(lo0); lo1 = wave_min(lo1); lo2 = wave_min(lo2);
  hi0 = wave_max(hi0); hi1 = wave_max(hi1); hi2 = wave_max(hi2);
  if ((threadIdx.x & 63) == 0) {
    int *b = s_box[threadIdx.x >> 6];
    b[0] = lo0; b[1] = lo1; b[2] = lo2; b[3] = hi0; b[4] = hi1; b[5] = hi2;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    int v = s_box[0][c];
#pragma unroll
    for (int w = 1; w < kPackThreads / 64; w++) v = c < 3 ? min(v, s_box[w][c]) : max(v, s_box[w][c]);
    if (c < 3) { if (v < 32767) atomicMin(&bbox[c], v); }
    else if (v > -32768) atomicMax(&bbox[c], v);
  }
}

// the header as 16 words (dslam_pack_info's layout); words 12..14 hold the six int16 of the box
struct PackHeaderWords { unsigned w[16]; };
__global__ void k_pack_header(unsigned *__restrict__ buf, PackHeaderWords h, const int *__restrict__ bbox) {
  const int t = threadIdx.x;
  if (t >= 16) return;
  unsigned v = h.w[t];
  if (t >= 12 && t < 15) v = ((unsigned)bbox[2 * (t - 12)] & 0xffffu) | ((unsigned)bbox[2 * (t - 12) + 1] << 16);
  buf[t] = v;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_blocks(const HashEntry *__restrict__ hash, const int *__restrict__ ranks,
                                                              const uint4 *__restrict__ voxels, int n_local,
                                                              uint4 *__restrict__ out /* buf + blocks_offset */, int n) {
  for (int k = blockIdx.x; k < n; k += gridDim.x) {   // (uniform)
    const int ptr = hash[ranks[k]].ptr;
    // (a resident entry names a slot of the pool; a table written behind the engine's back may name anything, and then
    // the block is packed empty -- nothing outside the pool is read)
    uint4 v = make_uint4(kEmptyVoxelLo, kEmptyVoxelHi, kEmptyVoxelLo, kEmptyVoxelHi);
    if ((unsigned)ptr < (unsigned)n_local) v = load_nt(voxels + (size_t)ptr * kPackThreads + threadIdx.x);
    out[(size_t)k * kPackThreads + threadIdx.x] = v;
  }
}

// What a pack (or its size query) has to know first: n and the counters, behind everything enqueued so far.
static int pack_counts(dslam_engine *e, const dslam_scene *s, int *n_out, int *f_out) {
  DSLAM_TRY(ensure_scratch(e, s->n_entries, s->p.num_local_blocks));
  int *count = e->misc_counter + 8;
  DSLAM_TRY(launch_live_list(e, s, e->list_a, count));
  DSLAM_HIP(hipGetLastError());
  char *host = reinterpret_cast<char *>(e->pinned.get());
  SceneCounters *sc = reinterpret_cast<SceneCounters *>(host);
  int *n_host = reinterpret_cast<int *>(host + 256);
  DSLAM_HIP(hipMemcpyAsync(sc, s->counters, sizeof(SceneCounters), hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipMemcpyAsync(n_host, count, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_TRY(sync_check(e));
  const int n = *n_host, f = sc->last_free_ex + 1;
  DSLAM_REQUIRE(n >= 0 && n <= s->n_entries && f >= 0 && f <= s->p.num_excess, "the scene's counters are not those of a map");
  *n_out = n; *f_out = f;
  return DSLAM_OK;
}

static void fill_header(const dslam_scene *s, int n, int f, dslam_pack_info *h) {
  memset(h, 0, sizeof *h);
  memcpy(h->magic, "DSPK", 4);
  h->version = 1;
  h->num_buckets = s->p.num_buckets; h->num_excess = s->p.num_excess;
  h->blocks = n; h->free_excess = f;
  memcpy(&h->voxel_size_bits, &s->p.voxel_size, 4);
  memcpy(&h->mu_bits, &s->p.mu, 4);
  int64_t off, total;
  pack_layout(n, f, &off, &total);
  h->blocks_offset = off; h->total_bytes = total;
  for (int c = 0; c < 3; c++) { h->bbox_min[c] = 32767; h->bbox_max[c] = -32768; }
}

// Is [p, p + bytes) memory the engine's device can address -- device memory of that device or page-locked host memory -- and
// 16-byte aligned?  Asks about the first and the last byte; *dev_out: the first byte as the device addresses it.
int pack_buffer_address(dslam_engine *e, const void *p, int64_t bytes, void **dev_out) {
  DSLAM_REQUIRE(p && bytes > 0 && ((uintptr_t)p & 15u) == 0, "the buffer of a packed map must be 16-byte aligned");
  const char *ends[2] = {static_cast<const char *>(p), static_cast<const char *>(p) + bytes - 1};
  for (int i = 0; i < 2; i++) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof attr);
    const hipError_t err = hipPointerGetAttributes(&attr, ends[i]);
    if (err != hipSuccess) (void)hipGetLastError();   // (an answer, not a failure of the runtime)
    const bool device = err == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == e->device;
    const bool pinned = err == hipSuccess && attr.type == hipMemoryTypeHost;
    DSLAM_REQUIRE(device || pinned, "the buffer of a packed map must be device memory of the engine's device or page-locked host memory");
    if (i == 0) *dev_out = attr.devicePointer ? attr.devicePointer : const_cast<void *>(p);
  }
  return DSLAM_OK;
}

// scene already checked by dslam_pack_scene; buf: the caller's pointer, null for the size query
int launch_pack_scene(dslam_engine *e, const dslam_scene *s, void *buf_user, int64_t capacity, dslam_pack_info *info) {
  void *buf_dev = nullptr;
  if (buf_user) DSLAM_TRY(pack_buffer_address(e, buf_user, 1, &buf_dev));   // (before anything is launched)
  int n = 0, f = 0;
  DSLAM_TRY(pack_counts(e, s, &n, &f));
  fill_header(s, n, f, info);
  const bool write = buf_user && capacity >= info->total_bytes;
  if (write) DSLAM_TRY(pack_buffer_address(e, buf_user, info->total_bytes, &buf_dev));   // (its last byte too)
  // a size query (and a buffer that is too small) run the records kernel without a buffer: it takes the box, which the
  // header they return owes, and stores nothing
  unsigned char *buf = write ? static_cast<unsigned char *>(buf_dev) : nullptr;
  int *bbox = e->misc_counter + 10;
  hipLaunchKernelGGL(k_pack_begin, dim3(1), dim3(64), 0, e->stream, bbox);
  const long long items = std::max<long long>(n, (info->blocks_offset - kPackHeaderBytes - kPackRecordBytes * (long long)n) / 4);
  hipLaunchKernelGGL(k_pack_records, dim3(record_grid(items)), dim3(kPackThreads), 0, e->stream, s->hash.get(), e->list_a.get(),
                     s->excess_list.get(), buf, n, f, (long long)info->blocks_offset, bbox);
  if (write) {
    PackHeaderWords hw;
    memcpy(hw.w, info, sizeof hw.w);
    hipLaunchKernelGGL(k_pack_header, dim3(1), dim3(64), 0, e->stream, reinterpret_cast<unsigned *>(buf), hw, bbox);
    if (n > 0)
      hipLaunchKernelGGL(k_pack_blocks, dim3(std::min(n, kPackGrid)), dim3(kPackThreads), 0, e->stream, s->hash.get(),
                         e->list_a.get(), reinterpret_cast<const uint4 *>(s->voxels), s->p.num_local_blocks,
                         reinterpret_cast<uint4 *>(buf + info->blocks_offset), n);
  }
  DSLAM_HIP(hipGetLastError());
  // the box goes into the caller's copy of the header too; the wait is the one that makes the buffer complete
  int *box_host = reinterpret_cast<int *>(reinterpret_cast<char *>(e->pinned.get()) + 320);
  DSLAM_HIP(hipMemcpyAsync(box_host, bbox, 6 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_TRY(sync_check(e));
  for (int c = 0; c < 3; c++) { info->bbox_min[c] = (int16_t)box_host[c]; info->bbox_max[c] = (int16_t)box_host[3 + c]; }
  DSLAM_REQUIRE(!buf_user || write, "the buffer is smaller than the packed map (ask with buf = NULL)");
  return DSLAM_OK;
}

// ---- unpack ----------------------------------------------------------------------------------------------------------
// Read-only: bit 0 of *verdict is set for a record index outside the table or not above its predecessor's, bit 1 for an
// offset outside [0, num_excess], bit 2 for a free value outside [0, num_excess).
__global__ __launch_bounds__(kPackThreads) void k_unpack_validate(const unsigned char *__restrict__ buf, int n, int f, int n_entries,
                                                                  int num_excess, int *verdict) {
  const int gtid = blockIdx.x * kPackThreads + threadIdx.x, stride = gridDim.x * kPackThreads;
  const u32x4 *rec = reinterpret_cast<const u32x4 *>(buf + kPackHeaderBytes);
  const int *free_list = reinterpret_cast<const int *>(buf + kPackHeaderBytes + kPackRecordBytes * (long long)n);
  int bad = 0;
  for (int k = gtid; k < n; k += stride) {
    const u32x4 r = rec[k];
    const int idx = (int)r.w, offset = (int)r.z;
    if ((unsigned)idx >= (unsigned)n_entries) bad |= 1;
    if (k > 0 && reinterpret_cast<const int *>(rec)[4 * (size_t)(k - 1) + 3] >= idx) bad |= 1;
    if (offset < 0 || offset > num_excess) bad |= 2;
  }
  for (int i = gtid; i < f; i += stride)
    if ((unsigned)free_list[i] >= (unsigned)num_excess) bad |= 4;
  if (bad) atomicOr(verdict, bad);
}

__global__ __launch_bounds__(kPackThreads) void k_unpack_records(const unsigned char *__restrict__ buf, int n, int f, HashEntry *hash,
                                                                 int n_entries, int n_local, int *excess_list, int num_excess,
                                                                 SceneCounters *cnt) {
  const int gtid = blockIdx.x * kPackThreads + threadIdx.x, stride = gridDim.x * kPackThreads;
  const u32x4 *rec = reinterpret_cast<const u32x4 *>(buf + kPackHeaderBytes);
  const int *free_list = reinterpret_cast<const int *>(buf + kPackHeaderBytes + kPackRecordBytes * (long long)n);
  for (int k = gtid; k < n; k += stride) {
    u32x4 r = rec[k];
    const int idx = (int)r.w;
    // validated, and judged again on the value this lane has just read: the address below depends on the index, and an
    // offset outside [0, num_excess] left in the table would send a later chain walk out of it.  A record that fails now
    // (the buffer changed under the call) is skipped: its entry stays the reset entry
    if ((unsigned)idx >= (unsigned)n_entries || (unsigned)r.z > (unsigned)num_excess) continue;
    r.y &= 0xffffu;
    r.w = (unsigned)(n_local - 1 - k);
    *reinterpret_cast<u32x4 *>(hash + idx) = r;
  }
  for (int i = gtid; i < f && i < num_excess; i += stride) {
    const int v = free_list[i];
    if ((unsigned)v < (unsigned)num_excess) excess_list[i] = v;   // (likewise: otherwise the reset's value stays)
  }
  if (gtid == 0) {
    cnt->last_free = n_local - 1 - n;
    cnt->last_free_ex = f - 1;
  }
}

// every slot of the pool: slot j < N - n empty, slot N-1-k block k
__global__ __launch_bounds__(kPackThreads) void k_unpack_blocks(const uint4 *__restrict__ in /* buf + blocks_offset */, int n,
                                                                uint4 *__restrict__ voxels, int n_local) {
  for (int j = blockIdx.x; j < n_local; j += gridDim.x) {   // (uniform)
    const int k = n_local - 1 - j;
    uint4 v = make_uint4(kEmptyVoxelLo, kEmptyVoxelHi, kEmptyVoxelLo, kEmptyVoxelHi);
    if (k < n) {
      const u32x4 r = *reinterpret_cast<const u32x4 *>(in + (size_t)k * kPackThreads + threadIdx.x);
      v = make_uint4(r.x, r.y, r.z, r.w);
    }
    store_nt(voxels + (size_t)j * kPackThreads + threadIdx.x, v);
  }
}

// The read-only half: header (already judged by the host) against the buffer's records.  DSLAM_ERR_INVALID for a bad image.
int launch_unpack_validate(dslam_engine *e, const dslam_scene *s, const void *buf_dev, const dslam_pack_info *h) {
  int *verdict = e->misc_counter + 10;
  DSLAM_HIP(hipMemsetAsync(verdict, 0, sizeof(int), e->stream));
  const int n = h->blocks, f = h->free_excess;
  hipLaunchKernelGGL(k_unpack_validate, dim3(record_grid(std::max(n, f))), dim3(kPackThreads), 0, e->stream,
                     static_cast<const unsigned char *>(buf_dev), n, f, s->n_entries, s->p.num_excess, verdict);
  DSLAM_HIP(hipGetLastError());
  int *host = reinterpret_cast<int *>(reinterpret_cast<char *>(e->pinned.get()) + 256);
  DSLAM_HIP(hipMemcpyAsync(host, verdict, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  DSLAM_TRY(sync_check(e));
  DSLAM_REQUIRE(!(*host & 1), "a record index of the packed map is outside the table or not ascending");
  DSLAM_REQUIRE(!(*host & 2), "a record of the packed map has an offset outside [0, num_excess]");
  DSLAM_REQUIRE(!(*host & 4), "a free excess value of the packed map is outside [0, num_excess)");
  return DSLAM_OK;
}

// The writing half, everything validated.  Enqueues only; the caller waits.
int launch_unpack_write(dslam_engine *e, dslam_scene *s, const void *buf_dev, const dslam_pack_info *h) {
  const unsigned char *buf = static_cast<const unsigned char *>(buf_dev);
  const int n = h->blocks, f = h->free_excess, N = s->p.num_local_blocks;
  DSLAM_TRY(launch_scene_reset_tables(e, s));
  hipLaunchKernelGGL(k_unpack_records, dim3(record_grid(std::max(n, f))), dim3(kPackThreads), 0, e->stream, buf, n, f, s->hash.get(),
                     s->n_entries, N, s->excess_list.get(), s->p.num_excess, s->counters.get());
  hipLaunchKernelGGL(k_unpack_blocks, dim3(std::min(N, kPackGrid)), dim3(kPackThreads), 0, e->stream,
                     reinterpret_cast<const uint4 *>(buf + h->blocks_offset), n, reinterpret_cast<uint4 *>(s->voxels), N);
  DSLAM_HIP(hipGetLastError());
  return launch_build_alloc_bits(e, s);
}

}  // namespace dslam
