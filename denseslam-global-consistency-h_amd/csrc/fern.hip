// fern.hip -- the fern keyframe index: place recognition on the device (dslam_fern_*; FernRelocLib's ProcessFrame in the
// reference's empty submodule).
//
// Reference: none that can be compared.  The law is this project's own (include/dslam_fusion.h states
// it in full) and all-integer: thumbnails by integer sums and floor divisions, decisions by integer comparisons, the
// dissimilarity a count, the order of a query (dissimilarity, id).  So the result is exact and the same on every run
// however the work is split.
//
// Device work:
//   k_fern_thumbs   the images once: a workgroup takes one row of cells (a run of at most kFernChunkCells of them) of one image.
//                   A lane owns kVec consecutive pixel columns and walks the cell's c pixel rows, so a wave's loads are
//                   consecutive 16-byte pieces of a depth row (8 pixels per lane: several cells per wave) when the rows are
//                   16-byte aligned, and single pixels otherwise; the column sums stay in registers, are added up along the
//                   lane's columns while the cell stays the same and go to the cell's LDS word by an integer add (n and S in
//                   one 64-bit word).  D and G go to the index's thumbnail scratch.
//   k_fern_codes    behind it in the stream, so it sees complete thumbnails: one workgroup per image, a thread evaluates two
//                   ferns (8 gathers from the thumbnail) into a byte, LDS assembles the 64 dwords.
//   k_fern_scan     a code is one dword per lane of a wave64: a wave takes one stored code with one coalesced 256-byte load,
//                   XORs it with the query's dword from LDS, counts the non-zero nibbles and adds over the wave -- three
//                   queries at a time in 10-bit fields of one word.  With many queries (up to 64: 16 KiB of LDS) each stored
//                   code is still loaded once.  The counts go to dist[q][id] (2 bytes each).
//   k_fern_select_slices / k_fern_select_merge
//                   the k best of a window by (dissimilarity, id) out of dist: per slice of the window a histogram over the
//                   513 possible dissimilarities finds the value at which the k-th falls, everything below it is taken, and
//                   of the entries AT it the first in id order (an ordered scan); the at most 64 keys taken are then ranked
//                   against each other.  Keys are unique, so the set and its order are fixed by the law alone: the only
//                   atomics are integer counts and slot numbers of a set that is sorted afterwards.  More than one slice:
//                   a second launch selects among the slices' keys the same way.
//   k_fern_append   dslam_fern_process: the harvest decision from the smallest dissimilarity over all ids (an integer
//                   atomicMin of the scan) and the copy of the code to its place.
// No float anywhere, no workgroup waits for another, no private memory.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "dslam_internal.h"

namespace dslam {

namespace {

constexpr int kFernThreads = 256;
constexpr int kFernChunkCells = 2048;      // cells of one workgroup of k_fern_thumbs: 256 lanes x 8 columns at cell 1
constexpr int kFernMaxSlices = 64;         // slices of a window in k_fern_select_slices
constexpr int kFernSliceIds = 8192;        // ... of this many ids, unless that would take more slices
constexpr int kScanBatch = 4;              // stored codes a wave of k_fern_scan has in flight
constexpr int kFernBins =DSLAM_FERN_CODE_DWORDS * 8 + 1;   // dissimilarities 0 .. 512
constexpr size_t kFernThumbBytes = (size_t)64 << 20;        // the thumbnail scratch never grows past this
constexpr unsigned kNoKey = 0xffffffffu;   // an absent key: sorts behind every real one ((dissimilarity << 22) | id)
// what a call reads back: [0 .. 64) the number of matches per query, [64] the smallest dissimilarity over all ids,
// [65] the id dslam_fern_process appended or -1, [66] it should have appended but the index is full; from [128] on the
// keys, 64 per query
constexpr int kResCounts = 0, kResMin = 64, kResAdded = 65, kResFull = 66, kResKeys = 128;
constexpr int kResWords = kResKeys + DSLAM_FERN_MAX_QUERIES * DSLAM_FERN_MAX_MATCHES;
static_assert(DSLAM_FERN_MAX_MATCHES == 64 && DSLAM_FERN_MAX_QUERIES == 64 && DSLAM_FERN_CODE_DWORDS == 64, "one wave64");

struct FernThumbArgs {
  const unsigned char *depth;    // slot 0's depth image; slot s at + s depth_slot_bytes
  const unsigned char *rgba;
  size_t depth_slot_bytes, rgba_slot_bytes;
  unsigned short *thumbs;        // [slots][2][cells]
  int w, cell, tw, th, channels;
  int chunk_cells, chunks;       // cells of a workgroup's run, runs per row of cells
};

// kVec = 8: the pixel rows are 16-byte aligned (depth) and 32-byte aligned pieces of them never straddle the used columns;
// kVec = 1: any size and address
template <int kVec>
__global__ __launch_bounds__(kFernThreads) void k_fern_thumbs(FernThumbArgs p) {
  __shared__ unsigned long long s_acc[kFernChunkCells];   // n << 32 | S
  __shared__ int s_grey[kFernChunkCells];
  const int tid = threadIdx.x;
  const int ty = (int)blockIdx.x / p.chunks, chunk = (int)blockIdx.x - ty * p.chunks;   // (uniform)
  const int slot = blockIdx.y;
  const int cell0 = chunk * p.chunk_cells;
  const int ncell = min(p.chunk_cells, p.tw - cell0);
  for (int i = tid; i < ncell; i += kFernThreads) { s_acc[i] = 0ull; s_grey[i] = 0; }
  __syncthreads();
  const int c = p.cell;
  const int rel0 = tid * kVec;                   // first column of this lane, counted from the run's first
  const int ncol = ncell * c;                    // columns of the run (kVec = 8: a multiple of 8)
  if (rel0 < ncol) {
    const size_t pix0 = (size_t)ty * c * p.w + (size_t)cell0 * c + rel0;
    const short *drow = reinterpret_cast<const short *>(p.depth + (size_t)slot * p.depth_slot_bytes) + pix0;
    const unsigned *crow = reinterpret_cast<const unsigned *>(p.rgba + (size_t)slot * p.rgba_slot_bytes) + pix0;
    int n[kVec], S[kVec], g[kVec];
#pragma unroll
    for (int j = 0; j < kVec; j++) { n[j] = 0; S[j] = 0; g[j] = 0; }
    for (int r = 0; r < c; r++) {
      int mm[kVec];
      if constexpr (kVec == 8) {
        const uint4 v = *reinterpret_cast<const uint4 *>(drow);
        mm[0] = (short)(v.x & 0xffffu); mm[1] = (short)(v.x >> 16);
        mm[2] = (short)(v.y & 0xffffu); mm[3] = (short)(v.y >> 16);
        mm[4] = (short)(v.z & 0xffffu); mm[5] = (short)(v.z >> 16);
        mm[6] = (short)(v.w & 0xffffu); mm[7] = (short)(v.w >> 16);
      } else {
        mm[0] = drow[0];
      }
#pragma unroll
      for (int j = 0; j < kVec; j++)
        if (mm[j] > 0) { n[j]++; S[j] += mm[j]; }
      if (p.channels == 2) {   // (uniform)
        unsigned px[kVec];
        if constexpr (kVec == 8) {
          const uint4 a = reinterpret_cast<const uint4 *>(crow)[0], b = reinterpret_cast<const uint4 *>(crow)[1];
          px[0] = a.x; px[1] = a.y; px[2] = a.z; px[3] = a.w;
          px[4] = b.x; px[5] = b.y; px[6] = b.z; px[7] = b.w;
        } else {
          px[0] = crow[0];
        }
#pragma unroll
        for (int j = 0; j < kVec; j++) g[j] += (int)(px[j] & 0xffu) + 2 * (int)((px[j] >> 8) & 0xffu) + (int)((px[j] >> 16) & 0xffu);
      }
      drow += p.w;
      crow += p.w;
    }
    // along the lane's columns: one LDS add per cell the lane touches
    int cellrel = rel0 / c, rem = rel0 - cellrel * c;
    int rn = 0, rS = 0, rg = 0;
#pragma unroll
    for (int j = 0; j < kVec; j++) {
      if (rel0 + j < ncol) { rn += n[j]; rS += S[j]; rg += g[j]; }
      rem++;
      if (rem == c || j == kVec - 1) {
        if (cellrel < ncell) {
          atomicAdd(&s_acc[cellrel], ((unsigned long long)(unsigned)rn << 32) | (unsigned long long)(unsigned)rS);
          if (p.channels == 2) atomicAdd(&s_grey[cellrel], rg);
        }
        rn = 0; rS = 0; rg = 0;
      }
      if (rem == c) { rem = 0; cellrel++; }
    }
  }
  __syncthreads();
  const size_t cells = (size_t)p.tw * p.th;
  unsigned short *out = p.thumbs + (size_t)slot * 2 * cells + (size_t)ty * p.tw + cell0;
  for (int i = tid; i < ncell; i += kFernThreads) {
    const unsigned long long acc = s_acc[i];
    const int nn = (int)(acc >> 32), SS = (int)(unsigned)acc;
    out[i] = (unsigned short)(2 * nn >= c * c ? SS / nn : 0);   // (2 n >= c c implies n >= 1)
    out[cells + i] = (unsigned short)(s_grey[i] / (4 * c * c));
  }
}

struct FernCodeArgs {
  const unsigned short *thumbs;  // [slots][2][cells]
  const int2 *table;             // [F][4] {2 cell + channel, threshold}
  unsigned *out;                 // code of slot s at out + s * 64
  unsigned *min_init;            // dslam_fern_process: the scan's minimum starts at "none"; or null
  int cells, num_ferns;
};

__global__ __launch_bounds__(kFernThreads) void k_fern_codes(FernCodeArgs p) {
  __shared__ unsigned s_words[DSLAM_FERN_CODE_DWORDS];
  const int tid = threadIdx.x;
  const unsigned short *th = p.thumbs + (size_t)blockIdx.x * 2 * p.cells;
  unsigned byte = 0;
  const int f0 = 2 * tid;   // (F is a multiple of 8: a pair of ferns is in or out together)
  if (f0 < p.num_ferns) {
#pragma unroll
    for (int d = 0; d < 8; d++) {
      const int2 dec = p.table[f0 * 4 + d];
      const int value = th[(size_t)(dec.x & 1) * p.cells + (dec.x >> 1)];
      byte |= (value > dec.y ? 1u : 0u) << d;
    }
  }
  reinterpret_cast<unsigned char *>(s_words)[tid] = (unsigned char)byte;   // byte k of dword l: ferns 8 l + 2 k, 8 l + 2 k + 1
  __syncthreads();
  if (tid < DSLAM_FERN_CODE_DWORDS) p.out[(size_t)blockIdx.x * DSLAM_FERN_CODE_DWORDS + tid] = s_words[tid];
  if (p.min_init && blockIdx.x == 0 && tid == 0) *p.min_init = kNoKey;
}

struct FernScanArgs {
  const unsigned *codes;         // [count][64]
  const unsigned *qbase;         // query q's code at qbase + qidx[q] * 64
  const int *qidx;
  unsigned short *dist;          // [nq][stride]
  size_t stride;
  unsigned *min_all;             // smallest dissimilarity of query 0 over [lo, hi), by atomicMin; or null
  int lo, hi, nq;
};

__device__ __forceinline__ unsigned nonzero_nibbles(unsigned x) {
  x |= x >> 1;
  x |= x >> 2;
  return (unsigned)__popc(x & 0x11111111u);
}

__global__ __launch_bounds__(kFernThreads) void k_fern_scan(FernScanArgs p) {
  __shared__ unsigned s_q[DSLAM_FERN_MAX_QUERIES * DSLAM_FERN_CODE_DWORDS];
  __shared__ unsigned s_min;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nq = p.nq;
  for (int i = tid; i < nq * 64; i += kFernThreads) s_q[i] = p.qbase[(size_t)p.qidx[i >> 6] * 64 + (i & 63)];
  if (tid == 0) s_min = kNoKey;
  __syncthreads();
  const int waves = (int)gridDim.x * (kFernThreads / 64);
  unsigned wmin = kNoKey;
  // kScanBatch stored codes per wave and round, their loads in flight together: with one load per round the wave waits out a
  // whole memory round trip per code
  for (int id0 = p.lo + (int)blockIdx.x * (kFernThreads / 64) + (tid >> 6); id0 < p.hi; id0 += waves * kScanBatch) {   // (uniform per wave)
    unsigned d[kScanBatch];
#pragma unroll
    for (int b = 0; b < kScanBatch; b++) {
      const int id = id0 + b * waves;
      d[b] = id < p.hi ? p.codes[(size_t)id * 64 + lane] : 0u;
    }
#pragma unroll
    for (int b = 0; b < kScanBatch; b++) {
      const int id = id0 + b * waves;
      if (id >= p.hi) continue;   // (uniform per wave)
      unsigned mine = 0;
      for (int q0 = 0; q0 < nq; q0 += 3) {
        unsigned w = nonzero_nibbles(d[b] ^ s_q[q0 * 64 + lane]);   // (at most 8 per lane, 512 per wave: 10 bits)
        if (q0 + 1 < nq) w |= nonzero_nibbles(d[b] ^ s_q[(q0 + 1) * 64 + lane]) << 10;
        if (q0 + 2 < nq) w |= nonzero_nibbles(d[b] ^ s_q[(q0 + 2) * 64 + lane]) << 20;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        const int r = lane - q0;
        if (r >= 0 && r < 3) mine = (w >> (10 * r)) & 1023u;
      }
      if (lane < nq) p.dist[(size_t)lane * p.stride + id] = (unsigned short)mine;   // lane q holds query q's count
      if (lane == 0) wmin = min(wmin, mine);
    }
  }
  if (p.min_all) {   // (uniform)
    if (lane == 0 && wmin != kNoKey) atomicMin(&s_min, wmin);
    __syncthreads();
    if (tid == 0 && s_min != kNoKey) atomicMin(p.min_all, s_min);
  }
}

// The k smallest of the keys load(0 .. n) -- kNoKey: none -- to out[0 .. k), ascending, padded with kNoKey; returns their
// number.  Keys are (dissimilarity << 22) | id and unique; among keys of one dissimilarity the id ascends with the position.
template <class Load>
__device__ __forceinline__ int select_k(const Load &load, int n, int k, unsigned *out) {
  __shared__ int s_hist[kFernBins + 3];
  __shared__ int s_red[kFernThreads / 64];
  __shared__ unsigned s_keys[DSLAM_FERN_MAX_MATCHES];
  __shared__ int s_cut, s_below, s_count_a;
  const int tid = threadIdx.x;
  for (int i = tid; i < kFernBins + 3; i += kFernThreads) s_hist[i] = 0;
  if (tid == 0) s_count_a = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kFernThreads) {
    const unsigned key = load(i);
    if (key != kNoKey) atomicAdd(&s_hist[min((int)(key >> 22), kFernBins - 1)], 1);
  }
  __syncthreads();
  // the dissimilarity at which the k-th key falls: thread t looks at the bins 3 t .. 3 t + 2
  int h[3] = {0, 0, 0};
  if (3 * tid < kFernBins) { h[0] = s_hist[3 * tid]; h[1] = s_hist[3 * tid + 1]; h[2] = s_hist[3 * tid + 2]; }
  int total;
  int before = block_excl_scan<kFernThreads / 64>(h[0] + h[1] + h[2], s_red, total);
  if (total < k) {
    if (tid == 0) { s_cut = kFernBins; s_below = total; }   // everything is taken
  } else {
#pragma unroll
    for (int b = 0; b < 3; b++) {
      if (before < k && before + h[b] >= k) { s_cut = 3 * tid + b; s_below = before; }   // (exactly one thread and bin)
      before += h[b];
    }
  }
  __syncthreads();
  const int cut = s_cut, below = s_below;
  const int at_cut = cut < kFernBins ? k - below : 0;   // how many of the keys AT the cut are taken: the first in id order
  int seen = 0;
  for (int base = 0; base < n; base += kFernThreads) {   // (uniform)
    const int i = base + tid;
    const unsigned key = i < n ? load(i) : kNoKey;
    const int d = (int)(key >> 22);
    if (key != kNoKey && d < cut) s_keys[atomicAdd(&s_count_a, 1)] = key;   // (any slot below `below`: ranked afterwards)
    const bool at = key != kNoKey && d == cut;
    int chunk_total;
    const int rank = block_excl_scan<kFernThreads / 64>(at ? 1 : 0, s_red, chunk_total);
    if (at && seen + rank < at_cut) s_keys[below + seen + rank] = key;
    seen += chunk_total;
  }
  __syncthreads();
  const int taken = min(total, k);
  if (tid < DSLAM_FERN_MAX_MATCHES) {
    const unsigned mine = tid < taken ? s_keys[tid] : kNoKey;
    int rank = 0;
    for (int j = 0; j < taken; j++) rank += s_keys[j] < mine ? 1 : 0;
    if (tid < taken) out[rank] = mine;
    else if (tid < k) out[tid] = kNoKey;
  }
  return taken;
}

struct FernSelectArgs {
  const unsigned short *dist;
  size_t stride;
  unsigned *partial;             // [nq][slices][64]
  unsigned *result;              // FernResult
  int lo, hi, slice_ids, slices, k;
};

__global__ __launch_bounds__(kFernThreads) void k_fern_select_slices(FernSelectArgs p) {
  const int g = blockIdx.x, q = blockIdx.y;
  const int a = p.lo + g * p.slice_ids;
  const int n = max(0, min(p.hi, a + p.slice_ids) - a);
  const unsigned short *row = p.dist + (size_t)q * p.stride + a;
  const auto load = [row, a](int i) { return ((unsigned)row[i] << 22) | (unsigned)(a + i); };
  unsigned *out = p.slices == 1 ? p.result + kResKeys + q * DSLAM_FERN_MAX_MATCHES
                                : p.partial + ((size_t)q * p.slices + g) * DSLAM_FERN_MAX_MATCHES;
  const int taken = select_k(load, n, p.k, out);
  if (p.slices == 1 && threadIdx.x == 0) p.result[kResCounts + q] = (unsigned)taken;
}

__global__ __launch_bounds__(kFernThreads) void k_fern_select_merge(FernSelectArgs p) {
  const int q = blockIdx.x;
  const unsigned *in = p.partial + (size_t)q * p.slices * DSLAM_FERN_MAX_MATCHES;
  const int k = p.k;
  const auto load = [in, k](int i) { const int g = i / k; return in[g * DSLAM_FERN_MAX_MATCHES + (i - g * k)]; };
  const int taken = select_k(load, p.slices * k, k, p.result + kResKeys + q * DSLAM_FERN_MAX_MATCHES);
  if (threadIdx.x == 0) p.result[kResCounts + q] = (unsigned)taken;
}

// one wave: dslam_fern_process' harvest rule
__global__ __launch_bounds__(64) void k_fern_append(unsigned *codes, const unsigned *qcode, int count, int capacity, int harvest,
                                                    unsigned *result) {
  const unsigned smallest = result[kResMin];   // (kNoKey when nothing is stored)
  const bool want = count == 0 || smallest >= (unsigned)harvest;
  const bool room = count < capacity;
  if (want && room) codes[(size_t)count * DSLAM_FERN_CODE_DWORDS + threadIdx.x] = qcode[threadIdx.x];
  if (threadIdx.x == 0) {
    result[kResAdded] = want && room ? (unsigned)count : kNoKey;
    result[kResFull] = want && !room ? 1u : 0u;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------

struct FernImages {
  const unsigned char *depth, *rgba;
  size_t depth_slot_bytes, rgba_slot_bytes;
  int slots;
};

size_t thumb_slot_bytes(const dslam_fern_index *idx) { return (size_t)idx->tw * idx->th * 2 * sizeof(unsigned short); }

int ensure_thumbs(dslam_engine *e, dslam_fern_index *idx, int slots) {
  if (slots <= idx->thumb_slots) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  FernThumbs n;
  DSLAM_TRY(n.thumbs.alloc((size_t)slots * idx->tw * idx->th * 2));
  n.thumb_slots = slots;
  static_cast<FernThumbs &>(*idx) = std::move(n);
  return DSLAM_OK;
}

int ensure_rows(dslam_engine *e, dslam_fern_index *idx, int nq) {
  const int rows = nq > 1 ? DSLAM_FERN_MAX_QUERIES : 1;
  if (rows <= idx->rows) return DSLAM_OK;
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  FernRows n;
  DSLAM_TRY(n.dist.alloc((size_t)rows * idx->dist_stride));
  DSLAM_TRY(n.partial.alloc((size_t)rows * kFernMaxSlices * DSLAM_FERN_MAX_MATCHES));
  n.rows = rows;
  static_cast<FernRows &>(*idx) = std::move(n);
  return DSLAM_OK;
}

// the codes of `im.slots` images to out + s * 64: two launches per batch that fits the thumbnail scratch (enqueue only)
int enqueue_encode(dslam_engine *e, dslam_fern_index *idx, const FernImages &im, unsigned *out, unsigned *min_init) {
  const int per_batch = (int)std::max<size_t>(1, std::min<size_t>(kFernThumbBytes / thumb_slot_bytes(idx), 32768));
  DSLAM_TRY(ensure_thumbs(e, idx, std::min(im.slots, per_batch)));
  const int c = idx->p.cell;
  // wide loads: every pixel row of every image starts on a 16-byte boundary and a lane's 8 columns never straddle the end of
  // the used columns (c divides 8 or 8 divides c, with W a multiple of 8)
  const bool wide = idx->w % 8 == 0 && (8 % c == 0 || c % 8 == 0) && ((uintptr_t)im.depth & 15) == 0 && im.depth_slot_bytes % 16 == 0 &&
                    (idx->p.channels == 1 || (((uintptr_t)im.rgba & 15) == 0 && im.rgba_slot_bytes % 16 == 0));
  const int vec = wide ? 8 : 1;
  FernThumbArgs ta;
  memset(&ta, 0, sizeof ta);
  ta.depth_slot_bytes = im.depth_slot_bytes; ta.rgba_slot_bytes = im.rgba_slot_bytes;
  ta.thumbs = idx->thumbs;
  ta.w = idx->w; ta.cell = c; ta.tw = idx->tw; ta.th = idx->th; ta.channels = idx->p.channels;
  ta.chunk_cells = std::min(idx->tw, kFernThreads * vec / c);   // (>= 8: c <= 32)
  ta.chunks = (idx->tw + ta.chunk_cells - 1) / ta.chunk_cells;
  FernCodeArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.thumbs = idx->thumbs; ca.table = idx->table_dev;
  ca.cells = idx->tw * idx->th; ca.num_ferns = idx->p.num_ferns;
  for (int first = 0; first < im.slots; first += per_batch) {
    const int n = std::min(per_batch, im.slots - first);
    ta.depth = im.depth + (size_t)first * im.depth_slot_bytes;
    ta.rgba = im.rgba + (size_t)first * im.rgba_slot_bytes;
    const dim3 grid((unsigned)(ta.chunks * idx->th), (unsigned)n);
    if (wide) hipLaunchKernelGGL(k_fern_thumbs<8>, grid, dim3(kFernThreads), 0, e->stream, ta);
    else hipLaunchKernelGGL(k_fern_thumbs<1>, grid, dim3(kFernThreads), 0, e->stream, ta);
    DSLAM_HIP(hipGetLastError());
    ca.out = out + (size_t)first * DSLAM_FERN_CODE_DWORDS;
    ca.min_init = first == 0 ? min_init : nullptr;
    hipLaunchKernelGGL(k_fern_codes, dim3((unsigned)n), dim3(kFernThreads), 0, e->stream, ca);
    DSLAM_HIP(hipGetLastError());
  }
  return DSLAM_OK;
}

FernImages view_images(const dslam_view *v) {
  return {reinterpret_cast<const unsigned char *>(v->raw_src), reinterpret_cast<const unsigned char *>(v->rgba_src), 0, 0, 1};
}

// dist of the queries against [scan_lo, scan_hi), then the k best of [lo, hi) per query into the result block (enqueue only;
// lo <= hi, both already clipped to [0, count))
int enqueue_search(dslam_engine *e, dslam_fern_index *idx, const unsigned *qbase, int nq, int scan_lo, int scan_hi, bool want_min,
                   int lo, int hi, int k) {
  DSLAM_TRY(ensure_rows(e, idx, nq));
  unsigned *res = idx->result;
  if (scan_hi > scan_lo) {
    FernScanArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.codes = idx->codes; sa.qbase = qbase; sa.qidx = idx->query_ids.device();
    sa.dist = idx->dist; sa.stride = idx->dist_stride;
    sa.min_all = want_min ? res + kResMin : nullptr;
    sa.lo = scan_lo; sa.hi = scan_hi; sa.nq = nq;
    // a round of kScanBatch codes per wave while the grid can grow; then the waves loop
    const int per_group = (kFernThreads / 64) * kScanBatch;
    const int grid = std::max(1, std::min(4096, (scan_hi - scan_lo + per_group - 1) / per_group));
    hipLaunchKernelGGL(k_fern_scan, dim3(grid), dim3(kFernThreads), 0, e->stream, sa);
    DSLAM_HIP(hipGetLastError());
  }
  FernSelectArgs se;
  memset(&se, 0, sizeof se);
  se.dist = idx->dist; se.stride = idx->dist_stride; se.partial = idx->partial; se.result = res;
  se.lo = lo; se.hi = hi; se.k = k;
  const int n = hi - lo;
  se.slices = std::max(1, std::min(kFernMaxSlices, (n + kFernSliceIds - 1) / kFernSliceIds));
  se.slice_ids = std::max(1, (n + se.slices - 1) / se.slices);
  hipLaunchKernelGGL(k_fern_select_slices, dim3((unsigned)se.slices, (unsigned)nq), dim3(kFernThreads), 0, e->stream, se);
  DSLAM_HIP(hipGetLastError());
  if (se.slices > 1) {
    hipLaunchKernelGGL(k_fern_select_merge, dim3((unsigned)nq), dim3(kFernThreads), 0, e->stream, se);
    DSLAM_HIP(hipGetLastError());
  }
  return DSLAM_OK;
}

// the result block of nq queries to the host; waits for the stream and reports what kernels reported
int read_back(dslam_engine *e, dslam_fern_index *idx, int nq) {
  DSLAM_HIP(hipMemcpyAsync(idx->result_host.get(), idx->result.get(), (size_t)(kResKeys + nq * DSLAM_FERN_MAX_MATCHES) * sizeof(unsigned),
                           hipMemcpyDeviceToHost, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));
  return device_errors(e);
}

void deliver(const dslam_fern_index *idx, int nq, int k, dslam_fern_match *matches_out, int32_t *num_out) {
  const unsigned *res = idx->result_host;
  for (int q = 0; q < nq; q++) {
    const int n = std::min((int)res[kResCounts + q], k);
    for (int j = 0; j < n; j++) {
      const unsigned key = res[kResKeys + q * DSLAM_FERN_MAX_MATCHES + j];
      matches_out[(size_t)q * k + j].id = (int32_t)(key & 0x3fffffu);
      matches_out[(size_t)q * k + j].dissimilarity = (int32_t)(key >> 22);
    }
    num_out[q] = n;
  }
}

// a failure behind the first enqueue waits for the stream before it returns, as dslam_survey_views does
int drained(dslam_engine *e, int rc) {
  if (rc != DSLAM_OK) (void)hipStreamSynchronize(e->stream);
  return rc;
}

}  // namespace

void fern_build_table(const dslam_fern_params &p, int tw, int th, std::vector<int32_t> &table) {
  unsigned long long state = (unsigned long long)p.seed;
  const auto next = [&state]() {
    state += 0x9E3779B97F4A7C15ull;
    unsigned long long z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  const unsigned long long cells = (unsigned long long)tw * th;
  table.resize((size_t)p.num_ferns * 12);
  for (int d = 0; d < p.num_ferns * 4; d++) {
    const int cell = (int)(next() % cells);
    const int channel = p.channels == 2 ? (int)(next() & 1ull) : 0;
    const int threshold = channel == 0 ? p.depth_min_mm + (int)(next() % (unsigned long long)(p.depth_max_mm - p.depth_min_mm + 1))
                                       : (int)(next() % 255ull);
    table[3 * d] = cell; table[3 * d + 1] = channel; table[3 * d + 2] = threshold;
  }
}

int fern_index_allocate(dslam_engine *e, dslam_fern_index *idx) {
  const int decisions = idx->p.num_ferns * 4;
  std::vector<int2> packed(decisions);
  for (int d = 0; d < decisions; d++) packed[d] = make_int2(2 * idx->table[3 * d] + idx->table[3 * d + 1], idx->table[3 * d + 2]);
  DSLAM_TRY(idx->table_dev.alloc(decisions));
  DSLAM_TRY(idx->codes.alloc((size_t)idx->capacity * DSLAM_FERN_CODE_DWORDS));
  DSLAM_TRY(idx->qcode.alloc(DSLAM_FERN_CODE_DWORDS));
  DSLAM_TRY(idx->result.alloc_zeroed(kResWords, e->stream));
  DSLAM_TRY(idx->result_host.alloc(kResWords));
  DSLAM_TRY(idx->query_ids.alloc(DSLAM_FERN_MAX_QUERIES, hipHostMallocMapped));
  memset(idx->query_ids, 0, DSLAM_FERN_MAX_QUERIES * sizeof(int));
  idx->dist_stride = ((size_t)idx->capacity + 63) & ~(size_t)63;
  DSLAM_HIP(hipMemcpyAsync(idx->table_dev.get(), packed.data(), packed.size() * sizeof(int2), hipMemcpyHostToDevice, e->stream));
  DSLAM_HIP(hipStreamSynchronize(e->stream));   // (`packed` goes with this call)
  DSLAM_TRY(ensure_thumbs(e, idx, 1));
  return ensure_rows(e, idx, 1);
}

int fern_encode_view(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, uint32_t *code_out) {
  const auto run = [&]() -> int {
    DSLAM_TRY(enqueue_encode(e, idx, view_images(v), idx->qcode, nullptr));
    DSLAM_HIP(hipMemcpyAsync(idx->result_host.get(), idx->qcode.get(), DSLAM_FERN_CODE_DWORDS * sizeof(unsigned), hipMemcpyDeviceToHost,
                             e->stream));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    return device_errors(e);
  };
  DSLAM_TRY(drained(e, run()));
  memcpy(code_out, idx->result_host, DSLAM_FERN_CODE_DWORDS * sizeof(unsigned));
  return DSLAM_OK;
}

int fern_query_view(dslam_engine *e, dslam_fern_index *idx, const dslam_view *v, int harvest, int first_id, int last_id, int k,
                    dslam_fern_match *matches_out, int32_t *num_out, int32_t *added_out) {
  const bool process = harvest >= 0;
  const int lo = std::min(first_id, idx->count), hi = std::min(last_id, idx->count);
  const auto run = [&]() -> int {
    idx->query_ids[0] = 0;
    DSLAM_TRY(enqueue_encode(e, idx, view_images(v), idx->qcode, process ? idx->result + kResMin : nullptr));
    // dslam_fern_process needs the smallest dissimilarity over all ids, whatever the window
    DSLAM_TRY(enqueue_search(e, idx, idx->qcode, 1, process ? 0 : lo, process ? idx->count : hi, process, lo, hi, k));
    if (process) {
      hipLaunchKernelGGL(k_fern_append, dim3(1), dim3(64), 0, e->stream, idx->codes.get(), idx->qcode.get(), idx->count, idx->capacity,
                         harvest, idx->result.get());
      DSLAM_HIP(hipGetLastError());
    }
    return read_back(e, idx, 1);
  };
  DSLAM_TRY(drained(e, run()));
  deliver(idx, 1, k, matches_out, num_out);
  if (!process) return DSLAM_OK;
  const unsigned *res = idx->result_host;
  *added_out = -1;
  if (res[kResAdded] != kNoKey) {
    *added_out = idx->count;
    idx->count++;
  } else if (res[kResFull]) {
    set_last_error("the fern index is full: the frame's code was not appended");
    return DSLAM_ERR_UNSUPPORTED;
  }
  return DSLAM_OK;
}

int fern_add_from_store(dslam_engine *e, dslam_fern_index *idx, const dslam_frame_store *fs, int first_slot, int num_slots) {
  const FernImages im = {fs->depth.get() + fs->depth_bytes * first_slot, fs->rgba.get() + fs->rgba_bytes * first_slot, fs->depth_bytes,
                         fs->rgba_bytes, num_slots};
  const auto run = [&]() -> int {
    DSLAM_TRY(enqueue_encode(e, idx, im, idx->codes + (size_t)idx->count * DSLAM_FERN_CODE_DWORDS, nullptr));
    DSLAM_HIP(hipStreamSynchronize(e->stream));
    return device_errors(e);
  };
  DSLAM_TRY(drained(e, run()));
  idx->count += num_slots;
  return DSLAM_OK;
}

int fern_query_stored(dslam_engine *e, dslam_fern_index *idx, const int32_t *query_ids, int num_queries, int first_id, int last_id,
                      int k, dslam_fern_match *matches_out, int32_t *num_out) {
  const int lo = std::min(first_id, idx->count), hi = std::min(last_id, idx->count);
  const auto run = [&]() -> int {
    for (int q = 0; q < num_queries; q++) idx->query_ids[q] = query_ids[q];
    DSLAM_TRY(enqueue_search(e, idx, idx->codes, num_queries, lo, hi, false, lo, hi, k));
    return read_back(e, idx, num_queries);
  };
  DSLAM_TRY(drained(e, run()));
  deliver(idx, num_queries, k, matches_out, num_out);
  return DSLAM_OK;
}

}  // namespace dslam
