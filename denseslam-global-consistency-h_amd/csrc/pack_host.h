// pack_host.h -- the host half of the packed-map law (include/dslam_fusion.h states the layout): the
// two layout functions of (n, f) and what makes 64 bytes the header of a packed map.  Plain C++, no device, no HIP call --
// dslam_pack_layout and dslam_pack_header_read (capi.hip) are these two functions behind the ABI's argument checks.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/dslam_fusion.h"

namespace dslam {

constexpr int64_t kPackHeaderBytes = 64, kPackRecordBytes = 16, kPackBlockBytes = 4096;
static_assert(sizeof(dslam_pack_info) == kPackHeaderBytes, "the header of a packed map is 64 bytes");

// n, f >= 0 (checked by the caller).  64-bit throughout: 16 n alone passes 2^31 from n = 2^27 on.
inline void pack_layout(int32_t n, int32_t f, int64_t *blocks_offset, int64_t *total_bytes) {
  const int64_t end = kPackHeaderBytes + kPackRecordBytes * (int64_t)n + 4 * (int64_t)f;
  *blocks_offset = (end + kPackBlockBytes - 1) / kPackBlockBytes * kPackBlockBytes;
  *total_bytes = *blocks_offset + kPackBlockBytes * (int64_t)n;
}

// magic, version, the reserved word, counts that can be counts, and the two layout identities
inline bool pack_header_valid(const dslam_pack_info &h) {
  if (memcmp(h.magic, "DSPK", 4) != 0 || h.version != 1u || h.reserved != 0u) return false;
  if (h.num_buckets < 0 || h.num_excess < 0 || h.blocks < 0 || h.free_excess < 0 || h.free_excess > h.num_excess) return false;
  int64_t off, total;
  pack_layout(h.blocks, h.free_excess, &off, &total);
  return h.blocks_offset == off && h.total_bytes == total;
}

}  // namespace dslam
