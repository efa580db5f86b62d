// combine_device.h -- CombineVoxelInformation, shared by the swap-in merge (maintain.hip) and the map merge (merge.hip).
#pragma once
#include "dslam_device.h"

#pragma clang fp contract(off)

namespace dslam {

// CombineVoxelInformation: merge the host copy (src) into the resident voxel (dst)
__device__ __forceinline__ void combine_voxel(unsigned slo, unsigned shi, unsigned &dlo, unsigned &dhi, int maxW) {
  {
    int newW = (int)((dlo >> 16) & 0xffu);
    const int oldW = (int)((slo >> 16) & 0xffu);
    if (oldW != 0) {
      float newF = sdf_to_float((short)(dlo & 0xffffu));
      const float oldF = sdf_to_float((short)(slo & 0xffffu));
      newF = (float)oldW * oldF + (float)newW * newF;
      newW = oldW + newW;
      newF /= (float)newW;
      newW = newW < maxW ? newW : maxW;
      dlo = (dlo & 0xff000000u) | ((unsigned)newW << 16) | (unsigned)(unsigned short)float_to_sdf(newF);
    }
  }
  {
    const int newW = (int)((dhi >> 16) & 0xffu), oldW = (int)((shi >> 16) & 0xffu);
    if (oldW != 0) {
      const int sumW = oldW + newW;
      const unsigned dc[3] = {dlo >> 24, dhi & 0xffu, (dhi >> 8) & 0xffu};
      const unsigned sc[3] = {slo >> 24, shi & 0xffu, (shi >> 8) & 0xffu};
      unsigned nc[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        float v = (float)dc[k] / 255.0f;
        const float oc = (float)sc[k] / 255.0f;
        v = oc * (float)oldW + v * (float)newW;
        v /= (float)sumW;
        nc[k] = (unsigned)(unsigned char)(v * 255.0f);
      }
      const unsigned w = (unsigned)(sumW < maxW ? sumW : maxW);
      dlo = (dlo & 0x00ffffffu) | (nc[0] << 24);
      dhi = (dhi & 0xff000000u) | nc[1] | (nc[2] << 8) | (w << 16);
    }
  }
}

}  // namespace dslam
