// combine_device.h -- CombineVoxelInformation, shared by the swap-in merge (maintain.hip) and the map merge (merge.hip),
// and its inverse for the map unmerge (unmerge.hip).
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

// The inverse of combine_voxel (dslam_unmerge_maps): take what combine_voxel(src, dst) added out of the resident voxel
// again, the two halves independent as there.  A half whose src weight is 0 idles; a half whose resident weight is below
// the src weight idles too and counts in depth_under / colour_under (the resident voxel does not hold that much).
__device__ __forceinline__ void uncombine_voxel(unsigned slo, unsigned shi, unsigned &dlo, unsigned &dhi, int &depth_under,
                                                int &colour_under) {
  {
    const int W = (int)((dlo >> 16) & 0xffu), ws = (int)((slo >> 16) & 0xffu);
    if (ws != 0) {
      if (W < ws) {
        depth_under++;
      } else if (W == ws) {   // the last observation leaves: the empty depth half (the colour byte of the word stays)
        dlo = (dlo & 0xff000000u) | kEmptyVoxelLo;
      } else {
        const int rem = W - ws;
        float F = (float)W * sdf_to_float((short)(dlo & 0xffffu)) - (float)ws * sdf_to_float((short)(slo & 0xffffu));
        F /= (float)rem;
        F = F < -1.0f ? -1.0f : (F > 1.0f ? 1.0f : F);
        dlo = (dlo & 0xff000000u) | ((unsigned)rem << 16) | (unsigned)(unsigned short)float_to_sdf(F);
      }
    }
  }
  {
    const int Wc = (int)((dhi >> 16) & 0xffu), wcs = (int)((shi >> 16) & 0xffu);
    if (wcs != 0) {
      if (Wc < wcs) {
        colour_under++;
      } else if (Wc == wcs) {
        dlo &= 0x00ffffffu;
        dhi &= 0xff000000u;
      } else {
        const int rem = Wc - wcs;
        const unsigned dc[3] = {dlo >> 24, dhi & 0xffu, (dhi >> 8) & 0xffu};
        const unsigned sc[3] = {slo >> 24, shi & 0xffu, (shi >> 8) & 0xffu};
        unsigned nc[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          float v = ((float)dc[k] / 255.0f) * (float)Wc - ((float)sc[k] / 255.0f) * (float)wcs;
          v /= (float)rem;
          v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
          nc[k] = (unsigned)(unsigned char)(v * 255.0f);
        }
        dlo = (dlo & 0x00ffffffu) | (nc[0] << 24);
        dhi = (dhi & 0xff000000u) | nc[1] | (nc[2] << 8) | ((unsigned)rem << 16);
      }
    }
  }
}

}  // namespace dslam
