// lightmap.h — the device half of rptgpu_bake_lightmap[_device] (kernels_lightmap.hip, kernels/lightmap.inc): the UV-space
// rasteriser, the per-texel interpolation with its compaction, the scatter and the dilation, on gfx950.  Every launcher
// enqueues on st and returns hipGetLastError() of its launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rptlightmap {

constexpr uint32_t NOBODY = 0xFFFFFFFFu; // the owner map's "no triangle covers this texel"

struct Triangles {
  const double* positions; // [n][3][3]
  const double* normals;   // [n][3][3] or nullptr: Triangle::from_vertices' flat normal
  const double* uvs;       // [n][3][2]
  uint32_t n;
};
// the raw channels of the whole map (nullptr: not named) — row-major, indexed by texel
struct RawOut {
  int32_t* owner;
  double *barycentric, *position, *normal;
};

// owner[0, width * height) = the lowest index of a triangle that covers the texel's centre, NOBODY without one.  large:
// [1 + n] uint32 of scratch (the triangles whose box the second launch strides with the whole grid)
hipError_t owners(hipStream_t st, const Triangles& t, uint32_t width, uint32_t height, uint32_t* owner, uint32_t* large);

// bytes of scratch the scan of a piece of at most `piece` texels needs
hipError_t scan_bytes(uint64_t piece, size_t* bytes);
// incl[i] = the number of owned texels among base .. base + i of the piece (an inclusive scan, in texel order)
hipError_t scan_owned(hipStream_t st, const uint32_t* owner, uint64_t base, uint32_t m, uint32_t* incl, void* tmp, size_t tmp_bytes);

// the texels base .. base + m: the named raw channels (+0.0 and -1 for a texel without an owner), and, with incl (the scan
// above; nullptr: no gather follows), the gather point, the normal and the stream id of the k-th owned texel of the piece at
// index k of points / normals / ids
hipError_t texels(hipStream_t st, const Triangles& t, uint32_t width, uint32_t height, double offset, uint32_t stream_base,
                  const uint32_t* owner, uint64_t base, uint32_t m, const RawOut& raw, const uint32_t* incl, double* points,
                  double* normals, uint32_t* ids);

// out[base + i][0, width) = res[incl[i] - 1][0, width) for an owned texel, +0.0 for every other (width: 3 or 1)
hipError_t scatter(hipStream_t st, const uint32_t* owner, uint64_t base, uint32_t m, const uint32_t* incl, const double* res,
                   uint32_t words, double* out);

// filled[i] = owner[i] != NOBODY over the whole map
hipError_t filled_from_owner(hipStream_t st, const uint32_t* owner, uint64_t n, uint8_t* filled);
// one round over the whole map, from (src, filled_src) into (dst, filled_dst); words: 3 or 1.  filled_dst may be nullptr
// (another channel's round of the same number writes it)
hipError_t dilate(hipStream_t st, uint32_t width, uint32_t height, uint32_t words, const double* src, const uint8_t* filled_src,
                  double* dst, uint8_t* filled_dst);

} // namespace rptlightmap
