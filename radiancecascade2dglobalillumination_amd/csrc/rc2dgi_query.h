// rc2dgi_query.h -- a frame queried on the device (rc2dgi_sample / rc2dgi_raycast and their _device variants,
// include/rc2dgi.h): point samples of any render texture and ray casts over the last frame's distRT, the two reads
// RadianceCascades.fs makes (a texture fetch; SampleRadianceSDF, RadianceCascades.fs:60-92).  See rc2dgi_query.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "rc2dgi_present.h"

namespace rc2dgi {

constexpr int kQueryMax = 1 << 24;            // points / rays a call
constexpr float kRayFieldMax = 1048576.0f;    // 2^20: the largest magnitude of a ray's fields (else INVALID)
constexpr int kRaySteps = 32;                 // RadianceCascades.fs:66

// what the march reads: the last frame's distRT and the painted inputs, as they are now
struct RayScene {
  const unsigned short *dist;  // packUNorm16 q
  const float4 *color;         // the input colorRT (not the merged output)
  const float4 *emissive;
  int pitch;                   // texels a row (the three share it)
  int W, powW, H, powH;
  float aspx, aspy;            // _Aspect = (W, H) / max(W, H)  (RC2DGI.cs:273)
  float reflectivity;
};

// One launch on `st`, one lane per point: rgba[k] = texture(T, uv[k]).  uv: n float2 (8-byte aligned), rgba: n float4
// (16-byte aligned).  n >= 1.
hipError_t launch_sample(const TexSource &t, const void *uv, int n, void *rgba, hipStream_t st);
// One launch on `st`, one lane per ray: n rc2dgi_ray in, n rc2dgi_rayhit out (both 4-byte aligned).  n >= 1.
hipError_t launch_raycast(const RayScene &s, const void *rays, int n, void *hits, hipStream_t st);

}  // namespace rc2dgi
