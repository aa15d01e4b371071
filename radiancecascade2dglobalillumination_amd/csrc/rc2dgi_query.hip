// rc2dgi_query.hip -- a frame queried on the device (include/rc2dgi.h, rc2dgi_sample / rc2dgi_raycast).
//
// The read side of RadianceCascades.fs is two operations: a texture fetch with GL NEAREST / LINEAR + REPEAT
// semantics, and SampleRadianceSDF (RadianceCascades.fs:60-92), the 32-step sphere trace over distRT with the
// emissive / albedo hit record.  k_sample and k_raycast run them for a caller's points and rays, so a host gets the
// light at a sprite, the nearest wall or a line of sight without downloading a texture.
//
// k_sample: one lane per point -- one float2 load, texture(T, (u, v)) through the decoder k_present uses
// (rc2dgi_texel.h; the resolved source arrives by value, its fields are scalar), one 16-byte store.  The taps are
// a gather: up to four texels a lane wherever the caller's points lie.
//
// k_raycast: one lane per ray, in the caller's order (the output order; rays are not re-sorted, so a wave runs as
// long as its longest ray).  The source reads a ray as three 8-byte loads and writes a hit as eleven dwords, all at
// the 4-byte alignment the 24- and 44-byte strides give; the compiler joins them into 16 + 8 byte loads and
// 16 + 16 + 12 byte stores, still declared 4-byte aligned, which gfx950's global accesses permit (forcing them
// apart with volatile turned them into system-scope flat accesses, and compiler fences do not stop the
// backend's pairing).  The march is the shader's, operation by operation: the unit is compiled without
// contraction like the pass kernels, so px = ox + (t * dx) * asp.y is three roundings.  No LDS, no scratch.
#include "rc2dgi_query.h"

#include "rc2dgi_device.h"
#include "rc2dgi_texel.h"

namespace rc2dgi {

namespace {

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(256) void k_sample(const TexSource t, const float2 *__restrict__ uv, int n,
                                                float4 *__restrict__ rgba) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= (unsigned)n) return;
  const float2 p = uv[k];
  const float qnan = __uint_as_float(0x7FC00000u);
  float4 r = make_float4(qnan, qnan, qnan, qnan);
  if (finite_f(p.x) && finite_f(p.y)) r = present_sample(t, p.x, p.y);  // (else: no memory read)
  rgba[k] = r;
}

// an 8-byte load of two floats from a 4-byte aligned address
typedef float ray2_t __attribute__((ext_vector_type(2), aligned(4)));

// |x| <= 2^20 and x is a number
__device__ __forceinline__ bool ray_field_ok(float x) { return fabsf(x) <= kRayFieldMax; }

__global__ __launch_bounds__(256) void k_raycast(const RayScene s, const ray2_t *__restrict__ rays, int n,
                                                 int *__restrict__ hits) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= (unsigned)n) return;
  const ray2_t *rp = rays + (size_t)k * 3;
  const ray2_t o = rp[0], d = rp[1], tt = rp[2];
  int status = RC2DGI_RAY_INVALID, steps = 0, ix = -1, iy = -1;
  float t = 0.0f, px = 0.0f, py = 0.0f;
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  // Within the bound nothing below overflows or turns NaN: |t * d| <= (2^20 + 32) * 2^20 < 2^41 (t grows by at
  // most 1 a step, 32 steps), the aspect is at most 1, and |o| <= 2^20, all far inside float range.
  if (ray_field_ok(o.x) && ray_field_ok(o.y) && ray_field_ok(d.x) && ray_field_ok(d.y) && ray_field_ok(tt.x) &&
      ray_field_ok(tt.y)) {
    const Axis ax{s.W, s.powW}, ay{s.H, s.powH};
    status = RC2DGI_RAY_STEPS;
    c = make_float4(0.0f, 0.0f, 0.0f, 1.0f);  // the shader's initial `hit`
    t = tt.x;
    for (int it = 0; it < kRaySteps; ++it) {
      px = o.x + (t * d.x) * s.aspy;  // rayOrigin + t * rayDirection * _Aspect.yx
      py = o.y + (t * d.y) * s.aspx;
      if (t > tt.y) {
        status = RC2DGI_RAY_RANGE;
        break;
      }
      if (px < 0.0f || py < 0.0f || px > 1.0f || py > 1.0f) {
        status = RC2DGI_RAY_EDGE;
        break;
      }
      // 0 <= x < W, 0 <= y < H (wrap_nearest masks / clamps): px == 1.0 reads column 0, the REPEAT fetch
      const int x = wrap_nearest(px, ax), y = wrap_nearest(py, ay);
      const size_t at = (size_t)y * s.pitch + x;
      const float dist = (float)s.dist[at] / 65535.0f;
      ++steps;
      if (dist < 0.001f) {
        const float4 e = s.emissive[at];
        ix = x;
        iy = y;
        if (sqrtf(e.x * e.x + e.y * e.y + e.z * e.z) > 0.0f) {
          status = RC2DGI_RAY_EMISSIVE;
          c = make_float4(e.x, e.y, e.z, 1.0f);
        } else {
          const float4 col = s.color[at];
          status = RC2DGI_RAY_SURFACE;
          c = make_float4(col.x, col.y, col.z, s.reflectivity);
        }
        break;
      }
      t += dist;
    }
  }
  int *h = hits + (size_t)k * 11;
  h[0] = status;
  h[1] = steps;
  h[2] = ix;
  h[3] = iy;
  h[4] = __float_as_int(t);
  h[5] = __float_as_int(px);
  h[6] = __float_as_int(py);
  h[7] = __float_as_int(c.x);
  h[8] = __float_as_int(c.y);
  h[9] = __float_as_int(c.z);
  h[10] = __float_as_int(c.w);
}

}  // namespace

hipError_t launch_sample(const TexSource &t, const void *uv, int n, void *rgba, hipStream_t st) {
  hipLaunchKernelGGL(k_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, static_cast<const float2 *>(uv),
                     n, static_cast<float4 *>(rgba));
  return hipGetLastError();
}

hipError_t launch_raycast(const RayScene &s, const void *rays, int n, void *hits, hipStream_t st) {
  hipLaunchKernelGGL(k_raycast, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s,
                     static_cast<const ray2_t *>(rays), n, static_cast<int *>(hits));
  return hipGetLastError();
}

}  // namespace rc2dgi
