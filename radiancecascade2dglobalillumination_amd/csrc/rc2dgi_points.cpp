// rc2dgi_points.cpp -- the point calls of the C ABI (include/rc2dgi.h): rc2dgi_sample and rc2dgi_raycast with their
// _device variants (rc2dgi_query.hip).  A point sample resolves its texture as a view does (rc2dgi_accessory.h).
#include "rc2dgi_accessory.h"

namespace {

static_assert(sizeof(rc2dgi_ray) == 24 && sizeof(rc2dgi_rayhit) == 44, "the query records are 24 and 44 bytes");

// the checks the four query calls share; n == 0 is left to the caller (a successful no-op)
int query_args(rc2dgi_ctx *c, const void *in, int n, const void *out) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (n < 0 || n > kQueryMax) return fail(c, RC2DGI_E_ARG, "n is 0 .. 1 << 24");
  if (n > 0 && (!in || !out)) return fail(c, RC2DGI_E_ARG, "null argument");
  return refuse_shard(c, "query");
}

int ray_scene(rc2dgi_ctx *c, RayScene &s) {
  if (!c->have_frame) return fail(c, RC2DGI_E_STATE, "a ray cast marches the last frame's distRT: run a frame first");
  const float mx = (float)std::max(c->W, c->H);
  s = RayScene{c->dist, c->color_in, c->emissive, c->sd.pitch, c->W, is_pow2(c->W) ? 1 : 0, c->H, is_pow2(c->H) ? 1 : 0,
               (float)c->W / mx, (float)c->H / mx, c->reflectivity};
  return RC2DGI_OK;
}

int sample_enqueue(rc2dgi_ctx *c, const TexSource &t, const void *uv_dev, int n, void *rgba_dev) {
  HIPCHK(c, launch_sample(t, uv_dev, n, rgba_dev, c->stream));
  return RC2DGI_OK;
}

int raycast_enqueue(rc2dgi_ctx *c, const RayScene &s, const void *rays_dev, int n, void *hits_dev) {
  HIPCHK(c, launch_raycast(s, rays_dev, n, hits_dev, c->stream));
  return RC2DGI_OK;
}

}  // namespace

extern "C" {

int rc2dgi_sample_device(rc2dgi_ctx *c, int which, int filter, const void *uv_dev, int n, void *rgba_dev) {
  if (int rc = query_args(c, uv_dev, n, rgba_dev)) return rc;
  TexSource t{};
  if (int rc = resolve_texture(c, which, filter, "sample: ", t)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(uv_dev, 8) || !aligned_to(rgba_dev, 16))
    return fail(c, RC2DGI_E_ARG, "the points are aligned to 8 bytes and the results to 16");
  HIPCHK(c, hipSetDevice(c->device));
  return sample_enqueue(c, t, uv_dev, n, rgba_dev);
}

int rc2dgi_sample(rc2dgi_ctx *c, int which, int filter, const float *uv, int n, float *rgba) {
  if (int rc = query_args(c, uv, n, rgba)) return rc;
  TexSource t{};
  if (int rc = resolve_texture(c, which, filter, "sample: ", t)) return rc;
  if (n == 0) return RC2DGI_OK;
  return host_call(c, uv, (size_t)n * 8, rgba, (size_t)n * 16,
                   [&](void *in, void *out) { return sample_enqueue(c, t, in, n, out); });
}

int rc2dgi_raycast_device(rc2dgi_ctx *c, const void *rays_dev, int n, void *hits_dev) {
  if (int rc = query_args(c, rays_dev, n, hits_dev)) return rc;
  RayScene s{};
  if (int rc = ray_scene(c, s)) return rc;
  if (n == 0) return RC2DGI_OK;
  if (!aligned_to(rays_dev, 4) || !aligned_to(hits_dev, 4))
    return fail(c, RC2DGI_E_ARG, "the rays and the hit records are aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  return raycast_enqueue(c, s, rays_dev, n, hits_dev);
}

int rc2dgi_raycast(rc2dgi_ctx *c, const rc2dgi_ray *rays, int n, rc2dgi_rayhit *hits) {
  if (int rc = query_args(c, rays, n, hits)) return rc;
  RayScene s{};
  if (int rc = ray_scene(c, s)) return rc;
  if (n == 0) return RC2DGI_OK;
  return host_call(c, rays, (size_t)n * sizeof(rc2dgi_ray), hits, (size_t)n * sizeof(rc2dgi_rayhit),
                   [&](void *in, void *out) { return raycast_enqueue(c, s, in, n, out); });
}

}  // extern "C"
