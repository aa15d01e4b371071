// rc2dgi_capi.cpp -- the C ABI (include/rc2dgi.h): context, uniforms (RC2DGI.cs:408-433), tables, texture I/O,
// timing and the tuning entry points.  The frame itself: rc2dgi_frame.cpp; shards: rc2dgi_group.cpp.
#include "rc2dgi_ctx.h"
#include "rc2dgi_read.h"
#include "rc2dgi_gradients.h"
#include "rc2dgi_shapes.h"
#include "rc2dgi_sprites_xf.h"
#include "rc2dgi_tilemap.h"

namespace {

bool screen_rt(int which) {
  return which == RC2DGI_RT_COLOR || which == RC2DGI_RT_EMISSIVE || which == RC2DGI_RT_JUMP1 ||
         which == RC2DGI_RT_JUMP2 || which == RC2DGI_RT_DIST || which == RC2DGI_RT_TEMP;
}

// The cascade textures stay within the 32768 texels per axis of the screen's: the accessory calls' planners, the
// read buffer (a row of at most 32768 * 16 bytes) and the workgroup map's 16-bit tile fields are written for that
// bound, and nothing wider has been run.  derive_sizes rounds W * renderScale up to a multiple of 2^N, and 32768 is
// one for every N <= 15: the cascade fits exactly when the scaled screen does, whatever the cascade count (so
// _CascadeCount cannot push it over).  Tested before derive_sizes, whose int sizes a large renderScale would wrap.
constexpr float kMaxAxis = 32768.0f;
bool cascade_fits(int W, int H, float rs) { return (float)W * rs <= kMaxAxis && (float)H * rs <= kMaxAxis; }

inline unsigned char to_unorm8(float x) {  // GL readback conversion: clamp, round to nearest even; NaN -> 0 as q8 does
  float v = x > 0.0f ? (x > 1.0f ? 1.0f : x) : 0.0f;  // (a NaN compares false: the rows a strip shard does not hold)
  return (unsigned char)std::nearbyint(v * 255.0f);
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

int rc2dgi_abi_version(void) { return RC2DGI_ABI_VERSION; }

int rc2dgi_create(const rc2dgi_config *cfg, rc2dgi_ctx **out) {
  if (!cfg || !out) return RC2DGI_E_ARG;
  *out = nullptr;
  if (cfg->screen_width <= 0 || cfg->screen_height <= 0 || cfg->screen_width > 32768 ||
      cfg->screen_height > 32768 || cfg->cascade_count < 1 || cfg->cascade_count > 15 ||
      !(cfg->render_scale > 0.0f))
    return RC2DGI_E_ARG;
  for (int r : cfg->reserved)
    if (r != 0) return RC2DGI_E_ARG;
  if (cfg->flags & ~RC2DGI_FLAG_LINUX_MERGE_FALLBACK) return RC2DGI_E_ARG;
  if (cfg->storage != RC2DGI_STORAGE_F32 && cfg->storage != RC2DGI_STORAGE_F16 &&
      cfg->storage != RC2DGI_STORAGE_RGBA8_COMPAT)
    return RC2DGI_E_ARG;
  if (!cascade_fits(cfg->screen_width, cfg->screen_height, cfg->render_scale)) {
    fprintf(stderr, "rc2dgi_create: the cascade resolution exceeds 32768 on an axis\n");
    return RC2DGI_E_ARG;
  }
  rc2dgi_ctx *c = new (std::nothrow) rc2dgi_ctx();
  if (!c) return RC2DGI_E_OOM;
  c->device = cfg->device;
  c->W = cfg->screen_width;
  c->H = cfg->screen_height;
  c->N = cfg->cascade_count;
  c->render_scale = cfg->render_scale;
  c->storage = cfg->storage;
  c->ray_range = cfg->ray_range;
  c->linux_merge = (cfg->flags & RC2DGI_FLAG_LINUX_MERGE_FALLBACK) != 0;
  c->paint_dev.plan = paint_dev_plan(c->W, c->H);
  int rc = RC2DGI_OK;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    fprintf(stderr, "rc2dgi_create: %s\n", hipGetErrorString(e));
    delete c;
    return e == hipErrorOutOfMemory ? RC2DGI_E_OOM : RC2DGI_E_HIP;
  }
  c->stream = c->own_stream;
  for (auto &ev : c->ev) (void)hipEventCreateWithFlags(&ev, timing_event_flags());
  (void)hipEventCreateWithFlags(&c->ev_phase1, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&c->ev_frame, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming);
  for (auto &ev : c->ev_jfa) (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  rc = allocate(c);
  if (rc != RC2DGI_OK) {
    fprintf(stderr, "rc2dgi_create: %s\n", c->err.c_str());
    rc2dgi_destroy(c);
    return rc;
  }
  for (auto &ev : c->ev_level) (void)hipEventCreateWithFlags(&ev, timing_event_flags());
  *out = c;
  return RC2DGI_OK;
}

int rc2dgi_destroy(rc2dgi_ctx *c) {
  if (!c) return RC2DGI_E_ARG;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  drop_comm(c);
  if (c->ev_phase1) (void)hipEventDestroy(c->ev_phase1);
  if (c->ev_frame) (void)hipEventDestroy(c->ev_frame);
  if (c->ev_side) (void)hipEventDestroy(c->ev_side);
  for (auto &ev : c->ev_jfa)
    if (ev) (void)hipEventDestroy(ev);
  free_buffers(c);
  if (c->curves_dev) (void)hipFree(c->curves_dev);  // (the tone curves outlive a reallocation of the textures)
  c->curves_dev = nullptr;
  for (auto &ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : c->ev_level)
    if (ev) (void)hipEventDestroy(ev);
  if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
  for (hipEvent_t ev : {c->ev_fork, c->ev_join})
    if (ev) (void)hipEventDestroy(ev);
  if (c->side_stream) (void)hipStreamDestroy(c->side_stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return RC2DGI_OK;
}

const char *rc2dgi_last_error(rc2dgi_ctx *c) { return c ? c->err.c_str() : "null context"; }

int rc2dgi_set_uniform(rc2dgi_ctx *c, const char *name, const float *v, int n) {
  if (!c || !name || !v) return fail(c, RC2DGI_E_ARG, "null argument");
  std::string s(name);
  auto scalar = [&](float &dst, bool affects_sky) -> int {
    if (n != 1) return fail(c, RC2DGI_E_UNIFORM, s + " takes 1 component");
    dst = v[0];
    if (affects_sky) c->tables_dirty = true;
    return RC2DGI_OK;
  };
  auto vec3 = [&](float *dst) -> int {
    if (n != 3) return fail(c, RC2DGI_E_UNIFORM, s + " takes 3 components");
    for (int k = 0; k < 3; ++k) dst[k] = v[k];
    c->tables_dirty = true;
    return RC2DGI_OK;
  };
  if (s == "_RayRange") return scalar(c->ray_range, false);
  if (s == "_SkyRadiance") return scalar(c->sky_radiance, true);
  if (s == "_SunAngle") return scalar(c->sun_angle, true);
  if (s == "_Reflectivity") return scalar(c->reflectivity, false);
  if (s == "_BlurRadius") return scalar(c->blur_radius, false);
  if (s == "_SkyColor") return vec3(c->sky_color);
  if (s == "_SunColor") return vec3(c->sun_color);
  if (s == "_StepSize" || s == "_Aspect" || s == "_CascadeResolution" || s == "_CascadeLevel" ||
      s == "_Resolution" || s == "_CascadeCount")
    return fail(c, RC2DGI_E_UNIFORM, s + " is derived per pass by rc2dgi_do (or use rc2dgi_set_uniform_i)");
  return fail(c, RC2DGI_E_UNIFORM, "unknown uniform " + s);
}

int rc2dgi_get_uniform(rc2dgi_ctx *c, const char *name, float *v, int n) {
  if (!c || !name || !v) return fail(c, RC2DGI_E_ARG, "null argument");
  std::string s(name);
  const float *src = nullptr;
  int k = 1;
  if (s == "_RayRange") src = &c->ray_range;
  else if (s == "_SkyRadiance") src = &c->sky_radiance;
  else if (s == "_SunAngle") src = &c->sun_angle;
  else if (s == "_Reflectivity") src = &c->reflectivity;
  else if (s == "_BlurRadius") src = &c->blur_radius;
  else if (s == "_SkyColor") { src = c->sky_color; k = 3; }
  else if (s == "_SunColor") { src = c->sun_color; k = 3; }
  else return fail(c, RC2DGI_E_UNIFORM, "unknown uniform " + s);
  if (n != k) return fail(c, RC2DGI_E_UNIFORM, s + " has " + std::to_string(k) + " components");
  for (int q = 0; q < k; ++q) v[q] = src[q];
  return RC2DGI_OK;
}

int rc2dgi_set_uniform_i(rc2dgi_ctx *c, const char *name, int v) {
  if (!c || !name) return fail(c, RC2DGI_E_ARG, "null argument");
  std::string s(name);
  if (s != "_CascadeCount") return fail(c, RC2DGI_E_UNIFORM, "unknown integer uniform " + s);
  if (v < 1 || v > 15) return fail(c, RC2DGI_E_ARG, "_CascadeCount must be in 1..15");
  if (v == c->N) return RC2DGI_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto &ev : c->ev_level)
    if (ev) (void)hipEventDestroy(ev);
  c->ev_level.clear();
  c->N = v;
  // the painted inputs survive the reallocation
  std::vector<float4> col((size_t)c->sd.pitch * c->H), em((size_t)c->sd.pitch * c->H);
  HIPCHK(c, hipMemcpy(col.data(), c->color_in, col.size() * sizeof(float4), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(em.data(), c->emissive, em.size() * sizeof(float4), hipMemcpyDeviceToHost));
  c->sky_override.clear();
  int rc = allocate(c);
  if (rc != RC2DGI_OK) {
    c->broken = true;  // no half-allocated context runs a frame: every later call reports it
    return rc;
  }
  for (auto &ev : c->ev_level) (void)hipEventCreateWithFlags(&ev, timing_event_flags());
  HIPCHK(c, hipMemcpy(c->color_in, col.data(), col.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->emissive, em.data(), em.size() * sizeof(float4), hipMemcpyHostToDevice));
  return RC2DGI_OK;
}

int rc2dgi_upload(rc2dgi_ctx *c, int which, const void *host, int pitch_bytes, int format) {
  if (!c || !host) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are inputs");
  const int W = c->W, H = c->H;
  const int row = format == RC2DGI_FMT_RGBA32F ? W * 16 : (format == RC2DGI_FMT_RGBA8 ? W * 4 : -1);
  if (row < 0) return fail(c, RC2DGI_E_ARG, "bad format");
  if (pitch_bytes == 0) pitch_bytes = row;
  if (pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  if (format == RC2DGI_FMT_RGBA32F) {
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)c->sd.pitch * 16, host, pitch_bytes, (size_t)W * 16, H,
                               hipMemcpyHostToDevice, c->stream));
    if (rgba8(c)) HIPCHK(c, launch_quantize_u8(dst, c->sd.pitch, W, H, c->stream));  // into an RGBA8 texture
  } else {
    std::vector<float4> tmp((size_t)W * H);
    const unsigned char *src = static_cast<const unsigned char *>(host);
    const bool u8 = rgba8(c);
    for (int j = 0; j < H; ++j)
      for (int i = 0; i < W; ++i) {
        const unsigned char *p = src + (size_t)j * pitch_bytes + 4 * (size_t)i;
        tmp[(size_t)j * W + i] =
            u8 ? make_float4((float)p[0] * kInv255h, (float)p[1] * kInv255h, (float)p[2] * kInv255h,
                             (float)p[3] * kInv255h)
               : make_float4((float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, (float)p[3] / 255.0f);
      }
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)c->sd.pitch * 16, tmp.data(), (size_t)W * 16, (size_t)W * 16, H,
                               hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_paint(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const rc2dgi_prim *prims, int n) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are painted");
  if (n < 0 || (n > 0 && !prims)) return fail(c, RC2DGI_E_ARG, "bad primitive list");
  const float lim = 4194304.0f;  // 2^22 pixels
  for (int k = 0; k < n; ++k) {
    const rc2dgi_prim &q = prims[k];
    if (q.kind != RC2DGI_PRIM_RECT && q.kind != RC2DGI_PRIM_CIRCLE)
      return fail(c, RC2DGI_E_ARG, "primitive " + std::to_string(k) + ": unknown kind");
    const float v[4] = {q.x, q.y, q.w, q.kind == RC2DGI_PRIM_RECT ? q.h : 0.0f};
    for (float x : v)
      if (!(std::fabs(x) < lim)) return fail(c, RC2DGI_E_ARG, "primitive " + std::to_string(k) + ": coordinates");
    if (q.kind == RC2DGI_PRIM_RECT && !(std::fabs(q.x + q.w) < lim && std::fabs(q.y + q.h) < lim))
      return fail(c, RC2DGI_E_ARG, "primitive " + std::to_string(k) + ": coordinates");
    if (q.kind == RC2DGI_PRIM_CIRCLE && !(std::fabs(q.x) + std::fabs(q.w) < lim && std::fabs(q.y) + std::fabs(q.w) < lim))
      return fail(c, RC2DGI_E_ARG, "primitive " + std::to_string(k) + ": coordinates");
  }
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  HIPCHK(c, paint_prims(dst, c->W, c->H, c->sd.pitch, rgba8(c), clear_rgba, prims, n, c->paint_buf, c->stream));
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

// rc2dgi_paint_device and rc2dgi_shapes_device: one validation in one order, then `draw` (paint_prims_device or
// shapes_device) on the context's working memory and stream.  Rec is the list's record: its size is checked where the
// call is named.
typedef hipError_t (*PaintListFn)(float4 *, int, int, int, bool, const unsigned char *, const void *, int, const void *,
                                  void *, PaintDevBuffers &, hipStream_t);
extern "C++" template <class Rec, size_t Bytes>
static int paint_list_call(rc2dgi_ctx *c, const char *call, PaintListFn draw, int which,
                           const unsigned char *clear_rgba, const void *list_dev, int n, const void *count_dev,
                           void *status_dev) {
  static_assert(sizeof(Rec) == Bytes && Bytes % 4 == 0, "a record of the list is whole 32-bit words");
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  const std::string name(call);
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are painted");
  if (n < 0 || n > (1 << 20)) return fail(c, RC2DGI_E_ARG, name + ": n is 0 .. 1 << 20");
  if (n > 0 && !list_dev) return fail(c, RC2DGI_E_ARG, name + ": null primitive list");
  for (const void *p : {list_dev, count_dev, static_cast<const void *>(status_dev)})
    if (reinterpret_cast<uintptr_t>(p) % 4 != 0)
      return fail(c, RC2DGI_E_ARG, name + ": the list, the count and the status are aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  HIPCHK(c, draw(dst, c->W, c->H, c->sd.pitch, rgba8(c), clear_rgba, list_dev, n, count_dev, status_dev, c->paint_dev,
                 c->stream));
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_paint_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const void *prims_dev, int n,
                        const void *count_dev, void *status_dev) {
  return paint_list_call<rc2dgi_prim, 24>(c, "paint_device", paint_prims_device, which, clear_rgba, prims_dev, n,
                                          count_dev, status_dev);
}

int rc2dgi_shapes_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const void *shapes_dev, int n,
                         const void *count_dev, void *status_dev) {
  static_assert(offsetof(rc2dgi_shape, v) == 4 && offsetof(rc2dgi_shape, r) == 28, "a shape is eight 32-bit words");
  return paint_list_call<rc2dgi_shape, 32>(c, "shapes_device", shapes_device, which, clear_rgba, shapes_dev, n,
                                           count_dev, status_dev);
}

int rc2dgi_gradients_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const void *grads_dev, int n,
                            const void *count_dev, void *status_dev) {
  static_assert(offsetof(rc2dgi_gradient, v) == 4 && offsetof(rc2dgi_gradient, c) == 28 &&
                    offsetof(rc2dgi_gradient, gain) == 44,
                "a gradient is twelve 32-bit words");
  return paint_list_call<rc2dgi_gradient, 48>(c, "gradients_device", gradients_device, which, clear_rgba, grads_dev, n,
                                              count_dev, status_dev);
}

int rc2dgi_paint_device_limits(const rc2dgi_config *cfg, int *batch_prims, long long *work_bytes) {
  if (!cfg || cfg->screen_width <= 0 || cfg->screen_height <= 0 || cfg->screen_width > 32768 ||
      cfg->screen_height > 32768)
    return RC2DGI_E_ARG;
  const PaintDevPlan plan = paint_dev_plan(cfg->screen_width, cfg->screen_height);
  if (batch_prims) *batch_prims = plan.batch;
  if (work_bytes) *work_bytes = (long long)plan.bytes;
  return RC2DGI_OK;
}

// The atlas checks of the sprite calls and rc2dgi_tilemap_device, in one order and one wording; `a` is the atlas
// with its pitch resolved.
static int atlas_check(rc2dgi_ctx *c, const std::string &name, const rc2dgi_atlas *atlas, SpriteAtlas &a) {
  if (!atlas || !atlas->dev) return fail(c, RC2DGI_E_ARG, name + ": null atlas");
  if (atlas->w < 1 || atlas->h < 1 || atlas->w > 32768 || atlas->h > 32768)
    return fail(c, RC2DGI_E_ARG, name + ": the atlas is 1 .. 32768 pixels on each axis");
  if (atlas->format != RC2DGI_FMT_RGBA8 && atlas->format != RC2DGI_FMT_RGBA16F && atlas->format != RC2DGI_FMT_RGBA32F)
    return fail(c, RC2DGI_E_ARG, name + ": bad atlas format");
  const int pxb = read_pixel_bytes(atlas->format), row = atlas->w * pxb;  // (w <= 32768)
  const int apitch = atlas->pitch_bytes == 0 ? row : atlas->pitch_bytes;
  if (apitch < row || apitch % pxb != 0)
    return fail(c, RC2DGI_E_ARG, name + ": the atlas pitch is at least a row and a multiple of a pixel");
  if (reinterpret_cast<uintptr_t>(atlas->dev) % (uintptr_t)pxb != 0)
    return fail(c, RC2DGI_E_ARG, name + ": the atlas is aligned to a pixel");
  a = SpriteAtlas{static_cast<const unsigned char *>(atlas->dev), atlas->w, atlas->h, (size_t)apitch, atlas->format};
  return RC2DGI_OK;
}

// rc2dgi_sprites_device and rc2dgi_sprites_xf_device: one validation in one order, then `draw` (sprites_device or
// sprites_xf_device) on the context's working memory and stream
typedef hipError_t (*SpriteListFn)(float4 *, int, int, int, bool, const unsigned char *, const SpriteAtlas &,
                                   const void *, int, const void *, void *, PaintDevBuffers &, hipStream_t);
static int sprite_list_call(rc2dgi_ctx *c, const char *call, SpriteListFn draw, int which,
                            const unsigned char *clear_rgba, const rc2dgi_atlas *atlas, const void *sprites_dev, int n,
                            const void *count_dev, void *status_dev) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  const std::string name(call);
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are drawn into");
  if (n < 0 || n > (1 << 20)) return fail(c, RC2DGI_E_ARG, name + ": n is 0 .. 1 << 20");
  SpriteAtlas a{};
  if (const int rc = atlas_check(c, name, atlas, a)) return rc;
  if (n > 0 && !sprites_dev) return fail(c, RC2DGI_E_ARG, name + ": null sprite list");
  for (const void *p : {sprites_dev, count_dev, static_cast<const void *>(status_dev)})
    if (reinterpret_cast<uintptr_t>(p) % 4 != 0)
      return fail(c, RC2DGI_E_ARG, name + ": the list, the count and the status are aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  HIPCHK(c, draw(dst, c->W, c->H, c->sd.pitch, rgba8(c), clear_rgba, a, sprites_dev, n, count_dev, status_dev,
                 c->paint_dev, c->stream));
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_sprites_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                          const void *sprites_dev, int n, const void *count_dev, void *status_dev) {
  static_assert(sizeof(rc2dgi_sprite) == 32, "a sprite is eight 32-bit words");
  return sprite_list_call(c, "sprites_device", sprites_device, which, clear_rgba, atlas, sprites_dev, n, count_dev,
                          status_dev);
}

int rc2dgi_sprites_xf_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                             const void *sprites_dev, int n, const void *count_dev, void *status_dev) {
  static_assert(sizeof(rc2dgi_sprite_xf) == 48 && offsetof(rc2dgi_sprite_xf, px) == 16 &&
                    offsetof(rc2dgi_sprite_xf, r) == 40 && offsetof(rc2dgi_sprite_xf, flags) == 44,
                "a transformed sprite is twelve 32-bit words");
  return sprite_list_call(c, "sprites_xf_device", sprites_xf_device, which, clear_rgba, atlas, sprites_dev, n,
                          count_dev, status_dev);
}

int rc2dgi_tilemap_device(rc2dgi_ctx *c, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                          const rc2dgi_tilemap *map, void *status_dev) {
  static_assert(sizeof(rc2dgi_tilemap) == 56 && offsetof(rc2dgi_tilemap, cols) == 8 &&
                    offsetof(rc2dgi_tilemap, r) == 48 && offsetof(rc2dgi_tilemap, flags) == 52,
                "a tile map is a pointer, ten ints, a tint and the flags");
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  const std::string name("tilemap_device");
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are drawn into");
  SpriteAtlas a{};
  if (const int rc = atlas_check(c, name, atlas, a)) return rc;
  if (!map) return fail(c, RC2DGI_E_ARG, name + ": null map");
  const rc2dgi_tilemap &m = *map;
  auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
  if (m.flags & ~(unsigned)RC2DGI_SPRITE_REPLACE) return fail(c, RC2DGI_E_ARG, name + ": flags is RC2DGI_SPRITE_REPLACE or 0");
  if (!in(m.cols, 0, 32768) || !in(m.rows, 0, 32768)) return fail(c, RC2DGI_E_ARG, name + ": cols and rows are 0 .. 32768");
  if (m.pitch_cells != 0 && !in(m.pitch_cells, m.cols, 1 << 20))
    return fail(c, RC2DGI_E_ARG, name + ": pitch_cells is 0 or cols .. 1 << 20");
  if (!in(m.tile_w, 1, 32768) || !in(m.tile_h, 1, 32768))
    return fail(c, RC2DGI_E_ARG, name + ": tile_w and tile_h are 1 .. 32768");
  if (!in(m.ox, -(1 << 22), 1 << 22) || !in(m.oy, -(1 << 22), 1 << 22))
    return fail(c, RC2DGI_E_ARG, name + ": ox and oy are within 2^22 of zero");
  if (!in(m.set_cols, 1, 32768) || !in(m.margin, 0, 32768) || !in(m.spacing, 0, 32768))
    return fail(c, RC2DGI_E_ARG, name + ": set_cols is 1 .. 32768, margin and spacing are 0 .. 32768");
  if (m.margin + m.tile_w > a.w || m.margin + m.tile_h > a.h)
    return fail(c, RC2DGI_E_ARG, name + ": tile 0 does not fit the atlas");
  if (!m.cells_dev && (long long)m.cols * m.rows > 0) return fail(c, RC2DGI_E_ARG, name + ": null cells");
  for (const void *p : {m.cells_dev, static_cast<const void *>(status_dev)})
    if (reinterpret_cast<uintptr_t>(p) % 4 != 0)
      return fail(c, RC2DGI_E_ARG, name + ": the cells and the status are aligned to 4 bytes");
  TilemapLayer layer{};
  layer.cells = static_cast<const unsigned *>(m.cells_dev);
  layer.g = TilemapGeom{m.cols, m.rows, m.pitch_cells == 0 ? std::max(m.cols, 1) : m.pitch_cells, m.tile_w, m.tile_h,
                        m.ox, m.oy, m.set_cols, m.margin, m.tile_w + m.spacing, m.tile_h + m.spacing,
                        tilemap_max_tile(a.w, m.margin, m.tile_w, m.spacing),
                        tilemap_max_tile(a.h, m.margin, m.tile_h, m.spacing)};
  layer.tint[0] = m.r, layer.tint[1] = m.g, layer.tint[2] = m.b, layer.tint[3] = m.a;
  layer.replace = (m.flags & RC2DGI_SPRITE_REPLACE) != 0;
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  HIPCHK(c, tilemap_device(dst, c->W, c->H, c->sd.pitch, rgba8(c), clear_rgba, a, layer, status_dev, &c->tilemap_cnt,
                           c->stream));
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_upload_device(rc2dgi_ctx *c, int which, const void *dev, int pitch_bytes, int format) {
  if (!c || !dev) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  if (which != RC2DGI_RT_COLOR && which != RC2DGI_RT_EMISSIVE)
    return fail(c, RC2DGI_E_ARG, "only COLOR and EMISSIVE are inputs");
  const int W = c->W, H = c->H;
  const int row = format == RC2DGI_FMT_RGBA32F ? W * 16 : (format == RC2DGI_FMT_RGBA8 ? W * 4 : -1);
  if (row < 0) return fail(c, RC2DGI_E_ARG, "bad format");
  if (pitch_bytes == 0) pitch_bytes = row;
  if (pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  if (format == RC2DGI_FMT_RGBA8) {  // (k_unorm8_to_f32 loads a pixel as one dword)
    if (pitch_bytes % 4 != 0) return fail(c, RC2DGI_E_ARG, "the pitch is a multiple of 4 bytes");
    if (reinterpret_cast<uintptr_t>(dev) % 4 != 0) return fail(c, RC2DGI_E_ARG, "the source is aligned to 4 bytes");
  }
  HIPCHK(c, hipSetDevice(c->device));
  float4 *dst = which == RC2DGI_RT_COLOR ? c->color_in : c->emissive;
  if (format == RC2DGI_FMT_RGBA32F) {
    HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)c->sd.pitch * 16, dev, pitch_bytes, (size_t)W * 16, H,
                               hipMemcpyDeviceToDevice, c->stream));
    if (rgba8(c)) HIPCHK(c, launch_quantize_u8(dst, c->sd.pitch, W, H, c->stream));
  } else {
    HIPCHK(c, launch_unorm8_to_f32(static_cast<const unsigned char *>(dev), pitch_bytes, dst, c->sd.pitch, W, H,
                                   c->stream, rgba8(c)));
  }
  if (which == RC2DGI_RT_COLOR) c->frame_done = false;
  return RC2DGI_OK;
}

int rc2dgi_device_buffer(rc2dgi_ctx *c, int which, void **dev, int *pitch_bytes) {
  if (!c || !dev || !pitch_bytes) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  const int sp = c->sd.pitch, cp = c->cd.pitch;
  if (which == RC2DGI_RT_FINAL_GI && c->gwin && c->frame_done) {  // a shard's strip-sized copy-back texture
    *dev = c->gi_spare;
    *pitch_bytes = cp * (int)gi_bytes(c);
    return RC2DGI_OK;
  }
  if (which == RC2DGI_RT_FINAL_GI) which = c->final_gi == 2 ? RC2DGI_RT_GI2 : RC2DGI_RT_GI1;
  switch (which) {
    case RC2DGI_RT_COLOR: *dev = c->frame_done ? c->color_out : c->color_in; *pitch_bytes = sp * 16; break;
    case RC2DGI_RT_EMISSIVE: *dev = c->emissive; *pitch_bytes = sp * 16; break;
    case RC2DGI_RT_TEMP: *dev = c->temp; *pitch_bytes = sp * 16; break;
    case RC2DGI_RT_JUMP1: *dev = c->jump1; *pitch_bytes = sp * 4; break;
    case RC2DGI_RT_JUMP2: *dev = c->jump2; *pitch_bytes = sp * 4; break;
    case RC2DGI_RT_DIST: *dev = c->dist; *pitch_bytes = sp * 2; break;
    case RC2DGI_RT_GI1: *dev = c->gi1; *pitch_bytes = cp * (int)gi_bytes(c); break;
    case RC2DGI_RT_GI2: *dev = c->gi2; *pitch_bytes = cp * (int)gi_bytes(c); break;
    case RC2DGI_RT_BLUR: *dev = c->blur; *pitch_bytes = cp * 16; break;
    default: return fail(c, RC2DGI_E_ARG, "bad render texture id");
  }
  return RC2DGI_OK;
}

int rc2dgi_download_table(rc2dgi_ctx *c, int which, void *host, int bytes) {
  if (!c || bytes < 0 || (bytes > 0 && !host)) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  const void *src = nullptr;
  size_t n = 0;
  const size_t cells = (size_t)kCminDim * kCminDim;
  bool built = true;  // (what the last frame built: do_phase2's flags; the step boxes are static)
  switch (which) {
    case RC2DGI_TAB_HITC: src = c->hitc; n = cells; built = built && c->built_hitc; break;
    case RC2DGI_TAB_CMIN: src = c->cmin; n = cells * sizeof(CminT); built = built && c->built_cmin; break;
    case RC2DGI_TAB_DCLR: src = c->dclr; n = (size_t)kDirBins * cells; built = built && c->built_dclr; break;
    case RC2DGI_TAB_DBOXES: src = c->dboxes; n = (size_t)kDirBins * kCminDim * sizeof(int4); built = true; break;
    case RC2DGI_TAB_CELLPAL: src = c->cell_pal; n = cells * kCellPalStride * sizeof(float4); built = built && c->built_pal; break;
    case RC2DGI_TAB_MFIELD: src = c->mfield; n = (size_t)c->sd.pitch * c->H * sizeof(unsigned short); built = built && c->built_pal; break;
    default: return fail(c, RC2DGI_E_ARG, "bad table id");
  }
  if (!src || !built) return fail(c, RC2DGI_E_STATE, "table not built by the last frame");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (bytes > 0) HIPCHK(c, hipMemcpy(host, src, std::min(n, (size_t)bytes), hipMemcpyDeviceToHost));
  return (int)std::min(n, (size_t)0x7FFFFFFF);
}

int rc2dgi_sync(rc2dgi_ctx *c) {
  if (!c) return RC2DGI_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return check_chain(c);
}

int rc2dgi_set_stream(rc2dgi_ctx *c, void *s) {
  if (!c) return RC2DGI_E_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->stream = s ? static_cast<hipStream_t>(s) : c->own_stream;
  return RC2DGI_OK;
}

int rc2dgi_set_timing(rc2dgi_ctx *c, int enable) {
  if (!c) return RC2DGI_E_ARG;
  if (enable < 0 || enable > 2) return fail(c, RC2DGI_E_ARG, "timing mode is 0 (off), 1 (passes + levels) or 2 (passes)");
  c->timing = enable;
  c->level_times = false;
  return RC2DGI_OK;
}

int rc2dgi_pass_times(rc2dgi_ctx *c, float *pass_ms, int n_pass, float *level_ms, int n_level) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (!c->timing || !c->have_frame) return fail(c, RC2DGI_E_STATE, "enable timing and run a frame first");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventSynchronize(c->ev[5]));
  float t[P_COUNT];
  for (int p = 0; p < P_TOTAL; ++p) HIPCHK(c, hipEventElapsedTime(&t[p], c->ev[p], c->ev[p + 1]));
  HIPCHK(c, hipEventElapsedTime(&t[P_TOTAL], c->ev[0], c->ev[5]));
  if (pass_ms)
    for (int p = 0; p < n_pass && p < P_COUNT; ++p) pass_ms[p] = t[p];
  if (level_ms && !c->level_times)
    return fail(c, RC2DGI_E_STATE, "per-level times need timing mode 1 for the last frame");
  if (level_ms)
    for (int L = 0; L < n_level && L < c->N; ++L)
      HIPCHK(c, hipEventElapsedTime(&level_ms[L], c->ev_level[L + 1], c->ev_level[L]));
  return RC2DGI_OK;
}

int rc2dgi_query(rc2dgi_ctx *c, int *cw, int *ch, int *jfa_steps, int *final_gi) {
  if (!c) return RC2DGI_E_ARG;
  if (cw) *cw = c->CW;
  if (ch) *ch = c->CH;
  if (jfa_steps) *jfa_steps = c->S;
  if (final_gi) *final_gi = (c->N % 2 == 0) ? 2 : 1;
  return RC2DGI_OK;
}

int rc2dgi_set_direction_table(rc2dgi_ctx *c, int level, const float *cos_sin, int n) {
  if (!c) return RC2DGI_E_ARG;
  if (level < 0 || level >= c->N) return fail(c, RC2DGI_E_ARG, "level out of range");
  if (!cos_sin) {
    c->dir_override[level].clear();
  } else {
    if (n != (4 << (2 * level))) return fail(c, RC2DGI_E_ARG, "direction table must hold 4^(level+1) entries");
    c->dir_override[level].assign(cos_sin, cos_sin + 2 * (size_t)n);
  }
  c->tables_dirty = true;
  return RC2DGI_OK;
}

int rc2dgi_set_sky_table(rc2dgi_ctx *c, const float *rgb, int n) {
  if (!c) return RC2DGI_E_ARG;
  if (!rgb) {
    c->sky_override.clear();
  } else {
    if (n != (4 << (2 * (c->N - 1)))) return fail(c, RC2DGI_E_ARG, "sky table must hold 4^N entries");
    c->sky_override.assign(rgb, rgb + 3 * (size_t)n);
  }
  c->tables_dirty = true;
  return RC2DGI_OK;
}

// The knobs: rc2dgi_tuning.cpp parses the key and validates the value on a copy; the device steps its effect tags ask
// for follow, and the new values are stored once the steps that can fail have passed.
int rc2dgi_set_tuning(rc2dgi_ctx *c, const char *key, int value) {
  if (!c || !key) return fail(c, RC2DGI_E_ARG, "null argument");
  Tuning t = *c;
  std::string err;
  unsigned fx = 0;
  if (!tuning_set(t, c->N, rc_variant_count(), key, value, &err, &fx)) return fail(c, RC2DGI_E_ARG, err);
  // (the side stream is made on first use only: every extra stream takes a share of the process's hardware
  // queues, and the 8 in-process shards of the strips rehearsal ran 0.8 ms slower with one per context)
  if ((fx & kTuneSideStream) && t.side_overlap == 1 && !(c->side_stream && c->ev_fork && c->ev_join)) {
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->side_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
    if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    if (!c->ev_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  }
  if (fx & kTuneChain) {  // no frame in flight while the chain changes
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (fx & kTunePaintPlan) {
    const PaintDevPlan plan = paint_dev_plan(c->W, c->H, t.paint_plan);
    if (plan.mask_bytes() > kPaintDevMaskBytes)
      return fail(c, RC2DGI_E_ARG, "paint_plan: this screen's masks under that plan exceed 40 MiB");
    const PaintDevPlan &old = c->paint_dev.plan;
    if (c->paint_dev.work && (plan.tile_h != old.tile_h || plan.batch != old.batch)) {
      // the masks are laid out by the plan: no painting in flight while the memory goes; the next device call
      // allocates and zeroes it again
      HIPCHK(c, hipSetDevice(c->device));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      c->paint_dev.release();
    }
    c->paint_dev.plan = plan;
  }
  static_cast<Tuning &>(*c) = std::move(t);
  if ((fx & kTuneChain) && !c->rc_chain) free_chain(c);
  if (fx & kTuneAlloff) c->alloff.clear();  // (the no-sample proofs divide as the levels do)
  // (which copies, tables and whether the record texture are held follows these knobs: strip_tables_apply)
  if (!(fx & kTuneSideBuffers) || c->broken) return RC2DGI_OK;
  return prepare_side_buffers(c);
}

int rc2dgi_get_tuning(rc2dgi_ctx *c, const char *key, int *value) {
  if (!c || !key || !value) return fail(c, RC2DGI_E_ARG, "null argument");
  // read-only keys: state of the context, not knobs
  const std::string k(key);
  const struct {
    const char *key;
    int value;
  } state[] = {
      {"rc_variant_count", rc_variant_count()},
      {"strip_tables_active", c->st_last ? 1 : 0},  // the last frame ran with strip tables (strip_tables_apply)
      {"blur_strip_sized", c->gwin ? 1 : 0},  // cascadeBlurRT / the copy-back texture hold the own rows (gi_window_apply)
      {"cascade_banded", c->gband ? 1 : 0},   // giRT1 / giRT2 hold the shard's band of every direction block
      {"rc_fill_levels", c->fill_mask},       // levels the last frame wrote as per-block fills (bits)
      {"paint_tile_h", c->paint_dev.plan.tile_h},  // the device painters' plan in force ("paint_plan")
      {"paint_batch", c->paint_dev.plan.batch},
  };
  for (const auto &s : state)
    if (k == s.key) {
      *value = s.value;
      return RC2DGI_OK;
    }
  if (k == "rc_rdiv_levels") {  // levels whose divisions take the reciprocal form on both non-power-of-two axes (bits)
    int m = 0;
    for (int L = 0; L < c->N && L < 31; ++L)
      if ((c->cd.powW || c->rdiv_x[L]) && (c->cd.powH || c->rdiv_y[L])) m |= 1 << L;
    *value = m;
    return RC2DGI_OK;
  }
  if (k == "rc_chain_timeouts") {  // workgroups of the chain that stopped waiting (synchronises; 0 in a correct run)
    *value = c->chain ? rc_chain_timeouts(c->chain, c->stream) : 0;
    return RC2DGI_OK;
  }
  std::string err;
  if (!tuning_get(*c, c->N, key, value, &err)) return fail(c, RC2DGI_E_ARG, err);
  return RC2DGI_OK;
}

int rc2dgi_set_keep_levels(rc2dgi_ctx *c, int enable) {
  if (!c) return RC2DGI_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_level_bufs(c);
  c->keep_levels = enable != 0;
  if (c->keep_levels) {
    c->level_bufs.assign(c->N, nullptr);
    for (auto &p : c->level_bufs) HIPCHK(c, alloc(&p, (size_t)c->cd.pitch * c->CH * gi_bytes(c)));
  }
  return RC2DGI_OK;
}

int rc2dgi_download_level(rc2dgi_ctx *c, int level, void *host, int pitch_bytes, int format) {
  if (!c || !host) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  if (!c->keep_levels || !c->have_frame) return fail(c, RC2DGI_E_STATE, "enable keep_levels and run a frame first");
  if (level < 0 || level >= c->N) return fail(c, RC2DGI_E_ARG, "level out of range");
  if (format != RC2DGI_FMT_RGBA32F && format != RC2DGI_FMT_RGBA8) return fail(c, RC2DGI_E_ARG, "bad format");
  if (format != RC2DGI_FMT_RGBA32F) return fail(c, RC2DGI_E_UNSUPPORTED, "levels download as RGBA32F");
  const int row = c->CW * 16;
  if (pitch_bytes == 0) pitch_bytes = row;
  if (pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  if (gi_bytes(c) != 16) {
    std::vector<float4> img((size_t)c->CW * c->CH);
    int rc = fetch_gi(c, c->level_bufs[level], img, gi_bytes(c));
    if (rc != RC2DGI_OK) return rc;
    for (int j = 0; j < c->CH; ++j)
      std::memcpy(static_cast<char *>(host) + (size_t)j * pitch_bytes, img.data() + (size_t)j * c->CW, (size_t)row);
    return RC2DGI_OK;
  }
  HIPCHK(c, hipMemcpy2D(host, pitch_bytes, c->level_bufs[level], (size_t)c->cd.pitch * 16, row, c->CH,
                        hipMemcpyDeviceToHost));
  return RC2DGI_OK;
}

int rc2dgi_download(rc2dgi_ctx *c, int which, void *host, int pitch_bytes, int format) {
  if (!c || !host) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  // (a shard on strip-sized blur textures: the final GI is the copy-back texture's own rows)
  const bool win_final = which == RC2DGI_RT_FINAL_GI && c->gwin && c->frame_done;
  if (which == RC2DGI_RT_FINAL_GI) which = (c->N % 2 == 0) ? RC2DGI_RT_GI2 : RC2DGI_RT_GI1;
  if (which < RC2DGI_RT_COLOR || which > RC2DGI_RT_BLUR) return fail(c, RC2DGI_E_ARG, "bad render texture id");
  if (format != RC2DGI_FMT_RGBA32F && format != RC2DGI_FMT_RGBA8) return fail(c, RC2DGI_E_ARG, "bad format");
  const bool scr = screen_rt(which);
  const int w = scr ? c->W : c->CW, h = scr ? c->H : c->CH;
  const int pitch = scr ? c->sd.pitch : c->cd.pitch;
  const int row = format == RC2DGI_FMT_RGBA32F ? w * 16 : w * 4;
  if (pitch_bytes == 0) pitch_bytes = row;
  if (pitch_bytes < row) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = check_chain(c)) return rc;
  std::vector<float4> img((size_t)w * h);
  auto fetch4 = [&](const float4 *src) -> int {
    HIPCHK(c, hipMemcpy2D(img.data(), (size_t)w * 16, src, (size_t)pitch * 16, (size_t)w * 16, h,
                          hipMemcpyDeviceToHost));
    return RC2DGI_OK;
  };
  // tempRT / the merged colorRT: the rows the context holds (a row-strip shard: its own rows; the others read NaN)
  auto fetch_out = [&](const float4 *src) -> int {
    if (c->ow0 > 0 || c->ow1 < h) std::memset(img.data(), 0xFF, img.size() * sizeof(float4));
    HIPCHK(c, hipMemcpy2D(img.data() + (size_t)c->ow0 * w, (size_t)w * 16, src, (size_t)pitch * 16, (size_t)w * 16,
                          c->ow1 - c->ow0, hipMemcpyDeviceToHost));
    return RC2DGI_OK;
  };
  int rc = RC2DGI_OK;
  const bool n1 = c->N == 1;
  const int gw0 = c->gwin ? c->ow0 : 0, gw1 = c->gwin ? c->ow1 : c->CH;  // rows cascadeBlurRT / gi_spare hold
  // a banded giRT1 / giRT2 (gi_buffers): the band rows of the lowest level it received, the other rows NaN
  auto fetch_band = [&](const float4 *src, int b) -> int {
    int L = -1;
    for (int l = c->N - 1; l >= 0; --l)
      if (((c->N - 1 - l) & 1) == b) L = l;
    std::memset(img.data(), 0xFF, img.size() * sizeof(float4));
    if (L < 0) return RC2DGI_OK;
    const int bh = c->CH >> L, b0 = c->gb0[L], bn = c->gbn[L];
    for (int by = 0; by < (1 << L); ++by) {
      const int n1 = std::min(bn, bh - b0);  // band rows b0 .. bh - 1, then 0 .. (the cyclic rest)
      const float4 *row = src + (size_t)by * bn * c->cd.pitch;
      HIPCHK(c, hipMemcpy2D(img.data() + (size_t)(by * bh + b0) * w, (size_t)w * 16, row, (size_t)pitch * 16,
                            (size_t)w * 16, n1, hipMemcpyDeviceToHost));
      if (bn > n1)
        HIPCHK(c, hipMemcpy2D(img.data() + (size_t)(by * bh) * w, (size_t)w * 16, row + (size_t)n1 * c->cd.pitch,
                              (size_t)pitch * 16, (size_t)w * 16, bn - n1, hipMemcpyDeviceToHost));
    }
    return RC2DGI_OK;
  };
  if (win_final) which = -1;
  switch (which) {
    case -1: rc = fetch_gi(c, c->gi_spare, img, gi_bytes(c), gw0, gw1); break;
    case RC2DGI_RT_COLOR: rc = c->frame_done ? fetch_out(c->color_out) : fetch4(c->color_in); break;
    case RC2DGI_RT_EMISSIVE: rc = fetch4(c->emissive); break;
    case RC2DGI_RT_TEMP: rc = fetch_out(c->temp); break;
    case RC2DGI_RT_GI1: rc = c->gband ? fetch_band(c->gi1, 0) : fetch_gi(c, c->gi1, img, gi_bytes(c)); break;
    case RC2DGI_RT_BLUR: rc = fetch_gi(c, c->blur, img, rgba8(c) ? 4 : 16, gw0, gw1); break;  // RGBA8 mode: bytes
    case RC2DGI_RT_GI2:
      if (n1) {  // giRT2 is never drawn with one cascade: ClearAllRTs content
        for (auto &p : img) p = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
      } else {
        rc = c->gband ? fetch_band(c->gi2, 1) : fetch_gi(c, c->gi2, img, gi_bytes(c));
      }
      break;
    case RC2DGI_RT_JUMP1:
    case RC2DGI_RT_JUMP2: {  // packed seed -> the reference's (u, v, 0, 1), (0,0,0,1) = no seed
      std::vector<unsigned> s((size_t)w * h, rgba8(c) ? 0u : 0x80008000u);
      const unsigned *jb = which == RC2DGI_RT_JUMP1 ? c->jump1 : c->jump2;
      if (c->strip) {  // a row-strip shard holds its own rows (window rows m .. m + h - 1)
        int y0, y1;
        strip_rows(c->H, c->rank, c->world, y0, y1);
        HIPCHK(c, hipMemcpy2D(s.data() + (size_t)y0 * w, (size_t)w * 4, jb + (size_t)c->jx.m * pitch,
                              (size_t)pitch * 4, (size_t)w * 4, y1 - y0, hipMemcpyDeviceToHost));
      } else {
        HIPCHK(c, hipMemcpy2D(s.data(), (size_t)w * 4, jb, (size_t)pitch * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost));
      }
      for (size_t k = 0; k < s.size(); ++k) {
        if (rgba8(c)) {  // the unorm8 seed uv (kv << 16 | ku) itself
          img[k] = make_float4((float)(s[k] & 0xFFFFu) * kInv255h, (float)(s[k] >> 16) * kInv255h, 0.0f, 1.0f);
        } else if (s[k] == 0x80008000u) {  // kNoSeed
          img[k] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        } else {
          const int si = (int)(s[k] & 0xFFFFu), sj = (int)(s[k] >> 16);
          img[k] = make_float4(((float)si + 0.5f) / (float)w, ((float)sj + 0.5f) / (float)h, 0.0f, 1.0f);
        }
      }
      break;
    }
    case RC2DGI_RT_DIST: {
      std::vector<unsigned short> d((size_t)w * h);
      HIPCHK(c, hipMemcpy2D(d.data(), (size_t)w * 2, c->dist, (size_t)pitch * 2, (size_t)w * 2, h,
                            hipMemcpyDeviceToHost));
      for (size_t k = 0; k < d.size(); ++k) {  // DistanceField.fs packUNorm16 encoding of q
        const float hi = (float)((d[k] >> 8) & 255u), lo = (float)(d[k] & 255u);
        img[k] = rgba8(c) ? make_float4(hi * kInv255h, lo * kInv255h, 0.0f, 1.0f)  // RGBA8 texel k: k * (1/255)
                          : make_float4(hi / 255.0f, lo / 255.0f, 0.0f, 1.0f);
      }
      break;
    }
    default: return fail(c, RC2DGI_E_ARG, "bad render texture id");
  }
  if (rc != RC2DGI_OK) return rc;
  unsigned char *dst = static_cast<unsigned char *>(host);
  for (int j = 0; j < h; ++j) {
    if (format == RC2DGI_FMT_RGBA32F) {
      std::memcpy(dst + (size_t)j * pitch_bytes, img.data() + (size_t)j * w, (size_t)w * 16);
    } else {
      for (int i = 0; i < w; ++i) {
        const float4 p = img[(size_t)j * w + i];
        unsigned char *o = dst + (size_t)j * pitch_bytes + 4 * (size_t)i;
        o[0] = to_unorm8(p.x);
        o[1] = to_unorm8(p.y);
        o[2] = to_unorm8(p.z);
        o[3] = to_unorm8(p.w);
      }
    }
  }
  return RC2DGI_OK;
}

}  // extern "C"
