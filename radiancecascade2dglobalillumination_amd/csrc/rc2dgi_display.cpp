// rc2dgi_display.cpp -- the display frame of the C ABI (include/rc2dgi.h): the reference's display layout
// (RC2DGI.cs:139-163), the views resolved to their stored textures for k_present (rc2dgi_present.hip), and the edge
// tables that tone them (rc2dgi_set_curve / rc2dgi_compose_tone, rc2dgi_tone.hip).  A view's clip geometry is
// rc2dgi_rectplan.cpp's.
#include "rc2dgi_accessory.h"
#include "rc2dgi_rectplan.h"

namespace {

constexpr int kMaxOut = 32768;

unsigned pack_rgba(const unsigned char *p) {
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

// Validate the call and resolve every view to source pointer, pitch, axes, storage kind and filter, as
// rc2dgi_download reads that texture.  Views that miss the window are dropped.
// The tone of every kept view (`tones`: n records, or null for {1.0f, 0}) goes to `tn`, and toned tells whether any
// differs from {1.0f, 0}: where none does the call is rc2dgi_compose's own kernel.
int resolve_views(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h, const unsigned char *clear,
                  const void *dst, int *pitch_bytes, PresentArgs &a, const rc2dgi_tone *tones, ToneArgs &tn,
                  bool &toned) {
  if (!c || !views || !dst) return fail(c, RC2DGI_E_ARG, "null argument");
  RC2DGI_USABLE(c);
  if (int rc = refuse_shard(c, "compose on")) return rc;
  if (n < 1 || n > RC2DGI_MAX_VIEWS) return fail(c, RC2DGI_E_ARG, "1 .. RC2DGI_MAX_VIEWS views");
  if (out_w < 1 || out_h < 1 || out_w > kMaxOut || out_h > kMaxOut)
    return fail(c, RC2DGI_E_ARG, "the window is 1 .. 32768 pixels on each side");
  if (*pitch_bytes == 0) *pitch_bytes = out_w * 4;
  if (*pitch_bytes < out_w * 4) return fail(c, RC2DGI_E_ARG, "pitch smaller than a row");
  if (*pitch_bytes % 4 != 0) return fail(c, RC2DGI_E_ARG, "the pitch is a multiple of 4 bytes");
  static const unsigned char black[4] = {0, 0, 0, 255};
  a.n = 0;
  a.clear = pack_rgba(clear ? clear : black);
  a.out_w = out_w;
  a.out_h = out_h;
  for (int k = 0; k < n; ++k) {
    const rc2dgi_view &q = views[k];
    const std::string tag = "view " + std::to_string(k) + ": ";
    if (q.which < RC2DGI_RT_COLOR || q.which > RC2DGI_RT_FINAL_GI) return fail(c, RC2DGI_E_ARG, tag + "bad render texture id");
    if (q.w < 1 || q.h < 1) return fail(c, RC2DGI_E_ARG, tag + "w and h are at least 1");
    PresentView v{};
    if (int rc = resolve_texture(c, q.which, q.filter, tag, v)) return rc;
    const rc2dgi_tone tone = tones ? tones[k] : rc2dgi_tone{1.0f, 0};
    if (!(tone.exposure >= 0.0f) || std::isinf(tone.exposure))
      return fail(c, RC2DGI_E_ARG, tag + "the exposure is finite and not negative");
    if (tone.curve < 0 || tone.curve > RC2DGI_MAX_CURVES)
      return fail(c, RC2DGI_E_ARG, tag + "the curve is 0 .. RC2DGI_MAX_CURVES");
    if (tone.curve > 0 && c->curve_host[tone.curve - 1].empty())
      return fail(c, RC2DGI_E_STATE, tag + "its curve slot is not set (rc2dgi_set_curve)");
    v.x = q.x;
    v.y = q.y;
    v.w = q.w;
    v.h = q.h;
    v.border = q.a ? pack_rgba(&q.r) : 0u;
    const bool blit = !v.linear && q.w == v.nx && q.h == v.ny && (v.kind == PK_F32 || v.kind == PK_U8);
    ViewClip cl;
    if (!clip_view(q.x, q.y, q.w, q.h, out_w, out_h, q.a ? 1 : 0, blit, cl)) continue;  // wholly outside the window
    v.cx0 = cl.cx0, v.cx1 = cl.cx1, v.cy0 = cl.cy0, v.cy1 = cl.cy1;
    v.fx0 = cl.fx0, v.fx1 = cl.fx1, v.fy0 = cl.fy0, v.fy1 = cl.fy1;
    tn.exposure[a.n] = tone.exposure;
    tn.curve[a.n] = tone.curve;
    if (tone.curve > 0) tn.used |= 1u << (tone.curve - 1);
    if (tone.exposure != 1.0f || tone.curve != 0) toned = true;
    a.v[a.n++] = v;
  }
  return RC2DGI_OK;
}

// q8 as rc2dgi_device.h states it (the host's rintf rounds to nearest even, as v_rndne does)
unsigned q8_host(float x) { return (unsigned)std::rint(std::fmin(std::fmax(x, 0.0f), 1.0f) * 255.0f); }

float bits_float(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// the two kernels of a display frame: k_present where no view is toned
int launch_frame(rc2dgi_ctx *c, const PresentArgs &a, ToneArgs &tn, bool toned, void *dst, int pitch_bytes) {
  if (!toned) {
    HIPCHK(c, launch_present(a, dst, pitch_bytes, c->stream));
    return RC2DGI_OK;
  }
  tn.tables = c->curves_dev;  // (a named slot is set, so the tables exist)
  HIPCHK(c, launch_present_tone(a, tn, dst, pitch_bytes, c->stream));
  return RC2DGI_OK;
}

int compose_device(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                   const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  PresentArgs a;
  ToneArgs tn{};
  bool toned = false;
  if (int rc = resolve_views(c, views, n, out_w, out_h, clear_rgba, dev, &pitch_bytes, a, tones, tn, toned)) return rc;
  if (!aligned_to(dev, 4)) return fail(c, RC2DGI_E_ARG, "the destination is aligned to 4 bytes");
  HIPCHK(c, hipSetDevice(c->device));
  return launch_frame(c, a, tn, toned, dev, pitch_bytes);
}

int compose_host(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                 const unsigned char *clear_rgba, void *host, int pitch_bytes) {
  PresentArgs a;
  ToneArgs tn{};
  bool toned = false;
  if (int rc = resolve_views(c, views, n, out_w, out_h, clear_rgba, host, &pitch_bytes, a, tones, tn, toned)) return rc;
  if (int rc = host_begin(c)) return rc;
  const size_t dpitch = (size_t)round_up(out_w, 4) * 4;  // 16-byte rows: vector stores
  if (int rc = grow_buffer(c, c->present_buf, c->present_cap, dpitch * (size_t)out_h)) return rc;
  if (int rc = launch_frame(c, a, tn, toned, c->present_buf, (int)dpitch)) return rc;
  HIPCHK(c, hipMemcpy2DAsync(host, (size_t)pitch_bytes, c->present_buf, dpitch, (size_t)out_w * 4, (size_t)out_h,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return RC2DGI_OK;
}

}  // namespace

extern "C" {

int rc2dgi_display_layout(const rc2dgi_config *cfg, rc2dgi_view *views, int max_views) {
  if (!cfg || max_views < 0 || (max_views > 0 && !views)) return RC2DGI_E_ARG;
  const int W = cfg->screen_width, H = cfg->screen_height;
  // DrawTexturePro(colorRT.Texture, ..) over the window, then DrawDebugRT per thumbnail (RC2DGI.cs:139-163, 435-448)
  static const int thumbs[7] = {RC2DGI_RT_COLOR, RC2DGI_RT_EMISSIVE, RC2DGI_RT_JUMP2, RC2DGI_RT_DIST,
                                RC2DGI_RT_GI1,   RC2DGI_RT_GI2,      RC2DGI_RT_TEMP};
  for (int k = 0; k < 8 && k < max_views; ++k) {
    rc2dgi_view v{};
    if (k == 0) {
      v = rc2dgi_view{RC2DGI_RT_COLOR, 0, 0, W, H, RC2DGI_FILTER_RT, 0, 0, 0, 0};
    } else {
      const int t = k - 1;
      v = rc2dgi_view{thumbs[t], W - 110, 10 * (t + 1) + 100 * t, 100, 100, RC2DGI_FILTER_RT, 230, 41, 55, 255};
    }
    views[k] = v;
  }
  return 8;
}

int rc2dgi_compose_device(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h,
                          const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  return compose_device(c, views, nullptr, n, out_w, out_h, clear_rgba, dev, pitch_bytes);
}

int rc2dgi_compose(rc2dgi_ctx *c, const rc2dgi_view *views, int n, int out_w, int out_h, const unsigned char *clear_rgba,
                   void *host, int pitch_bytes) {
  return compose_host(c, views, nullptr, n, out_w, out_h, clear_rgba, host, pitch_bytes);
}

// ---- edge tables, toned views (rc2dgi_tone.hip)
int rc2dgi_check_edges(const float *edges, int m) {
  if (!edges || m < 1) return RC2DGI_E_ARG;
  for (int i = 0; i < m; ++i)
    if (std::isnan(edges[i]) || (i + 1 < m && edges[i] > edges[i + 1])) return RC2DGI_E_ARG;
  return RC2DGI_OK;
}

int rc2dgi_curve_q8(float *edges255) {
  if (!edges255) return RC2DGI_E_ARG;
  for (unsigned k = 1; k <= 255u; ++k) {
    // the smallest bit pattern in [0, bits(1.0f)] whose float has q8 >= k: q8 is monotone there, q8(1.0f) = 255
    uint32_t lo = 0u, hi = 0x3F800000u;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (q8_host(bits_float(mid)) >= k) hi = mid;
      else lo = mid + 1;
    }
    edges255[k - 1] = bits_float(lo);
  }
  return RC2DGI_OK;
}

int rc2dgi_set_curve(rc2dgi_ctx *c, int slot, const float *edges255) {
  if (!c) return RC2DGI_E_ARG;
  RC2DGI_USABLE(c);
  if (slot < 1 || slot > RC2DGI_MAX_CURVES) return fail(c, RC2DGI_E_ARG, "set_curve: the slot is 1 .. RC2DGI_MAX_CURVES");
  if (!edges255) {
    c->curve_host[slot - 1].clear();  // (the device table stays: a compose enqueued earlier still reads it)
    return RC2DGI_OK;
  }
  if (rc2dgi_check_edges(edges255, RC2DGI_CURVE_EDGES) != RC2DGI_OK)
    return fail(c, RC2DGI_E_ARG, "set_curve: 255 ascending edges, none a NaN (rc2dgi_check_edges)");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->curves_dev) HIPCHK(c, alloc(&c->curves_dev, (size_t)RC2DGI_MAX_CURVES * kCurveWords * sizeof(float)));
  std::vector<float> copy(edges255, edges255 + RC2DGI_CURVE_EDGES);
  TableChunk ch;
  tree_layout(copy.data(), RC2DGI_CURVE_EDGES, kCurveLevels, std::numeric_limits<float>::infinity(), ch.v);
  HIPCHK(c, launch_store_table(ch, kCurveWords, c->curves_dev + (size_t)(slot - 1) * kCurveWords, nullptr, 0, c->stream));
  c->curve_host[slot - 1].swap(copy);
  return RC2DGI_OK;
}

int rc2dgi_compose_tone_device(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w,
                               int out_h, const unsigned char *clear_rgba, void *dev, int pitch_bytes) {
  return compose_device(c, views, tones, n, out_w, out_h, clear_rgba, dev, pitch_bytes);
}

int rc2dgi_compose_tone(rc2dgi_ctx *c, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                        const unsigned char *clear_rgba, void *host, int pitch_bytes) {
  return compose_host(c, views, tones, n, out_w, out_h, clear_rgba, host, pitch_bytes);
}

}  // extern "C"
