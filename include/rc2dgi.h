/*
 * rc2dgi.h -- C ABI of librc2dgi.so, the MI355X-native DoRC2DGI() pass chain.
 *
 * Drop-in boundary for the reference's per-frame GI path:
 *   DoRC2DGI()           RC2DGI.cs:267-406   -> rc2dgi_do()
 *   SetGIShaderValues()  RC2DGI.cs:408-433   -> rc2dgi_set_uniform() / rc2dgi_set_uniform_i()
 *   RT set + knobs       RC2DGI.cs:28-41, 66-98 -> rc2dgi_config + rc2dgi_create()
 *   ClearAllRTs()        RC2DGI.cs:450-483   -> folded into rc2dgi_do() (every target the
 *                                               frame reads is rewritten before it is read)
 *   painted colorRT/emissiveRT (RenderScene RC2DGI.cs:224-264, RedrawSceneToRTs
 *                       RC2DGI.cs:528-545)  -> rc2dgi_upload()
 *   debug thumbnails / final blit (RC2DGI.cs:135-163, 435-448) -> rc2dgi_compose() (the window composed on the
 *                                               device); rc2dgi_download() (one texture to the host, a debug path)
 *
 * Conventions:
 *   - plain C, blittable arguments (P/Invoke int/float/IntPtr), UTF-8 uniform names;
 *   - every entry point returns 0 (RC2DGI_OK) or a negative rc2dgi_status; nothing
 *     aborts or throws across the ABI; rc2dgi_last_error() explains the last failure;
 *   - the context owns every device buffer; host buffers are caller-owned and only
 *     touched during the call (upload/download are synchronous w.r.t. the host pointer);
 *   - images are RGBA, rows in GL texture order (row 0 = bottom), the memory layout of
 *     rlReadTexturePixels / UpdateTexture for a render texture;
 *   - one context per thread at a time (the reference drives one GL context from its
 *     main thread); independent contexts may run concurrently on different streams or
 *     devices (batch / replica mode);
 *   - the ping-pong identities of the reference are preserved: jumpRT1 holds the
 *     ScreenUV seeds and every other JFA step; giRT1 receives level N-1; the final GI
 *     texture is giRT2 when N is even and giRT1 when N is odd (RC2DGI.cs:365).
 *
 * Storage: f32 semantics (RGBA32F render textures, the reference's own commented intent,
 * RC2DGI.cs:100-107).  RC2DGI_STORAGE_F16 keeps that but stores giRT1 / giRT2 as RGBA16F,
 * the format RC2DGI.cs:105-106 names (stores round toward zero as the GL reference
 * implementation does; downloads convert exactly).  RC2DGI_STORAGE_RGBA8_COMPAT is the literal
 * app: every render texture RGBA8 (LoadRenderTexture's default, RC2DGI.cs:79-98) with the GL
 * reference implementation's unorm8 arithmetic -- a texel k reads as k * (1/255), every pass
 * output is blended in 8 bits, LINEAR fetches filter in 8.8 fixed point, the JFA seeds are
 * quantized uv (an occluder whose u or v quantizes to 0 is no seed).  Float downloads return
 * the values the shaders read (k * (1/255)); RGBA8 downloads the texels.  Float uploads are
 * quantized as glTexSubImage into an RGBA8 texture does.
 */
#ifndef RC2DGI_H
#define RC2DGI_H

#ifdef __cplusplus
extern "C" {
#endif

#define RC2DGI_ABI_VERSION 5  /* 2: row-strip sharding entry points; 3: JumpFlood exchange planner;
                                 4: rc2dgi_config.flags (Linux merge fallback); 5: RC2DGI_E_DEVICE.
                                 rc2dgi_display_layout / rc2dgi_compose / rc2dgi_compose_device only add exports and leave
                                 the version at 5: a host detects them by symbol lookup */

typedef struct rc2dgi_ctx rc2dgi_ctx;

typedef enum rc2dgi_status {
  RC2DGI_OK = 0,
  RC2DGI_E_ARG = -1,          /* bad argument (null pointer, size, enum value) */
  RC2DGI_E_UNIFORM = -2,      /* unknown or read-only uniform name / wrong component count */
  RC2DGI_E_HIP = -3,          /* HIP runtime error (message in rc2dgi_last_error) */
  RC2DGI_E_OOM = -4,          /* device allocation failed */
  RC2DGI_E_UNSUPPORTED = -5,  /* valid request this build does not implement */
  RC2DGI_E_STATE = -6,        /* call not valid in the current state */
  RC2DGI_E_DEVICE = -7        /* a device-side check failed: an enqueued frame's results are wrong (the cascade
                                 chain's wait timed out; reported by the next rc2dgi_sync / _download /
                                 _download_level / _compose / _reduce / _compose_tone / _histogram / _read / _do /
                                 _do_phase) */
} rc2dgi_status;

typedef enum rc2dgi_storage {
  RC2DGI_STORAGE_F32 = 0,
  RC2DGI_STORAGE_RGBA8_COMPAT = 1,
  RC2DGI_STORAGE_F16 = 2
} rc2dgi_storage;

/* render textures of the reference (RC2DGI.cs:19-25) */
typedef enum rc2dgi_rt {
  RC2DGI_RT_COLOR = 0,     /* colorRT: painted scene in, merged result out      (W x H) */
  RC2DGI_RT_EMISSIVE = 1,  /* emissiveRT                                        (W x H) */
  RC2DGI_RT_JUMP1 = 2,     /* jumpRT1                                           (W x H) */
  RC2DGI_RT_JUMP2 = 3,     /* jumpRT2                                           (W x H) */
  RC2DGI_RT_DIST = 4,      /* distRT (16-bit distance packed into R,G)          (W x H) */
  RC2DGI_RT_GI1 = 5,       /* giRT1                                             (CW x CH) */
  RC2DGI_RT_GI2 = 6,       /* giRT2                                             (CW x CH) */
  RC2DGI_RT_TEMP = 7,      /* tempRT                                            (W x H) */
  RC2DGI_RT_BLUR = 8,      /* cascadeBlurRT                                     (CW x CH) */
  RC2DGI_RT_FINAL_GI = 9   /* alias of giRT1 / giRT2 per RC2DGI.cs:365          (CW x CH) */
} rc2dgi_rt;

/* rc2dgi_config.flags */
typedef enum rc2dgi_flag {
  /* The literal app on a case-sensitive filesystem: LoadShader(null,
   * "shaders/Merge.fs") (RC2DGI.cs:62) finds no such file (it is merge.fs on disk), raylib substitutes
   * its default shader, and the merge pass (RC2DGI.cs:389-397) draws colorRT into tempRT unchanged:
   * colorRT gets no GI added.  finalGI and every other render texture are unaffected. */
  RC2DGI_FLAG_LINUX_MERGE_FALLBACK = 1
} rc2dgi_flag;

typedef enum rc2dgi_format {
  RC2DGI_FMT_RGBA8 = 0,    /* 4 x uint8, unorm (k/255) */
  RC2DGI_FMT_RGBA32F = 1,  /* 4 x float32 */
  RC2DGI_FMT_RGBA16F = 2   /* 4 x IEEE binary16; accepted by rc2dgi_read / rc2dgi_read_device and rc2dgi_write /
                              rc2dgi_write_device only: rc2dgi_upload, rc2dgi_upload_device, rc2dgi_download and
                              rc2dgi_download_level know the two formats above and refuse this one with RC2DGI_E_ARG */
} rc2dgi_format;

typedef struct rc2dgi_config {
  int screen_width;        /* screenWidth  (RC2DGI.cs:7), 1..32768.  Verified against the CPU oracle, bit for bit: an axis
                              up to 32768 on screens a few texels thin (32768 x 8, 8 x 32768, 16 x 32768, 20000 x 12 ...),
                              squares up to 2048^2 over the whole frame, 4096^2 pass by pass; larger squares are admitted
                              and not verified against it */
  int screen_height;       /* screenHeight (RC2DGI.cs:8), 1..32768 */
  int cascade_count;       /* cascadeCount (RC2DGI.cs:66), 1..15.  Verified: 1..12.  13, 14 and 15 are admitted and NOT
                              verified: they need cascades of at least 8192^2, 16384^2, 32768^2 and tables of 4^N entries
                              (N = 15: 8 GiB of directions, 16 GiB of sky), and from N = 13 on (float)((1 << 2N) - 1), the
                              denominator of the ray intervals, is no longer exact in fp32 */
  float render_scale;      /* renderScale  (RC2DGI.cs:67), > 0, with (float)screen_width * render_scale and
                              (float)screen_height * render_scale <= 32768: the cascade textures (that size rounded up
                              to a multiple of 2^cascade_count) hold at most 32768 texels per axis, whatever the cascade
                              count.  Anything larger is RC2DGI_E_ARG from rc2dgi_create */
  float ray_range;         /* rayRange     (RC2DGI.cs:68) -> _RayRange */
  int storage;             /* rc2dgi_storage */
  int device;              /* HIP device ordinal */
  int flags;               /* rc2dgi_flag bits, 0 = the Windows behaviour (merge.fs) */
  int reserved[4];         /* must be zero */
} rc2dgi_config;

/* ---- lifetime (RC2DGI.cs:57-109) */
int rc2dgi_create(const rc2dgi_config *cfg, rc2dgi_ctx **out);
int rc2dgi_destroy(rc2dgi_ctx *ctx);

/* ---- uniforms (SetGIShaderValues RC2DGI.cs:408-433, Blur RC2DGI.cs:373-374).
 * Accepted names (reference spelling): _RayRange(1) _SkyRadiance(1) _SkyColor(3)
 * _SunColor(3) _SunAngle(1) _Reflectivity(1) _BlurRadius(1).  The per-pass uniforms the
 * reference derives itself (_StepSize _Aspect _CascadeResolution _CascadeLevel _Resolution)
 * are computed inside rc2dgi_do() and are rejected here with RC2DGI_E_UNIFORM. */
int rc2dgi_set_uniform(rc2dgi_ctx *ctx, const char *name, const float *v, int n);
/* _CascadeCount (reallocates the cascade textures, like re-running RC2DGI.cs:66-98) */
int rc2dgi_set_uniform_i(rc2dgi_ctx *ctx, const char *name, int v);
int rc2dgi_get_uniform(rc2dgi_ctx *ctx, const char *name, float *v, int n);

/* ---- inputs: the painted colorRT / emissiveRT (W x H).  Host source: synchronous copy.
 * Device source (a HIP device pointer on the context's device): enqueued on the context
 * stream, the caller keeps the source alive until rc2dgi_sync().
 * pitch_bytes == 0 means a tight row (W * 4 or W * 16 bytes); bytes of a row past that are not read.
 * Errors: RC2DGI_E_ARG for a null context or source, a `which` other than COLOR / EMISSIVE, a bad format, a pitch
 * smaller than a row and, for rc2dgi_upload_device with RC2DGI_FMT_RGBA8, a device source not aligned to 4 bytes or a
 * pitch not a multiple of 4 (the kernel loads a pixel as one dword). */
int rc2dgi_upload(rc2dgi_ctx *ctx, int which, const void *host, int pitch_bytes, int format);
int rc2dgi_upload_device(rc2dgi_ctx *ctx, int which, const void *dev, int pitch_bytes, int format);

/* ---- one DoRC2DGI() frame: enqueues every pass on the context stream and returns. */
int rc2dgi_do(rc2dgi_ctx *ctx);
int rc2dgi_sync(rc2dgi_ctx *ctx);

/* ---- outputs: any render texture, in the reference's RGBA encoding (synchronous).  RC2DGI_FMT_RGBA8 converts as
 * q8 does: rint(clamp(x, 0, 1) * 255), NaN -> 0.  pitch_bytes == 0 means a tight row; bytes of a row past the
 * texture's own are not written. */
int rc2dgi_download(rc2dgi_ctx *ctx, int which, void *host, int pitch_bytes, int format);

/* ---- the display frame, composed on the device (the display half of the reference's main loop, RC2DGI.cs:135-165,
 * 435-448: the final blit of colorRT and the seven debug thumbnails).  One kernel reads the render textures in their
 * stored formats and writes one RGBA8 image of the window, 4 bytes a pixel, to the host (rc2dgi_compose) or into a
 * device buffer (rc2dgi_compose_device).
 *   Output   RGBA8, out_w x out_h, row 0 = the TOP of the window (rc2dgi_download returns GL row order, the other
 *            way up).  pitch_bytes == 0 means out_w * 4; bytes of a row between out_w * 4 and pitch_bytes are not
 *            written.
 *   Clear    every pixel starts as clear_rgba; NULL = (0, 0, 0, 255), ClearBackground(Color.Black).
 *   Draws    the views are drawn in array order, each one its texture and then its border.  Every draw blends into
 *            the 8-bit framebuffer with the blend of the RGBA8 passes, in every storage mode (the window is RGBA8
 *            whatever the render textures are): a8 = q8(src.a) and per channel, alpha included,
 *            min(255, mul8(q8(src_c), a8) + mul8(dst_c, 255 - a8)), q8(x) = rint(clamp(x, 0, 1) * 255),
 *            mul8(x, y) = (x * y * 257 + 32768) >> 16.
 *   Sampling for a window pixel (px, py) inside the view, i = px - x and j = h - 1 - (py - y) (the flip is the
 *            reference's negative source height); u = ((float)i + 0.5f) / (float)w, v = ((float)j + 0.5f) / (float)h.
 *            POINT takes the texel NEAREST + REPEAT names; LINEAR the four REPEAT-wrapped taps and weights of GL's
 *            LINEAR filter, lerped as the texture's storage does: fma lerps on floats (f32; f16 after the exact
 *            unpack), 8.8 fixed point on the bytes (rgba8).
 *   Texels   a texel's value is what rc2dgi_download returns for that texture as floats: JUMP1 / JUMP2 decoded to
 *            (u, v, 0, 1) or no seed (0, 0, 0, 1), DIST to its hi / lo bytes, COLOR the input before the first frame
 *            and the merged output after, GI2 (0, 0, 0, 1) with one cascade, FINAL_GI the alias of GI1 / GI2.
 *   Border   the pixels of the rectangle with px == x, px == x + w - 1, py == y or py == y + h - 1, blended with the
 *            border colour's bytes as the 8-bit source (a == 0: no border).
 * Limits: a 1:1 view is exactly the reference's blit.  For scaled views the texcoord form above is this library's
 * statement (not probed against a GL implementation); the border is a one-pixel frame, not raylib's GL line
 * rasterisation; text and the GUI are the caller's.
 * Errors: RC2DGI_E_ARG for a null context, view list or destination, n outside 1 .. RC2DGI_MAX_VIEWS, w or h below 1,
 * out_w or out_h outside 1 .. 32768, a pitch smaller than a row or not a multiple of 4, a device destination not
 * aligned to 4 bytes, a bad `which` or `filter`; RC2DGI_E_UNSUPPORTED for RC2DGI_FILTER_LINEAR on a texture other
 * than GI1 / GI2 / BLUR / FINAL_GI and for any call on a row-strip shard (world > 1: its textures hold windows and
 * bands). */
enum { RC2DGI_FILTER_RT = 0,     /* the filter the reference sets on that texture (RC2DGI.cs:89-98):
                                    LINEAR for GI1 / GI2 / BLUR / FINAL_GI, POINT for the rest */
       RC2DGI_FILTER_POINT = 1, RC2DGI_FILTER_LINEAR = 2 };
#define RC2DGI_MAX_VIEWS 16

typedef struct rc2dgi_view {
  int which;                 /* rc2dgi_rt, RC2DGI_RT_FINAL_GI allowed */
  int x, y, w, h;            /* destination rectangle in window pixels, y down; w, h >= 1; may hang over the
                                window on any side (clipped) */
  int filter;                /* RC2DGI_FILTER_* */
  unsigned char r, g, b, a;  /* border colour; a == 0: no border */
} rc2dgi_view;               /* 28 bytes, blittable */

/* host-only, no device: the reference's display (RC2DGI.cs:139-163) for this config -- view 0 is COLOR at
 * (0, 0, W, H) without a border, then the thumbnails COLOR, EMISSIVE, JUMP2, DIST, GI1, GI2, TEMP, thumbnail k at
 * (W - 110, 10 * (k + 1) + 100 * k, 100, 100) with RC2DGI_FILTER_RT and raylib's Red (230, 41, 55, 255) as border.
 * Writes up to max_views views; returns 8. */
int rc2dgi_display_layout(const rc2dgi_config *cfg, rc2dgi_view *views, int max_views);
/* synchronous w.r.t. `host`: synchronises the context stream (a cascade chain timeout returns RC2DGI_E_DEVICE, as
 * rc2dgi_download does), composes into a context-owned device buffer and copies out_h rows of out_w * 4 bytes */
int rc2dgi_compose(rc2dgi_ctx *ctx, const rc2dgi_view *views, int n, int out_w, int out_h,
                   const unsigned char *clear_rgba, void *host, int pitch_bytes);
/* enqueues the kernel on the context stream, after whatever frame is in flight, and returns; `dev` is a device
 * pointer on the context's device that the caller keeps alive until rc2dgi_sync() */
int rc2dgi_compose_device(rc2dgi_ctx *ctx, const rc2dgi_view *views, int n, int out_w, int out_h,
                          const unsigned char *clear_rgba, void *dev, int pitch_bytes);

/* ---- queries: a few values of the frame without downloading a texture.  The two reads RadianceCascades.fs makes --
 * a texture fetch and SampleRadianceSDF -- for a caller's points and rays, one kernel a call.  (The light arriving at a
 * sprite: a sample of FINAL_GI; the nearest wall: a sample of JUMP2 / DIST; a line of sight, what lies under the
 * cursor: a ray cast.)
 *
 * Point samples: rgba[k] = texture(T, (u, v)[k]) for n points, uv = n x 2 floats, rgba = n x 4 floats.
 *   which    any rc2dgi_rt, RC2DGI_RT_FINAL_GI included; filter RC2DGI_FILTER_RT / _POINT / _LINEAR as for a view.
 *   (u, v)   GL texture coordinates, v up, row 0 at the bottom: the coordinates the shaders use.  A host with y-down
 *            pixels passes ((x + 0.5f) / W, 1 - (y + 0.5f) / H) for the centre of pixel (x, y) of a W x H texture.
 *   POINT    the texel NEAREST + REPEAT names: per axis of n texels, floor(u * n) & (n - 1) when n is a power of
 *            two, else min((int)(min(u - floor(u), 0.99999994f) * n), n - 1).
 *   LINEAR   the four REPEAT-wrapped taps and weights of GL's LINEAR filter (x = u * n - 0.5, or
 *            (u - floor(u)) * n - 0.5 when n is no power of two; i0 = floor(x), w = x - i0), lerped as the texture's
 *            storage does: fma(w, b - a, a), x then y, on floats (f32; f16 after the exact unpack), 8.8 fixed point on
 *            the bytes (rgba8: w8 = rint(w * 256), (a * 256 + (b - a) * w8 + 128) >> 8, the result k * (1/255)).
 *   Texels   a texel's value is what rc2dgi_download returns for it as floats -- the list under rc2dgi_compose:
 *            JUMP1 / JUMP2 decoded, DIST its hi / lo bytes, COLOR the input before the first frame and the merged
 *            output after, GI2 (0, 0, 0, 1) with one cascade.  These are the functions rc2dgi_compose's kernel calls: a
 *            sample equals what a view would fetch at that texcoord.
 *   A point with a non-finite u or v yields four quiet NaNs (0x7FC00000) and reads no memory; every finite value,
 *   however large, addresses a texel of the texture (the index is masked or clamped).  n == 0 is a successful no-op.
 *
 * Ray casts: SampleRadianceSDF (RadianceCascades.fs:60-92) for n rays, over the last frame's distRT, the input
 * colorRT (the painted scene, not the merged output) and emissiveRT as they are now.  With asp = (W, H) / max(W, H)
 * (_Aspect, RC2DGI.cs:273) and t = t0, each of at most 32 steps evaluates, every operation single and unfused, in
 * this order,
 *            px = ox + (t * dx) * asp.y,  py = oy + (t * dy) * asp.x
 * (the direction as given: it is not normalised) and applies in order:
 *   1. t > t1: RC2DGI_RAY_RANGE;
 *   2. else px < 0 || py < 0 || px > 1 || py > 1: RC2DGI_RAY_EDGE;
 *   3. else read q, the 16-bit distance of texel (ix, iy) = the POINT texel of (px, py) above (so px == 1.0 reads
 *      column 0, as the shader's REPEAT fetch does); d = (float)q / 65535.0f;
 *   4. d < 0.001f: a hit at that texel.  With e its emissive texel, sqrtf(e.x * e.x + e.y * e.y + e.z * e.z) > 0:
 *      RC2DGI_RAY_EMISSIVE, rgba = (e.rgb, 1); otherwise RC2DGI_RAY_SURFACE, rgba = (color.rgb, _Reflectivity);
 *   5. otherwise t += d.
 * 32 texels read without an exit: RC2DGI_RAY_STEPS.  In the hit record, steps is the number of distRT texels read
 * (0 .. 32); t the value that ended the loop (RC2DGI_RAY_STEPS: after the 32nd increment); (u, v) the last position
 * evaluated; (ix, iy) the hit texel in GL order (row 0 at the bottom) or (-1, -1) without a hit; rgba (0, 0, 0, 1)
 * for RANGE, EDGE and STEPS, the shader's initial `hit`.  The march is the same in every storage mode (distRT is the
 * same 16-bit q, the inputs are floats in all three).
 * A ray with a non-finite field or a field of magnitude above 2^20 is RC2DGI_RAY_INVALID: every other field of its
 * record is 0, ix = iy = -1, and no memory is read.  Within that bound no position overflows or becomes NaN: t grows
 * by at most 1 a step (d <= 1), so |t * dx| <= (2^20 + 32) * 2^20 < 2^41, asp <= 1, and the sum with |ox| <= 2^20 is
 * far inside float range; every product and sum is of finite numbers.
 *
 * The host variants are synchronous w.r.t. the host pointers: they synchronise the context stream (a cascade chain
 * timeout returns RC2DGI_E_DEVICE, as rc2dgi_compose does), run the kernel over context-owned device buffers and copy
 * the results back.  The _device variants take device pointers on the context's device, enqueue the kernel on the
 * context stream, after whatever frame is in flight, and return; the caller keeps the buffers alive until
 * rc2dgi_sync().
 * Errors, each leaving the context valid: RC2DGI_E_ARG for a null context, a null pointer with n > 0, n < 0 or
 * n > 1 << 24, a bad `which` or `filter`, a device pointer not aligned to 8 bytes (uv), 16 (rgba) or 4 (rays, hits);
 * RC2DGI_E_UNSUPPORTED for RC2DGI_FILTER_LINEAR on a texture other than GI1 / GI2 / BLUR / FINAL_GI and for any of
 * the four calls on a row-strip shard (world > 1: its textures hold windows and bands); RC2DGI_E_STATE for a ray
 * cast before the context's first completed frame (there is no distRT yet; sampling before a frame is allowed, as
 * rc2dgi_compose allows it).  These calls only add exports: RC2DGI_ABI_VERSION stays 5. */
int rc2dgi_sample(rc2dgi_ctx *ctx, int which, int filter, const float *uv, int n, float *rgba);
int rc2dgi_sample_device(rc2dgi_ctx *ctx, int which, int filter, const void *uv_dev, int n, void *rgba_dev);

typedef struct rc2dgi_ray {
  float ox, oy;              /* origin, GL texture coordinates */
  float dx, dy;              /* direction, used as given */
  float t0, t1;              /* the interval marched */
} rc2dgi_ray;                /* 24 bytes, blittable */
typedef struct rc2dgi_rayhit {
  int status;                /* RC2DGI_RAY_* */
  int steps;                 /* distRT texels read */
  int ix, iy;                /* the hit texel (GL order), or (-1, -1) */
  float t, u, v;             /* where the loop ended */
  float r, g, b, a;          /* the shader's hit record */
} rc2dgi_rayhit;             /* 44 bytes, blittable */
enum { RC2DGI_RAY_INVALID = -1, RC2DGI_RAY_RANGE = 0, RC2DGI_RAY_EDGE = 1, RC2DGI_RAY_EMISSIVE = 2,
       RC2DGI_RAY_SURFACE = 3, RC2DGI_RAY_STEPS = 4 };
int rc2dgi_raycast(rc2dgi_ctx *ctx, const rc2dgi_ray *rays, int n, rc2dgi_rayhit *hits);
int rc2dgi_raycast_device(rc2dgi_ctx *ctx, const void *rays_dev, int n, void *hits_dev);

/* ---- region statistics: rectangles of a render texture measured without downloading it.  (The light arriving at a
 * sprite: the mean of FINAL_GI over the sprite's texels; an exposure: the maximum and mean of FINAL_GI; health: the
 * count of NaN and infinite texels.)  For each of n rectangles and each channel: how many values are not finite, the
 * smallest and the largest finite value, and the float64 sum of the finite values in ONE fixed order, so that a
 * result is the same bits on every run and equals a restatement on the host.
 *
 * Texture and rectangle.
 *   which    any rc2dgi_rt, RC2DGI_RT_FINAL_GI included.
 *   Texels   a texel's value is what rc2dgi_download returns for it as floats -- the list under rc2dgi_compose (JUMP1 /
 *            JUMP2 decoded, DIST its hi / lo bytes, COLOR the input before the first frame and the merged output
 *            after, GI2 (0, 0, 0, 1) with one cascade), through the decoder the views and the point samples use: a
 *            1 x 1 rectangle equals a RC2DGI_FILTER_POINT sample at that texel's centre.
 *   rect     texels of that texture in GL order (row 0 = the bottom, as rc2dgi_download returns them).  With TW x TH
 *            the texture's size, a rectangle is valid when w >= 1, h >= 1, x >= 0, y >= 0, w <= TW - x and
 *            h <= TH - y (compared in this form: nothing overflows, whatever the four ints hold).  Any other
 *            rectangle yields status = RC2DGI_STATS_INVALID with every other field 0 and reads no texture memory;
 *            the other records of the array are unaffected.  There is no wrap and no clipping.
 *
 * Per channel (r, g, b, a = 0 .. 3).
 *   Each value enters as x + 0.0f: -0.0 becomes +0.0 and nothing else changes.  Subnormals are values like any other
 *   (not flushed).  A NaN or +-inf is counted in nonfinite[c] and takes no part in min, max or sum of that channel.
 *   min / max are the smallest and the largest finite value (every order gives the same result: no -0.0 is left).
 *   With no finite value in the channel, min = +inf, max = -inf and sum = 0.0.
 *
 * The sum is float64 in one fixed order.
 *   Leaf (i, j), 0 <= i < w, 0 <= j < h, is the exact conversion to double of that finite value, or +0.0 for an
 *   excluded one.
 *   A row is reduced by the adjacent-pair tree over P = the smallest power of two >= w leaves, the leaves from w up
 *   being +0.0: level by level s[i] = s[2i] + s[2i+1], until one value is left.
 *   The h row sums are reduced by the same tree, padded to the power of two >= h.
 *   No leaf is -0.0 and no sum of these can be, so x + 0.0 == x everywhere: an implementation may skip all-padding
 *   subtrees and use a + b == b + a freely.  Equivalently: a sequence of length 1 is its value, a longer one splits
 *   at the largest power of two below its length into left + right.
 *   Nothing overflows: |v| < 2^128 and there are at most 2^30 leaves.
 *   sum[c] / (texels - nonfinite[c]) is the mean of the finite values; the library does not divide.
 *
 * Calls.  `rects` is host memory in both variants, read only during the call (as the views of rc2dgi_compose_device
 * and the primitives of rc2dgi_paint are): the host validates the rectangles and plans the work from them.
 * rc2dgi_reduce synchronises the context stream (a cascade chain timeout returns RC2DGI_E_DEVICE, as rc2dgi_compose
 * does), runs the kernels over context-owned device buffers and copies the n records back.  rc2dgi_reduce_device
 * enqueues the kernels on the context stream, after whatever frame is in flight, and returns.  Up to 4 rectangles
 * travel in the kernels' arguments; a longer list is planned into host memory and copied stream-ordered, a batch at a
 * time, as rc2dgi_paint copies its primitives: the runtime may stage such a copy from pageable memory or wait for it
 * on the host, so with a long list the call may return only when the work queued before it has run (not measured).
 * stats_dev is a device pointer on the context's device, aligned to 8 bytes, with room for n records, that the
 * caller keeps alive until rc2dgi_sync().  Reducing before the first frame is allowed, as sampling is (COLOR is then
 * the input).  n == 0 is a successful no-op.
 * Errors, each leaving the context valid: RC2DGI_E_ARG for a null context, a null pointer with n > 0, n < 0 or
 * n > 1 << 20, a bad `which`, a stats_dev not aligned to 8 bytes; RC2DGI_E_UNSUPPORTED on a row-strip shard
 * (world > 1: its textures hold windows and bands).  These calls only add exports: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_rect {
  int x, y, w, h;            /* texels of that texture, GL order (row 0 = bottom) */
} rc2dgi_rect;               /* 16 bytes, blittable */
enum { RC2DGI_STATS_OK = 0, RC2DGI_STATS_INVALID = -1 };
typedef struct rc2dgi_stats {
  int status;                /* RC2DGI_STATS_* */
  int texels;                /* w * h */
  int nonfinite[4];          /* per channel r, g, b, a: values that are NaN or +-inf */
  float min[4], max[4];      /* of the finite values */
  double sum[4];             /* offset 56: of the finite values, in the order above */
} rc2dgi_stats;              /* 88 bytes, 8-byte aligned, blittable */
int rc2dgi_reduce(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rects, int n, rc2dgi_stats *stats);
int rc2dgi_reduce_device(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rects, int n, void *stats_dev);

/* ---- edge tables: tone curves for the views and histograms of rectangles.  (An exposure for the HDR final GI that
 * rc2dgi_compose clamps into 8 bits: histogram its luminance, take a percentile, show the frame through
 * rc2dgi_compose_tone with that exposure and an sRGB or filmic curve -- nothing is downloaded.)  Both rest on one
 * primitive that is exact on any hardware: a table of m ascending float edges e[0] <= e[1] <= .. <= e[m-1] with
 *
 *            bin(v) = the number of edges e[i] with e[i] <= v            (0 .. m; IEEE <=, no rounding anywhere)
 *
 * With 255 edges bin is a tone curve, any monotone map from a float to a byte: the host computes the edges of sRGB,
 * gamma, Reinhard or a filmic curve in whatever precision it likes and the device evaluates no transcendental.  With
 * m edges bin is a histogram's bin index.  A restatement on the host (a linear scan) equals the device bit for bit.
 *   Edges may repeat (a repeated edge makes a bin that is always empty) and may be +-inf or -0.0; IEEE <= treats -0.0
 *   and +0.0 alike, so -0.0 >= a +0.0 edge.  A value equal to an edge lands above it.  bin(NaN) is undefined at this
 *   level: each caller below says what a NaN becomes.
 * rc2dgi_check_edges (host-only): RC2DGI_OK, or RC2DGI_E_ARG for a null table, m < 1, a NaN edge or e[i] > e[i+1].
 * rc2dgi_curve_q8 (host-only): the 255 edges with bin(v) == q8(v) = rint(clamp(v, 0, 1) * 255) for every float v that
 * is no NaN (q8(NaN) = 0 is the callers' NaN rule below): edge k - 1, k = 1 .. 255, is the smallest non-negative float
 * x with q8(x) >= k, found by bisection over float bit patterns (the bits of a non-negative float order as the float
 * does) on q8 as rc2dgi_device.h states it.  The table is strictly ascending and edge 127 (k = 128) is exactly 0.5f:
 * 0.5f * 255 = 127.5 rounds to the even 128. */
#define RC2DGI_CURVE_EDGES 255
#define RC2DGI_MAX_CURVES 8
#define RC2DGI_HIST_MAX_EDGES 1023
int rc2dgi_check_edges(const float *edges, int m);
int rc2dgi_curve_q8(float *edges255);

/* ---- toned views: rc2dgi_compose with an exposure and a tone curve per view.
 * Everything said under rc2dgi_compose holds word for word -- clear, draw order, sampling, texel decode, border,
 * errors, the refusal on a row-strip shard, the host variant's synchronisation and chain timeout (RC2DGI_E_DEVICE) --
 * with one step changed.  Where a draw forms its 8-bit source from the sampled float4 (r, g, b, a), view k uses
 *            (T(r * E), T(g * E), T(b * E), q8(a)),     E = tones[k].exposure, each product ONE fp32 multiply,
 *   T = q8                               when tones[k].curve == 0,
 *   T(v) = isnan(v) ? 0 : bin(v)         over the 255 edges of curve slot tones[k].curve otherwise.
 * Alpha and the border colour are not toned; the blend is unchanged.  tones == NULL, or every record {1.0f, 0}, is
 * rc2dgi_compose exactly (x * 1.0f is x for every float, a NaN stays one); so is {1.0f, s} with rc2dgi_curve_q8's table
 * in slot s.  Any render texture in any storage mode may be toned: the value toned is the float rc2dgi_download
 * returns (DIST at exposure 255 shows which texels have a non-zero low byte, the faintest distances).  0 * inf is NaN
 * and shows as 0.
 * rc2dgi_set_curve(ctx, slot, edges255): slot 1 .. RC2DGI_MAX_CURVES; copies the 255 edges into the context during the
 * call, and from there, ordered on the context stream, into a context-owned device table: a compose enqueued before
 * the call keeps the old curve, one enqueued after it uses the new one.  edges255 == NULL clears the slot.
 * Errors, each leaving the context valid: those of rc2dgi_compose; RC2DGI_E_ARG for an exposure that is NaN, infinite
 * or negative, a curve outside 0 .. RC2DGI_MAX_CURVES, a slot outside 1 .. RC2DGI_MAX_CURVES, a table that
 * rc2dgi_check_edges refuses; RC2DGI_E_STATE for a view that names a slot that is not set.  These calls only add
 * exports: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_tone {
  float exposure;            /* E >= 0, finite */
  int curve;                 /* 0: q8; 1 .. RC2DGI_MAX_CURVES: that slot's table */
} rc2dgi_tone;               /* 8 bytes, blittable */
int rc2dgi_set_curve(rc2dgi_ctx *ctx, int slot, const float *edges255);
int rc2dgi_compose_tone(rc2dgi_ctx *ctx, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w, int out_h,
                        const unsigned char *clear_rgba, void *host, int pitch_bytes);
int rc2dgi_compose_tone_device(rc2dgi_ctx *ctx, const rc2dgi_view *views, const rc2dgi_tone *tones, int n, int out_w,
                               int out_h, const unsigned char *clear_rgba, void *dev, int pitch_bytes);

/* ---- histograms of rectangles: for each of n rectangles of a render texture, how many of its texels fall into each
 * bin of an edge table.
 *   which, texels, rect   exactly as for rc2dgi_reduce: any rc2dgi_rt, a texel's value is what rc2dgi_download returns,
 *            a rectangle is valid when w >= 1, h >= 1, x >= 0, y >= 0, w <= TW - x and h <= TH - y (compared in this
 *            form), with no wrap and no clipping.
 *   channel  the scalar s of a texel (r, g, b, a): RC2DGI_CH_R / _G / _B / _A that channel as it is, RC2DGI_CH_LUMA
 *            ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b): five single, unfused fp32 operations in that order.
 *   edges    m ascending edges, 1 <= m <= RC2DGI_HIST_MAX_EDGES, as rc2dgi_check_edges admits them.
 *   counts   record k is m + 4 32-bit words at counts + k * (m + 4): {status, texels, nan, bin[0] .. bin[m]}.
 *            status is RC2DGI_STATS_OK and texels = w * h; a NaN scalar counts in nan, every other scalar, +-inf
 *            included, in bin[bin(s)]: nan + the sum of the bins == texels.  An invalid rectangle yields status =
 *            RC2DGI_STATS_INVALID (the word 0xFFFFFFFF) with every other word 0 and reads no texture memory; the other
 *            records are unaffected.
 * Determinism: the counts are integers, and integer addition gives the same words in any order.  That is the whole
 * argument -- the kernel adds with integer atomics in whatever order the hardware schedules, and no float is ever
 * accumulated.
 * Calls.  `rects` and `edges` are host memory in both variants, read only during the call.  The call initialises every
 * word of the n records itself: the caller's buffer may hold anything.  rc2dgi_histogram synchronises the context
 * stream (a cascade chain timeout returns RC2DGI_E_DEVICE, as rc2dgi_compose does), runs the kernels over context-owned
 * device buffers and copies the records back.  rc2dgi_histogram_device enqueues behind whatever frame is in flight
 * and returns; counts_dev is a device pointer on the context's device, aligned to 4 bytes, that the caller keeps alive
 * until rc2dgi_sync().  Up to 4 rectangles travel in the kernel's arguments, a longer list in batches as for
 * rc2dgi_reduce_device (with the same remark on when such a call returns).  n == 0 is a successful no-op.
 * Histogramming before the first frame is allowed (COLOR is then the input).
 * Errors, each leaving the context valid: RC2DGI_E_ARG for a null context, a null pointer with n > 0, m outside
 * 1 .. RC2DGI_HIST_MAX_EDGES, edges that rc2dgi_check_edges refuses, a bad channel or `which`, n < 0 or n > 1 << 20,
 * (long long)n * (m + 4) > 1 << 26, a counts_dev not aligned to 4 bytes; RC2DGI_E_UNSUPPORTED on a row-strip shard.
 * These calls only add exports: RC2DGI_ABI_VERSION stays 5. */
enum { RC2DGI_CH_R = 0, RC2DGI_CH_G = 1, RC2DGI_CH_B = 2, RC2DGI_CH_A = 3, RC2DGI_CH_LUMA = 4 };
int rc2dgi_histogram(rc2dgi_ctx *ctx, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges, int m,
                     unsigned *counts);
int rc2dgi_histogram_device(rc2dgi_ctx *ctx, int which, int channel, const rc2dgi_rect *rects, int n, const float *edges,
                            int m, void *counts_dev);

/* ---- a rectangle of a render texture as an image, converted on the device.  (The HDR final GI as a tensor for a
 * PyTorch consumer, a sprite-sized crop of it for the host, a frame saved as half floats -- without rc2dgi_download's
 * copy of the whole texture at 16 bytes a texel and its conversion on one host thread.)
 *   which, rect   as for rc2dgi_reduce: any rc2dgi_rt, RC2DGI_RT_FINAL_GI included; texels in GL order (row 0 = the
 *            bottom); valid when w >= 1, h >= 1, x >= 0, y >= 0, w <= TW - x and h <= TH - y (compared in this form).
 *            rect == NULL is the whole texture.  There is no wrap and no clipping.  One call is one image: an invalid
 *            rectangle is RC2DGI_E_ARG and nothing is written (it is not a per-record status).
 *   Pixels   pixel (i, j) of the image, 0 <= i < w, 0 <= j < h, is texel (x + i, y + j); with RC2DGI_READ_FLIP in
 *            `flags` it is texel (x + i, y + h - 1 - j): image row 0 is the rectangle's TOP row, the window's order, as
 *            rc2dgi_compose writes.  The texel's value is what rc2dgi_download returns for it as floats, through the
 *            decoder the views use -- the list under rc2dgi_compose (JUMP1 / JUMP2 decoded, DIST its hi / lo bytes,
 *            COLOR the input before the first frame and the merged output after, GI2 (0, 0, 0, 1) with one cascade,
 *            FINAL_GI the alias).
 *   Formats  RC2DGI_FMT_RGBA32F: the four floats as they are (a NaN stays a NaN; its payload is not part of the
 *            contract).  RC2DGI_FMT_RGBA8: q8 per channel, rint(clamp(x, 0, 1) * 255), NaN -> 0: the bytes
 *            rc2dgi_download(.., RC2DGI_FMT_RGBA8) gives.  RC2DGI_FMT_RGBA16F: each float converted to IEEE binary16
 *            with round to nearest, ties to even -- magnitudes from 65520 up become +-inf, results below 2^-14 are
 *            binary16 subnormals (not flushed), magnitudes up to 2^-25 become +-0 (the sign of zero is kept), a NaN
 *            becomes a NaN (payload unspecified): what numpy's and torch's float32 -> float16 do.  It is not the
 *            round-toward-zero pack that RC2DGI_STORAGE_F16 stores with.
 *   Pitch    pitch_bytes == 0 is a tight row: w * 16, w * 8 or w * 4 bytes.  Bytes of a row past that, and rows past
 *            h, are not written.  rc2dgi_read_device requires `dev` aligned to a pixel (16 / 8 / 4 bytes for RGBA32F /
 *            RGBA16F / RGBA8) and pitch_bytes a multiple of that; the host variant has no alignment rule.
 * Calls.  rc2dgi_read synchronises the context stream (a cascade chain timeout returns RC2DGI_E_DEVICE, as
 * rc2dgi_compose does), runs the kernel into a context-owned staging buffer and copies the rows out.  The staging is
 * 8 MiB of device memory whatever the image, allocated at the first call and freed with the context: a larger
 * rectangle goes through it in blocks of whole rows.  rc2dgi_read_device enqueues the kernel on the context stream,
 * after whatever frame is in flight, and returns; `dev` is a device pointer on the context's device that the caller
 * keeps alive until rc2dgi_sync().  Reading before the first frame is allowed (COLOR is then the input).
 * Errors, each leaving the context valid and the destination untouched: RC2DGI_E_ARG for a null context or
 * destination, a bad `which` or `format`, a flag bit other than RC2DGI_READ_FLIP, an invalid rectangle, a pitch smaller
 * than a row and, for the device variant, a misaligned pointer or pitch; RC2DGI_E_UNSUPPORTED on a row-strip shard
 * (world > 1: its textures hold windows and bands).  These calls only add exports: RC2DGI_ABI_VERSION stays 5. */
enum { RC2DGI_READ_FLIP = 1 };
int rc2dgi_read(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rect, int format, int flags, void *host,
                int pitch_bytes);
int rc2dgi_read_device(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rect, int format, int flags, void *dev,
                       int pitch_bytes);

/* ---- an image into a rectangle of an input texture, converted on the device: rc2dgi_read the other way.  (A sprite
 * or a light cookie drawn with DrawTextureRec into colorRT / emissiveRT, a half tensor of a PyTorch producer, the
 * 64 x 64 texels of a 4096^2 scene that changed -- without rc2dgi_upload's copy of the whole texture at 16 bytes a
 * texel and its conversion on one host thread.)
 *   which, rect   RC2DGI_RT_COLOR or RC2DGI_RT_EMISSIVE, the two inputs (the ids rc2dgi_upload takes); anything else is
 *            RC2DGI_E_ARG.  The rectangle is valid exactly as for rc2dgi_read: w >= 1, h >= 1, x >= 0, y >= 0,
 *            w <= W - x and h <= H - y (compared in this form); texels in GL order (row 0 = the bottom); rect == NULL is
 *            the whole texture.  There is no wrap and no clipping: an invalid rectangle is RC2DGI_E_ARG and nothing is
 *            written.
 *   Pixels   pixel (i, j) of the image, 0 <= i < w, 0 <= j < h, goes to texel (x + i, y + j); with RC2DGI_WRITE_FLIP in
 *            `flags` to texel (x + i, y + h - 1 - j): image row 0 is then the rectangle's TOP row, the order
 *            rc2dgi_compose and rc2dgi_read(.., RC2DGI_READ_FLIP) produce.
 *   Values   the inputs are float4 texels in all three storage modes.  The value a pixel becomes:
 *            RC2DGI_FMT_RGBA32F: the four floats as they are in F32 and F16 storage (a NaN stays a NaN; its payload is
 *            not part of the contract); in RC2DGI_STORAGE_RGBA8_COMPAT they are quantized as rc2dgi_upload quantizes a
 *            float image, q8 and then k * (1/255): rint(clamp(x, 0, 1) * 255) * (1.0f / 255.0f), NaN -> 0.
 *            RC2DGI_FMT_RGBA8: byte k becomes (float)k / 255.0f, one IEEE division, in F32 and F16 storage, and
 *            (float)k * (1.0f / 255.0f) in RGBA8_COMPAT storage: what rc2dgi_upload and rc2dgi_upload_device make of it.
 *            RC2DGI_FMT_RGBA16F: each binary16 is widened exactly to float -- a subnormal becomes its exact value,
 *            +-inf stays +-inf, a NaN stays a NaN (payload unspecified) -- and the result is treated as RGBA32F.  A
 *            write of the image rc2dgi_read(.., RC2DGI_FMT_RGBA16F) returned, read back as RGBA16F, is that image.
 *            So a write of the whole texture leaves the bits rc2dgi_upload of the same image leaves, in every storage
 *            mode, for RGBA32F and RGBA8.
 *   Blend    without RC2DGI_WRITE_BLEND the value replaces the texel.  With it the texel becomes blend(value, texel),
 *            the SRC_ALPHA / ONE_MINUS_SRC_ALPHA blend on all four channels that the render textures apply on every
 *            draw: in F32 and F16 storage value.c * a + texel.c * (1 - a) with a = value.a, every operation single and
 *            unfused; in RGBA8_COMPAT storage the 8-bit blend min(255, mul8(s8, a8) + mul8(d8, 255 - a8)) * (1/255)
 *            with s8 = q8(value.c), a8 = q8(value.a), d8 = q8(texel.c) and mul8(x, y) = (x*y*257 + 32768) >> 16.  These
 *            are the functions rc2dgi_paint blends with: a constant image holding a primitive's colour, blended over
 *            an integer rectangle, equals rc2dgi_paint of that DrawRectangle without a clear.  A non-finite value or
 *            alpha gives whatever those expressions give (in float storage NaN and inf propagate by IEEE rules, 0 * inf
 *            is NaN; in RGBA8_COMPAT storage q8 has clamped them first: NaN and -inf to 0, +inf to 255).
 *   Pitch    pitch_bytes == 0 is a tight row: w * 16, w * 8 or w * 4 bytes.  Bytes of a source row past the w pixels
 *            are not read.  rc2dgi_write_device requires `dev` aligned to a pixel (16 / 8 / 4 bytes for RGBA32F /
 *            RGBA16F / RGBA8) and pitch_bytes a multiple of that; the host variant has no alignment rule.  The source
 *            must not overlap the context's own textures.
 * Calls.  rc2dgi_write_device enqueues the kernel on the context stream and returns; `dev` is a device pointer on the
 * context's device that the caller keeps alive until rc2dgi_sync().  A frame enqueued before the call computes from
 * the old texels, a frame enqueued after it from the new ones.  rc2dgi_write is synchronous with respect to `host`, as
 * rc2dgi_upload is: it synchronises the context stream (a cascade chain timeout returns RC2DGI_E_DEVICE), copies rows
 * into the 8 MiB staging buffer of rc2dgi_read in blocks of whole rows -- the image crosses the bus in its own format
 * -- runs the kernel per block and returns when the last block is written.  Both do to the context's state what
 * rc2dgi_upload_device does: a write to COLOR makes COLOR the input again (the old input with the rectangle changed:
 * the merged output of the last frame is another buffer).  Writing before the first frame is allowed.  Both are
 * accepted on a row-strip shard, as rc2dgi_upload is: the inputs are replicated whole on every rank, and the caller
 * writes the same thing on every rank.
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in this order, for a null
 * context or source, a bad `which`, a bad `format`, a flag bit other than the two defined, an invalid rectangle, a pitch
 * smaller than a row and, for the device variant, a misaligned pointer or pitch.  These calls only add exports:
 * RC2DGI_ABI_VERSION stays 5. */
enum { RC2DGI_WRITE_FLIP = 1, RC2DGI_WRITE_BLEND = 2 };
int rc2dgi_write(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rect, int format, int flags, const void *host,
                 int pitch_bytes);
int rc2dgi_write_device(rc2dgi_ctx *ctx, int which, const rc2dgi_rect *rect, int format, int flags, const void *dev,
                        int pitch_bytes);

/* cascade resolution (RC2DGI.cs:70-77), JFA step count (RC2DGI.cs:289-292) and which
 * giRT holds the final GI (1 or 2, RC2DGI.cs:365) */
int rc2dgi_query(rc2dgi_ctx *ctx, int *cascade_w, int *cascade_h, int *jfa_steps, int *final_gi);
const char *rc2dgi_last_error(rc2dgi_ctx *ctx);
int rc2dgi_abi_version(void);

/* ---- stream / timing.  rc2dgi_set_stream: run on a caller-owned hipStream_t on the
 * context's device (NULL = back to the context's own stream).  It waits until the stream the
 * context leaves has run everything enqueued on it, so what follows on the new stream sees the
 * frames and writes enqueued before the call, whatever the two streams know of each other; the
 * caller orders the new stream's own earlier work.  rc2dgi_set_timing(ctx, mode):
 * 0 off; 1 rc2dgi_do() records HIP events around each pass and each RC level; 2 around each
 * pass only (every event idles the GPU a few microseconds before the next kernel, so mode 2
 * times the RC pass as it runs untimed).  rc2dgi_pass_times() returns the last frame's
 * milliseconds in the order {screenuv, jfa (all steps, DF fused into the last), rc (all N
 * levels), blur (+copy-back), merge (+copy-back), total} and, when level_ms != NULL (the
 * last frame ran in mode 1, else RC2DGI_E_STATE), the N per-level RC times indexed by level. */
int rc2dgi_set_stream(rc2dgi_ctx *ctx, void *hip_stream);
int rc2dgi_set_timing(rc2dgi_ctx *ctx, int enable);
int rc2dgi_pass_times(rc2dgi_ctx *ctx, float *pass_ms, int n_pass, float *level_ms, int n_level);

/* ---- transcendental tables.  rc2dgi_do() evaluates cos/sin (RadianceCascades.fs:117-121)
 * and the sky integral (RadianceCascades.fs:48-57, 150-154) as correctly rounded fp32
 * tables.  A host may instead supply the exact values its GL implementation produces
 * (used by the parity tests to reproduce llvmpipe bit-for-bit); pass NULL to revert. */
int rc2dgi_set_direction_table(rc2dgi_ctx *ctx, int level, const float *cos_sin, int n);
int rc2dgi_set_sky_table(rc2dgi_ctx *ctx, const float *rgb, int n);

/* ---- tuning knobs (performance only; results are identical for every value).
 * A per-level key ends in "_L<n>", n the level in decimal digits (0 .. cascade_count-1); where a key without the
 * suffix is listed beside it, that key sets every level at once and cannot be read.  Every other key rc2dgi_set_tuning
 * takes, rc2dgi_get_tuning returns.  A value out of range, a level out of range and an unknown key are RC2DGI_E_ARG and
 * change nothing.  Knobs said to be 1 (or 0) "by default" without other values take any value as value != 0.
 *   "rc_variant"      RC workgroup tile shape for every level (0 .. rc_variant_count-1)
 *   "rc_variant_L<n>" the same for level n only (default: 0 at levels 0..2, 13 from level 3 up)
 *   "blur_path"       blur / copy-back / merge kernels: 0 auto (fixed-tap blur with merge fused
 *                     where the sizes allow), 1 LDS-tiled blur + copy-back, then merge,
 *                     2 separate blur, copy-back and merge passes
 *   "rc_order_L<n>"   workgroup order of level n: px | py << 8 | dg << 16 = patches of px x py
 *                     probe tiles x groups of dg direction blocks (0: tile-major, the default of levels 0..2; from
 *                     level 3 up the default is 2 | 2 << 8 | 8 << 16); any value >= 0
 *   "poison"          debug, 0 (default) / 1: fill the intermediate render textures with 0xFF bytes before each
 *                     frame (rows a sharded frame never computes then read as NaN)
 *   "rc_skip"         march exit proofs from a coarse lower bound of distRT (the last sample of a
 *                     ray that misses is not read when the bound already proves the miss):
 *                     0 off, 1 auto (screens >= 2048), 2 interval only, 3 interval + screen edge
 *   "rc_wgproof"      1 (default): a workgroup whose first samples all provably miss skips the march
 *   "rc_tail" / "rc_tail_L<n>"  rays still marching after this many lockstep iterations finish one
 *                     per lane in a compacted queue (-1: every ray from the start; 0 off; up to 32; default 10)
 *   "rc_mp" / "rc_mp_L<n>"  1 (default): the one-probe tiles of a level with at least 64 direction blocks (level 3 up) skip rays that
 *                     the directional clear table proves to miss
 *   "rc_noproof_L<n>" 0 (default); 1: level n marches without the bound table (no exit or miss proofs)
 *   "rc_pal"          1 (default): surface palettes -- the side pass keeps the records of a cell's hittable texels as
 *                     a per-cell palette, and the plain-field levels march on a field that carries the palette index
 *                     (square power-of-two screens from 4096 up to 8192)
 *   "jfa_coset"       the first JumpFlood steps in one kernel: 2 (default) five steps (four on screens wider than
 *                     4096), 1 four steps, 0 off
 *   "jfa_lds"         0 (default); 1: the short JumpFlood steps stage their taps in LDS
 *   "shade_fused"    1 (default): surface records and the proofs' bound table in one pass over
 *                     distRT where its cells are >= 64 texels (square power-of-two screens >= 4096)
 *   "shade_split"     1 (default): that pass split in two, a light scan of every cell and the records and
 *                     surface palettes of the cells holding a hittable texel
 *   "side_overlap"    with the split pass, the directional clear table beside the records of the hit cells:
 *                     2 (default): its workgroups appended to the records launch; 1: on a second stream (the
 *                     fork / join costs more than it overlaps); 0: after the records, one launch of its own
 *   "jfa_rt"          rows per lane of the JumpFlood steps on small non-power-of-two screens: 1 (default),
 *                     2, 4
 *   "rc_chain"        0 (default); 1 / 2: the levels below the top in ONE launch of 16x16x1 tiles, a tile
 *                     starting when the upper tiles under its footprint are written (2: unrolled march);
 *                     4: the top level in that launch too; f32 cascades, one process.  A wait that times out
 *                     makes the next rc2dgi_sync / rc2dgi_download / rc2dgi_download_level / rc2dgi_compose /
 *                     rc2dgi_reduce / rc2dgi_compose_tone / rc2dgi_histogram / rc2dgi_read / rc2dgi_do / rc2dgi_do_phase return
 *                     RC2DGI_E_DEVICE and turns the chain off for the context
 *                     (never a silent wrong frame)
 *   "rc_chain_spin"   diagnostic: polls per chain wait (0: the default bound; -1: every wait times out at once)
 *   "jfa_rows"        0 (default), 4, 8: the short isotropic JumpFlood steps (offsets 1, 2, 4 on square power-of-two
 *                     screens) with that many consecutive rows per lane, each tap row loaded once (measured no faster)
 *   "cascade_band"    1 (default): row-strip shards on strip tables and the fused blur + merge band GI1 / GI2 (see
 *                     rc2dgi_device_buffer); 0: whole textures
 *   "rc_fill"         1 (default): a level whose every ray starts off screen (proven on the host from the uploaded
 *                     directions; with every level above it such a level too) is written as its per-direction-block
 *                     values (the merge of rays that take no sample with the sky or the upper block values) -- f32
 *                     frames without rc_chain; get_tuning "rc_fill_levels": the levels the last frame filled (bits)
 *   "rc_rdiv"         1 (default): non-power-of-two cascades divide by the cascade resolution as x * (1/n) plus one
 *                     fused correction on the levels where the context proved that equal to the IEEE quotient for
 *                     every numerator (get_tuning "rc_rdiv_levels": bit L set when level L does on both axes); 0: divide
 *   "jfa_tab"         the float-path JumpFlood steps' fragTexCoords (i + 0.5) / n: 2 (default) x * (1/n) plus one
 *                     fused correction, used where the context proved it equal to the division for every index (else
 *                     as 1); 1 from a per-context table (W + H <= 8192); 0 divided per tap
 *   "jfa_tail"        0 (default), 2, 3, 4: the last that many JumpFlood steps in one LDS-tiled kernel (square
 *                     power-of-two screens up to 16384)
 *   "strip_tables"    1 (default; f32 storage): row-strip shards build the march's side tables for their own cell rows and exchange
 *                     them with the march field instead of all-gathering distRT; no record texture (see the sharding
 *                     section below); get_tuning "strip_tables_active" tells whether the last frame did
 *   "paint_plan"      the tile height and the batch of rc2dgi_paint_device and rc2dgi_sprites_device: 0 (default) as the
 *                     screen size gives them (tiles of 64 x 4 texels and batches of 8192 while a mask of one bit a
 *                     tile and primitive fits 40 MiB; then tiles of 8 and 16 rows, batches of 4096 and 2048, tiles of
 *                     32, 64 and 128 rows); otherwise log2(tile_h) | (batch / 2048) << 8 with tile_h 4 .. 128 and batch
 *                     2048, 4096 or 8192.  RC2DGI_E_ARG for any other value, and for a plan whose masks would exceed
 *                     40 MiB on this screen (the working memory stays within its 64 MiB).  A set that changes the plan
 *                     of a context whose working memory exists waits for the context stream and frees that memory;
 *                     the next of the two calls allocates it again (their one wait).  rc2dgi_paint_device_limits
 *                     reports the default plan.  get_tuning "paint_tile_h" and "paint_batch": the plan in force
 * rc2dgi_get_tuning also answers "blur_strip_sized" (1: a shard's BLUR / FINAL_GI textures hold its own rows,
 * rc2dgi_device_buffer), "cascade_banded" (1: a shard's GI1 / GI2 hold its band of every direction block,
 * rc2dgi_device_buffer), "rc_variant_count" and "rc_chain_timeouts" (workgroups of the chained
 * frames since the chain was set up that stopped waiting for their upper tiles: 0 in a correct run;
 * synchronises). */
int rc2dgi_set_tuning(rc2dgi_ctx *ctx, const char *key, int value);
/* time `frames` frames per candidate workgroup order x march variant ("rc_variant" 0 / 13 / 14 / 15) on
 * the uploaded scene and keep the fastest per level (like a convolution library's benchmark mode; results are identical for every
 * order).  Runs whole frames on the context stream; synchronous. */
int rc2dgi_autotune(rc2dgi_ctx *ctx, int frames);
int rc2dgi_get_tuning(rc2dgi_ctx *ctx, const char *key, int *value);

/* ---- debug views beyond the reference's thumbnails: keep a copy of every cascade level G_L
 * as stored by its pass (costs N extra cascade textures and one copy per level). */
int rc2dgi_set_keep_levels(rc2dgi_ctx *ctx, int enable);
int rc2dgi_download_level(rc2dgi_ctx *ctx, int level, void *host, int pitch_bytes, int format);
/* the march's side tables of the last frame (no reference counterpart; for checking them): which =
 * RC2DGI_TAB_HITC (64 x 64 bytes: 1 where a cell holds a texel the hit test passes), _CMIN (64 x 64 bytes,
 * lower bounds k / 512), _DCLR (64 bins x 64 x 64 bytes, clear steps), _DBOXES (64 bins x 64 steps x 4 ints),
 * _CELLPAL (64 x 64 cells x 16 float4 palette entries), _MFIELD (H rows x W uint16, the march field).
 * Copies min(bytes, table size) bytes; returns the table size in bytes (or a negative status; a table not
 * built by the last frame is RC2DGI_E_STATE). */
enum { RC2DGI_TAB_HITC = 0, RC2DGI_TAB_CMIN = 1, RC2DGI_TAB_DCLR = 2, RC2DGI_TAB_DBOXES = 3, RC2DGI_TAB_CELLPAL = 4,
       RC2DGI_TAB_MFIELD = 5 };
int rc2dgi_download_table(rc2dgi_ctx *ctx, int which, void *host, int bytes);

/* ---- on-device scene producer: the painted inputs without a host upload.
 * rc2dgi_paint(ctx, COLOR | EMISSIVE, clear, prims, n) is
 *   BeginTextureMode(rt); ClearBackground(clear) [clear != NULL, RGBA 0..255]; draw prims in
 *   order; EndTextureMode()
 * as RenderScene / RedrawSceneToRTs do it (RC2DGI.cs:224-264, 528-545), with raylib 5.5 semantics:
 *   RC2DGI_PRIM_RECT    DrawRectangleRec(x, y, w, h) / DrawRectangle
 *   RC2DGI_PRIM_CIRCLE  DrawCircleV((x, y), radius = w)  (36-segment fan)
 * in raylib screen coordinates (y down), colours as raylib Color, alpha-blended.  Coordinates
 * must be finite with magnitude below 2^22 pixels.  Returns when the texture is painted. */
typedef struct rc2dgi_prim {
  int kind;                  /* RC2DGI_PRIM_RECT | RC2DGI_PRIM_CIRCLE */
  float x, y, w, h;          /* rect: top-left corner and size; circle: centre, w = radius */
  unsigned char r, g, b, a;  /* raylib Color */
} rc2dgi_prim;
enum { RC2DGI_PRIM_RECT = 0, RC2DGI_PRIM_CIRCLE = 1 };
int rc2dgi_paint(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const rc2dgi_prim *prims, int n);

/* ---- the same painting from a primitive list in device memory, enqueued on the context stream.  (Discs and squares
 * a PyTorch producer keeps in a tensor -- a particle system used as lights -- painted without a trip to the host, in a
 * loop that never waits: paint, rc2dgi_do, rc2dgi_read_device.)
 *   prims_dev  n records of rc2dgi_prim (24 bytes each) on the context's device, aligned to 4 bytes; 0 <= n <= 1 << 20.
 *              n == 0 admits a null prims_dev.
 *   count_dev  NULL, or one int32 on the device, aligned to 4 bytes, read on the stream when the work runs: the number
 *              painted is m = min(max(*count_dev, 0), n).  With NULL, m = n.  m == 0 with a clear colour is a clear
 *              only; m == 0 without one leaves the texture as it is.
 *   status_dev NULL, or two int32 on the device, aligned to 4 bytes: the call writes {m, refused} there on the stream,
 *              both words on every call, m == 0 included.
 *   Result     `which`, clear_rgba, draw order, coverage rule, colour conversion, blend and the three storage modes are
 *              those of rc2dgi_paint: for a list rc2dgi_paint accepts, the texture afterwards holds the bits that
 *              rc2dgi_paint(ctx, which, clear_rgba, list, m) leaves.
 *   Refused    the device cannot fail a call, so a primitive that rc2dgi_paint would answer with RC2DGI_E_ARG draws
 *              nothing and is counted in `refused`; the other primitives are unaffected.  With lim = 2^22 and the test
 *              ok(c) = fabsf(c) < lim (false for a NaN and for an infinity), a primitive is refused when
 *                kind is neither RC2DGI_PRIM_RECT nor RC2DGI_PRIM_CIRCLE, or
 *                !ok(x), !ok(y) or !ok(w); for a rectangle also !ok(h), !ok(x + w) or !ok(y + h), the sums in float;
 *                for a circle also !(fabsf(x) + fabsf(w) < lim) or !(fabsf(y) + fabsf(w) < lim) (its h is not read).
 *              Nothing read from prims_dev or count_dev becomes an address, an index or a loop bound before it has
 *              passed this test or that clamp and the primitive's pixel box has been clipped to the target: a buffer
 *              of garbage paints nothing and faults nothing.
 *   Order      the call is enqueued behind whatever is in flight on the context stream and returns; it does not wait
 *              for the stream or the device (the first call of a context allocates the working memory, the one
 *              exception).  The caller keeps the three buffers alive until rc2dgi_sync() and may overwrite them on the
 *              same stream as soon as the call has returned.  A frame enqueued before the call sees the old texels, a
 *              frame enqueued after it the new ones.  Painting COLOR makes COLOR the input again, as rc2dgi_paint does.
 *              Row-strip shards accept the call as they accept rc2dgi_paint.
 *   Memory     the context owns the working memory: allocated at the first call, freed with the context, its size
 *              fixed by the screen size whatever n is, at most 64 MiB.  A list longer than one batch is painted batch
 *              after batch on the stream, the draw order kept across batches (three kernels a batch of the n given,
 *              whatever *count_dev turns out to be: an empty batch's kernels leave at once).
 *              rc2dgi_paint_device_limits (host-only, no device) reports for a config the batch capacity (2048, 4096
 *              or 8192 primitives, by screen size) and the working bytes; either pointer may be NULL.
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in this order, for a null
 * context, a bad `which`, n out of range, a null prims_dev with n > 0, a misaligned pointer;
 * rc2dgi_paint_device_limits: RC2DGI_E_ARG for a null config or a screen size rc2dgi_create refuses.  These calls only
 * add exports: RC2DGI_ABI_VERSION stays 5. */
int rc2dgi_paint_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const void *prims_dev, int n,
                        const void *count_dev, void *status_dev);
int rc2dgi_paint_device_limits(const rc2dgi_config *cfg, int *batch_prims, long long *work_bytes);

/* ---- a sprite list in device memory, drawn from one atlas image, enqueued on the context stream.  (The textured draws
 * of a game that lights its world with this library: walls with albedo into colorRT, light cookies and glowing
 * particles into emissiveRT -- raylib's DrawTextureRec(atlas, source, position, tint) into the render texture, hundreds
 * to tens of thousands of times a frame, in one call instead of one rc2dgi_write_device launch a sprite.)  The values
 * are rc2dgi_write's, the list is rc2dgi_paint_device's.
 *   atlas      a host struct, read during the call: `dev` an image of w x h pixels (1 .. 32768 each) on the context's
 *              device whose row 0 is the TOP row (image order, y down), in `format` RC2DGI_FMT_RGBA8, _RGBA16F or
 *              _RGBA32F; pitch_bytes == 0 is a tight row, otherwise it is at least a row and a multiple of a pixel
 *              (4 / 8 / 16 bytes); `dev` is aligned to a pixel.  The atlas must not overlap the context's textures.
 *   sprites_dev  n records of rc2dgi_sprite (32 bytes, eight 32-bit words each) on the context's device, aligned to 4
 *              bytes; 0 <= n <= 1 << 20.  n == 0 admits a null sprites_dev.
 *   which, clear_rgba, count_dev, status_dev   as for rc2dgi_paint_device: RC2DGI_RT_COLOR or RC2DGI_RT_EMISSIVE; an
 *              optional ClearBackground colour that belongs to the first batch; NULL or one int32 on the device, read on
 *              the stream when the work runs, the number drawn being m = min(max(*count_dev, 0), n), or n with NULL
 *              (m == 0 with a clear colour is a clear only, m == 0 without one leaves the texture as it is); NULL or
 *              two int32 on the device that receive {m, refused} on the stream on every call, m == 0 included.
 *   Pixels     sprite k covers the screen pixels (dx + i, dy + j), 0 <= i < w, 0 <= j < h, in raylib screen coordinates
 *              (y down) as rc2dgi_paint, clipped to the W x H target.  Screen pixel (X, Y) is texel (X, H - 1 - Y) of
 *              the texture, which is in GL order.  Its source is atlas pixel (sx + i', sy + j') with
 *              i' = RC2DGI_SPRITE_FLIP_X ? w - 1 - i : i and j' = RC2DGI_SPRITE_FLIP_Y ? h - 1 - j : j.  That is 1:1 and
 *              POINT: the library's statement of an unscaled, unrotated DrawTextureRec at an integer position; like
 *              the scaled views of rc2dgi_compose it has not been probed against a GL implementation.  A sprite wholly
 *              off the target draws nothing and is not refused.
 *   Values     `value` is what rc2dgi_write makes of that pixel for the atlas format and the context's storage (its
 *              "Values" paragraph, unchanged).  The tint channel is t = (float)k / 255.0f in F32 and F16 storage and
 *              (float)k * (1.0f / 255.0f) in RGBA8_COMPAT storage (white is exactly 1.0f in both), and
 *              src.c = value.c * t.c, one single multiply a channel, alpha included.  Without RC2DGI_SPRITE_REPLACE the
 *              texel becomes blend(src, texel), the SRC_ALPHA / ONE_MINUS_SRC_ALPHA blend of
 *              rc2dgi_write(.., RC2DGI_WRITE_BLEND) in the context's storage; with it the texel becomes src in float
 *              storage and q8(src) * (1/255) in RGBA8_COMPAT storage.  So a white-tinted sprite that lies inside the
 *              target leaves the bits rc2dgi_write_device leaves for the same sub-image with RC2DGI_WRITE_FLIP (image
 *              row 0 is the top), and with RC2DGI_WRITE_BLEND unless RC2DGI_SPRITE_REPLACE is set.
 *   Draw order the sprites are applied in list order on every texel, across batches too.
 *   Refused    the device cannot fail a call, so a refused sprite draws nothing and is counted in `refused`; the other
 *              sprites are unaffected.  With AW x AH the atlas size, a sprite is refused when
 *                flags & ~7 != 0, or
 *                w < 1, h < 1, sx < 0, sy < 0, w > AW - sx or h > AH - sy (compared in this form), or
 *                dx or dy is outside [-2^22, 2^22].
 *              Nothing read from sprites_dev or count_dev becomes an address, an index or a loop bound before it has
 *              passed this test or that clamp and the sprite's pixel box has been clipped to the target: a buffer of
 *              garbage draws nothing and faults nothing.
 *   Order      the call is enqueued behind whatever is in flight on the context stream and returns; it does not wait
 *              for the stream or the device (the first call of a context allocates the working memory, the one
 *              exception).  The caller keeps the list, the count, the status and the atlas alive until rc2dgi_sync()
 *              and may overwrite the first three on the same stream as soon as the call has returned.  A frame enqueued
 *              before the call sees the old texels, a frame enqueued after it the new ones.  Drawing into COLOR makes
 *              COLOR the input again.  Row-strip shards accept the call: the inputs are replicated whole on every rank.
 *   Memory     the batch capacity and the working bytes are those rc2dgi_paint_device_limits reports: the two calls
 *              share the context's working memory, whichever runs first allocates it, and the stream order separates
 *              them.  A list longer than one batch is drawn batch after batch on the stream (three kernels a batch of
 *              the n given, whatever *count_dev turns out to be).
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in this order, for a null
 * context, a bad `which`, n out of range, a null atlas or atlas->dev or a bad atlas size, format, pitch or alignment, a
 * null sprites_dev with n > 0, a list, count or status pointer not aligned to 4 bytes.  The call only adds an export:
 * RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_atlas {
  const void *dev; /* device image on the context's device, row 0 = the top row */
  int w, h;        /* 1 .. 32768 */
  int pitch_bytes; /* 0 = tight */
  int format;      /* RC2DGI_FMT_RGBA8 | RC2DGI_FMT_RGBA16F | RC2DGI_FMT_RGBA32F */
} rc2dgi_atlas;
typedef struct rc2dgi_sprite {
  int sx, sy, w, h;         /* source rectangle in the atlas, pixels, y down */
  int dx, dy;               /* destination of its top-left pixel, raylib screen coordinates (y down) */
  unsigned char r, g, b, a; /* tint (raylib Color) */
  unsigned flags;           /* RC2DGI_SPRITE_* */
} rc2dgi_sprite;
enum { RC2DGI_SPRITE_FLIP_X = 1, RC2DGI_SPRITE_FLIP_Y = 2, RC2DGI_SPRITE_REPLACE = 4 };
int rc2dgi_sprites_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                          const void *sprites_dev, int n, const void *count_dev, void *status_dev);

/* ---- the same list with every sprite scaled, rotated, sheared or mirrored: the source rectangle is mapped onto a
 * parallelogram of the screen.  (A rotating wall, a swinging door, a spinning light cookie, a zoomed camera -- raylib's
 * DrawTexturePro(texture, source, dest, origin, rotation, tint), the draw DrawTextureRec is built on.)  There is no
 * trigonometry on the device: the producer computes the two edge vectors, as rc2dgi_raycast takes a direction as
 * given.  Everything not restated here is word for word rc2dgi_sprites_device's: `which`, `clear_rgba`, `atlas`,
 * `count_dev`, `status_dev`, m = min(max(*count_dev, 0), n), the "Order" and "Memory" paragraphs (three kernels a
 * batch, the working memory rc2dgi_paint_device_limits reports, shared by the three list calls), the shards, and
 * "drawing into COLOR makes COLOR the input again".
 *   sprites_dev  n records of rc2dgi_sprite_xf (48 bytes, twelve 32-bit words each) on the context's device, aligned to
 *              4 bytes; 0 <= n <= 1 << 20.  n == 0 admits a null sprites_dev.
 *   The record (sx, sy, w, h) is the source rectangle as in rc2dgi_sprite.  Its top-left CORNER (not its first pixel's
 *              centre) lands on P = (px, py), screen pixels, y down; its whole top edge (+u over w pixels) becomes the
 *              vector A = (ax, ay), its whole left edge (+v over h pixels) the vector B = (bx, by).  The destination
 *              is the parallelogram P, P + A, P + A + B, P + B.  Rotation, scale, shear and mirroring are whatever A
 *              and B say; a mirrored sprite is one with a negative determinant.  flags: RC2DGI_SPRITE_REPLACE (4) and
 *              RC2DGI_SPRITE_LINEAR (8); RC2DGI_SPRITE_FLIP_X / _FLIP_Y are not accepted in this record.
 *   Arithmetic every float operation named below is one single fp32 operation, rounded to nearest and not fused
 *              (a * b + c is two roundings); denormals are kept; divisions are IEEE-correct.  A host that restates
 *              the rules in float32 gets the device's bits.
 *   Refused    a refused sprite draws nothing and is counted in `refused`; the others are unaffected.  With AW x AH
 *              the atlas size, a sprite is refused when
 *                flags & ~(4 | 8) != 0, or
 *                w < 1, h < 1, sx < 0, sy < 0, w > AW - sx or h > AH - sy (compared in this form), or
 *                any c of px, py, ax, ay, bx, by fails fabsf(c) <= 0x1p20f (false for a NaN and an infinity), or
 *                det = ax * by - ay * bx (two products, one difference) fails fabsf(det) >= 0x1p-20f.
 *              Nothing read from sprites_dev or count_dev becomes an address, an index or a loop bound before it has
 *              passed this test or the count's clamp: a buffer of garbage draws nothing and faults nothing.
 *   Set-up     i00 = by / det, i01 = (-bx) / det, i10 = (-ay) / det, i11 = ax / det.  The x corners are px, px + ax,
 *              px + bx, (px + ax) + bx, the y corners py, py + ay, py + by, (py + ay) + by; lo / hi are their minimum /
 *              maximum.  The pixel box is X0 = max((int)floorf(lo_x) - 1, 0), X1 = min((int)floorf(hi_x) + 1, W - 1),
 *              and Y0, Y1 alike with H.  (With the bounds above every sum is finite and below 2^22: the conversions
 *              are safe.)  An empty box draws nothing and is not refused.
 *   The box    is part of the contract: only screen pixels X0 <= X <= X1, Y0 <= Y <= Y1 are ever tested.  For an
 *              ill-conditioned sprite (a tiny det against large coordinates) the inverse map cancels badly and the
 *              float test below may pass anywhere; the box confines what such a sprite can touch.
 *   A pixel    for screen pixel (X, Y) of the box, which is texel (X, H - 1 - Y):
 *                dxp = ((float)X + 0.5f) - px, dyp = ((float)Y + 0.5f) - py,
 *                a = dxp * i00 + dyp * i01, b = dxp * i10 + dyp * i11 (two products and one sum each);
 *              the pixel is covered iff a >= 0 && a < 1 && b >= 0 && b < 1 (a NaN fails).  Then
 *                s = a * (float)w, t = b * (float)h.
 *   POINT      (no RC2DGI_SPRITE_LINEAR) the source is atlas pixel (sx + min((int)s, w - 1), sy + min((int)t, h - 1)) and
 *              `value` is what rc2dgi_write makes of it for the atlas format and the context's storage.
 *   LINEAR     xs = s - 0.5f, i0 = (int)floorf(xs), fx = xs - (float)i0, and ys, j0, fy alike from t.  The four taps
 *              are columns clamp(i0, 0, w - 1) and clamp(i0 + 1, 0, w - 1) and rows clamp(j0, 0, h - 1) and
 *              clamp(j0 + 1, 0, h - 1) of the SOURCE RECTANGLE: nothing bleeds in from the atlas neighbours.  Each tap
 *              is first turned into rc2dgi_write's value (in RGBA8_COMPAT storage the quantised k * (1/255)); the
 *              values are lerped in x on both rows, then in y, per channel, with
 *              lerp(p, q, f) = p + f * (q - p): a difference, a product and a sum.  (Not the fused lerp of the GI
 *              textures' LINEAR fetch: no GL implementation is matched here, and an unfused lerp is restated exactly
 *              on a host.)  Like the scaled views of rc2dgi_compose the whole mapping is this library's statement and
 *              has not been probed against a GL implementation.
 *   Values     then as for rc2dgi_sprite: src.c = value.c * t.c with the tint t as defined there per storage, the
 *              blend or RC2DGI_SPRITE_REPLACE exactly as there, the sprites applied in list order on every texel,
 *              across batches too, and a texel stored only if a sprite or the clear touched it.
 *   Consequences (POINT):
 *              A = (w, 0), B = (0, h) and integer px, py leave the bits rc2dgi_sprites_device leaves for
 *              (sx, sy, w, h, dx = px, dy = py);
 *              A = (k * w, 0), B = (0, m * h) with whole k, m draws the sub-image with every pixel repeated k x m;
 *              P = (x + h, y), A = (0, w), B = (-h, 0) is the sub-image turned a quarter clockwise, placed at (x, y);
 *              P = (x + w, y), A = (-w, 0), B = (0, h) equals the RC2DGI_SPRITE_FLIP_X sprite at (x, y), and
 *              P = (x + w, y + h), A = (-w, 0), B = (0, -h) equals RC2DGI_SPRITE_FLIP_X | RC2DGI_SPRITE_FLIP_Y.
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in rc2dgi_sprites_device's
 * order.  The call only adds an export: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_sprite_xf {
  int sx, sy, w, h;         /* source rectangle in the atlas, whole pixels, y down (as rc2dgi_sprite) */
  float px, py;             /* where the source rectangle's top-left CORNER lands, screen pixels, y down */
  float ax, ay;             /* image of the rectangle's whole top edge (+u over w pixels) */
  float bx, by;             /* image of the rectangle's whole left edge (+v over h pixels) */
  unsigned char r, g, b, a; /* tint */
  unsigned flags;           /* RC2DGI_SPRITE_REPLACE (4) | RC2DGI_SPRITE_LINEAR (8) */
} rc2dgi_sprite_xf;         /* 48 bytes, twelve 32-bit words */
enum { RC2DGI_SPRITE_LINEAR = 8 };
int rc2dgi_sprites_xf_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                             const void *sprites_dev, int n, const void *count_dev, void *status_dev);

/* ---- the shapes 2-D level geometry is made of, from a list in device memory: rectangles, circles, triangles, thick
 * lines and ellipses, mixed in one list and painted in list order.  (Walls kept as a tensor of segments, a triangulated
 * polygon soup -- raylib's DrawTriangle, DrawLineEx and DrawEllipse beside DrawRectangleRec and DrawCircleV.  A polyline
 * is its segments as LINEs; the joints are the caller's: a CIRCLE of radius thick / 2 at each.)  Everything not
 * restated here is word for word rc2dgi_paint_device's: `which`, `clear_rgba`, `count_dev`, `status_dev` ({m, refused})
 * and m = min(max(*count_dev, 0), n); the error order; the "Order" paragraph (no wait except the first allocation);
 * the "Memory" paragraph (the same working memory and plan, rc2dgi_paint_device_limits, three kernels a batch, the
 * "paint_plan" knob honoured); the shards; "painting COLOR makes COLOR the input again"; and the guarantee that a
 * buffer of garbage paints nothing and faults nothing.
 *   shapes_dev n records of rc2dgi_shape (32 bytes, eight 32-bit words each) on the context's device, aligned to 4
 *              bytes; 0 <= n <= 1 << 20.  n == 0 admits a null shapes_dev.
 *   Arithmetic every float operation named below is one single fp32 operation, rounded to nearest and not fused
 *              (a * b + c is two roundings); denormals are kept; sqrtf and / are IEEE-correct.  A host that restates
 *              the rules in float32 gets the device's bits.
 *   Kinds      v[] by kind; words not named are not read.
 *     RC2DGI_SHAPE_RECT      v[0..3] = x, y, w, h.
 *     RC2DGI_SHAPE_CIRCLE    v[0..2] = x, y, radius.
 *              Both use rc2dgi_prim's refusal test (lim = 2^22, rc2dgi_paint_device's "Refused"), vertex arithmetic
 *              and triangles, term for term: a list of these two kinds leaves the bits and the `refused` count that
 *              rc2dgi_paint_device leaves for the same primitives.
 *     RC2DGI_SHAPE_TRIANGLE  v = x0, y0, x1, y1, x2, y2: one triangle, drawn whatever its winding (the painter makes
 *              every triangle counter-clockwise; raylib's DrawTriangle asks for counter-clockwise order, and a caller
 *              who wants that culling orders the vertices itself).
 *     RC2DGI_SHAPE_LINE      v = x0, y0, x1, y1, thick; v[5] is not read.  The library's statement of raylib 5.5
 *              DrawLineEx: dx = x1 - x0, dy = y1 - y0, len = sqrtf(dx * dx + dy * dy) (two products, one sum).
 *              Unless len > 0 && thick > 0 the shape draws nothing and is not refused.  Otherwise
 *              scale = thick / (2.0f * len), rx = (-scale) * dy, ry = scale * dx, the corners are
 *              s0 = (x0 - rx, y0 - ry), s1 = (x0 + rx, y0 + ry), s2 = (x1 - rx, y1 - ry), s3 = (x1 + rx, y1 + ry) and the
 *              triangles {s0, s1, s2} and {s1, s2, s3}.
 *     RC2DGI_SHAPE_ELLIPSE   v[0..3] = cx, cy, rh, rv.  The library's statement of DrawEllipse:
 *              T(k) = (cx + c37[k] * rh, cy + s37[k] * rv) with the 37 host cosf / sinf values of DEG2RAD * 10k that
 *              the circles use, and the 36 triangles (c, T(k + 1), T(k)), k = 0 .. 35.  No radius substitution.
 *   Refused    a refused shape draws nothing and is counted in `refused`; the other shapes are unaffected.  RECT and
 *              CIRCLE: as above.  TRIANGLE, LINE, ELLIPSE: every value c the kind reads must pass
 *              fabsf(c) < 0x1p20f (false for a NaN and for an infinity).  Any other `kind` is refused.
 *   Ranges     a LINE's |rx|, |ry| stay below 0.62 * 2^20 (|dy| / len <= sqrt(1.5) even where dy * dy is a denormal
 *              of one bit, and scale stays finite because len >= sqrtf(the least denormal) > 2^-75), so every vertex
 *              of the three kinds lies below 2^21 pixels.  The window transform keeps x and turns y into H - y with
 *              H <= 32768, so a snapped coordinate of theirs is below 2^29 + 2^23 in 1/256 pixel.  An edge's a = -dy
 *              and b = dx are differences of two such numbers, below 2^30 + 2^24: they fit 32 bits.
 *              c = dy * ax - dx * ay is below 2 * 2^30.1 * 2^29.1 < 2^61, and at a pixel centre (|X|, |Y| < 2^23) the
 *              raster's 64-bit sum a * X + b * Y + c is below 2^54 + 2^54 + 2^61 < 2^63.  RECT and CIRCLE keep
 *              rc2dgi_paint's bound and arithmetic.  The binning evaluates the same sums at pixel centres of the
 *              target only, as the raster does.
 *   Vertices to pixels  as rc2dgi_paint: the window transform, the snap to 1/256 pixel, dropping zero-area triangles,
 *              the counter-clockwise swap, the rule for centres exactly on an edge, the clipped pixel box.  A shape
 *              covers a texel when one of its triangles does; it blends over that texel ONCE, in list order, across
 *              batches too.  A shape wholly off the target draws nothing and is not refused.  Like the sprites, the
 *              vertex lists of the three new kinds have not been probed against a GL implementation; the coverage
 *              rule they feed has (the circles' fans, arbitrary slopes).
 *   Binning    a shape is tested only in the 64 x tile_h tiles in which one of its triangles can cover a pixel centre
 *              (an exact test on the integer edge equations); a thin diagonal LINE costs the tiles under it, not the
 *              tiles of its box.  The test only skips tiles in which no centre is covered: it changes no result.
 *   Consequences
 *              a TRIANGLE leaves the same bits for all six orders of its vertices;
 *              the TRIANGLEs (x,y),(x,y+h),(x+w,y+h) and (x,y),(x+w,y+h),(x+w,y) together leave RECT (x, y, w, h)'s
 *              bits for whole-number x, y, w, h, for a translucent colour too: a centre on the shared diagonal belongs
 *              to exactly one of them;
 *              LINE (4, y) -> (36, y) with thick 6 leaves RECT (4, y - 3, 32, 6)'s bits, and so for any length that
 *              is a power of two with whole coordinates;
 *              ELLIPSE with rh == rv == r > 0 leaves CIRCLE (cx, cy, r)'s bits;
 *              an ELLIPSE with a zero radius draws nothing.
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in rc2dgi_paint_device's
 * order.  The call only adds an export: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_shape {
  int kind;                  /* RC2DGI_SHAPE_* */
  float v[6];                /* by kind, above */
  unsigned char r, g, b, a;  /* raylib Color */
} rc2dgi_shape;              /* 32 bytes, eight 32-bit words */
enum { RC2DGI_SHAPE_RECT = 0, RC2DGI_SHAPE_CIRCLE = 1, RC2DGI_SHAPE_TRIANGLE = 2, RC2DGI_SHAPE_LINE = 3,
       RC2DGI_SHAPE_ELLIPSE = 4 };
int rc2dgi_shapes_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const void *shapes_dev, int n,
                         const void *count_dev, void *status_dev);

/* ---- the same five shapes with a colour a vertex and an HDR gain, from a list in device memory: what a 2-D scene is
 * lit with.  (A soft round light, bright at the centre and fading to nothing at the rim -- raylib's DrawCircleGradient;
 * a beam that fades along its length; a wall washed from one colour into another -- DrawRectangleGradientEx / H / V; a
 * triangle with a colour at each vertex.  A particle system kept as a tensor and used as lights.)  Everything not
 * restated here is word for word rc2dgi_shapes_device's, and through it rc2dgi_paint_device's: `which`, `clear_rgba`,
 * `count_dev`, `status_dev` ({m, refused}) and m = min(max(*count_dev, 0), n); the error order; the "Order" paragraph
 * (no wait except the first allocation); the "Memory" paragraph (the same working memory and plan,
 * rc2dgi_paint_device_limits, three kernels a batch, the "paint_plan" knob honoured; the call owns no memory of its
 * own); the "Binning" paragraph; the shards; "painting COLOR makes COLOR the input again"; and the guarantee that a
 * buffer of garbage paints nothing and faults nothing (colour bytes and the gain never become an address).
 *   grads_dev  n records of rc2dgi_gradient (48 bytes, twelve 32-bit words each) on the context's device, aligned to 4
 *              bytes; 0 <= n <= 1 << 20.  n == 0 admits a null grads_dev.  The records are read by the set-up of their
 *              batch alone.
 *   Arithmetic every float operation named below is one single fp32 operation, rounded to nearest and not fused;
 *              denormals are kept and / is IEEE-correct.  (float)E of a 64-bit integer E is one round-to-nearest-even
 *              conversion.  A host that restates the rules in float32 and int64 gets the device's bits.
 *   Geometry   v[] by kind is rc2dgi_shape's v[] of the kind of the same name, and so are the kind's vertex list and
 *              triangles, term for term.  The triangles, in the order in which they are LISTED, vertices in listed order:
 *     RC2DGI_GRAD_RECT      (TL, BL, BR), then (TL, BR, TR).
 *     RC2DGI_GRAD_CIRCLE    (centre, T(k + 1), T(k)), k = 0 .. 35, with the radius substitution.
 *     RC2DGI_GRAD_ELLIPSE   (centre, T(k + 1), T(k)), k = 0 .. 35, without it.
 *     RC2DGI_GRAD_TRIANGLE  its three vertices as given.
 *     RC2DGI_GRAD_LINE      {s0, s1, s2}, then {s1, s2, s3}.
 *              The window transform, the snap to 1/256 pixel, the zero-area drop, the counter-clockwise swap, the
 *              `incl` rule for centres exactly on an edge, the clipped pixel box and the exact tile rejection are
 *              rc2dgi_paint's and rc2dgi_shapes_device's.
 *   Colours by kind   c[k] is a raylib Color, bytes r, g, b, a; bytes not named are not read.
 *     TRIANGLE         c[0..2], one per vertex in order.
 *     RECT             c[0..3] = TL, BL, BR, TR.  This corner order is the library's statement of a two-triangle
 *              gradient quad; the argument order of raylib's DrawRectangleGradientEx differs between raylib versions
 *              (INTEGRATION.md gives the mapping from its argument names).
 *     CIRCLE, ELLIPSE  c[0] at the centre, c[1] at every rim vertex T(k).
 *     LINE             c[0] at s0 and s1 (the (x0, y0) end), c[1] at s2 and s3.
 *              A colour byte k becomes (float)k * (1.0f / 255.0f) in every storage mode (rc2dgi_shapes_device's
 *              conversion).
 *   Which triangle   a texel centre may be covered by more than one triangle of a shape (at a radius near 2^20 the
 *              fan's T(36) and T(0) differ by a fraction of a pixel).  The FIRST covering triangle in the listed order
 *              supplies the colour; dropped triangles are skipped.
 *   Interpolation   let the covering triangle's vertices in listed order be R0, R1, R2 with colours q0, q1, q2.  At the
 *              centre (X, Y) = (256 i + 128, 256 j + 128), E_k is the 64-bit edge function of the edge joining the
 *              other two vertices, oriented so that the inside is positive (the same number whether or not the
 *              triangle was swapped), and A = E_0 + E_1 + E_2 is twice the triangle's area, the same at every centre.
 *              rc2dgi_shapes_device's "Ranges" make each |E| smaller than 2^61 + 2^55, so the sum stays below 2^63
 *              (for RECT and CIRCLE, with rc2dgi_paint's bound: at a covered centre no E is negative and they sum to
 *              twice the area, below 2^62).  Then
 *                w1 = (float)E_1 / (float)A,  w2 = (float)E_2 / (float)A,
 *                col = (q0 + w1 * (q1 - q0)) + w2 * (q2 - q0)   per channel, alpha included: two differences, two
 *                                                               products, two sums, in that order,
 *                src.rgb = col.rgb * gain (one multiply each),  src.a = col.a.
 *   Values     src is treated exactly as rc2dgi_write treats an RGBA32F pixel of that value with RC2DGI_WRITE_BLEND:
 *              in F32 and F16 storage the texel becomes src.c * a + texel.c * (1 - a) with a = src.a; in RGBA8_COMPAT
 *              storage the 8-bit blend of q8(src) over the texel (q8 clamps first, so the gain saturates at 255
 *              there).  A shape blends over a texel ONCE, in list order, across batches too.
 *   Refused    a refused record draws nothing and is counted in `refused`; the others are unaffected.  The geometry test
 *              is that of the rc2dgi_shape kind of the same name (RECT and CIRCLE: rc2dgi_prim's at 2^22; the others:
 *              fabsf(c) < 0x1p20f for every value read).  In addition a record whose gain fails
 *              fabsf(gain) <= 0x1p20f is refused (false for a NaN and for an infinity; a negative gain is accepted).
 *              Any other `kind` is refused.
 *   Consequences
 *              a record whose named colours are all equal and whose gain is 1.0f leaves the bits and the `refused`
 *              count rc2dgi_shapes_device leaves for the shape of the same kind, v[] and colour, in all three storage
 *              modes (every difference q1 - q0 is exactly 0, and q8(k * (1/255)) is k for all 256 values of k);
 *              a centre exactly on an included edge has weight exactly 0 for the opposite vertex;
 *              a CIRCLE with c[1] = {r, g, b, 0} contributes nothing at a centre that lies on the rim edge of its
 *              triangle: there E_0 = 0, so w1 + w2 is 1 but for three roundings each, |col.a| stays below 2^-21, and
 *              in RGBA8_COMPAT storage q8 makes it 0 and the texel keeps its bits; where c[0].a is 0 too, col.a is
 *              exactly 0 and the texel keeps its value in every storage mode.
 *              Like the vertex lists of the three new shape kinds, the interpolation is this library's statement: it
 *              has not been probed against a GL implementation (a GL rasteriser interpolates with plane equations of
 *              its own precision).
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in rc2dgi_paint_device's
 * order.  The call only adds an export and a struct: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_gradient {
  int kind;                 /* RC2DGI_GRAD_* */
  float v[6];               /* geometry by kind, exactly rc2dgi_shape's v[] for the kind of the same name */
  unsigned char c[4][4];    /* up to four raylib Colors (r, g, b, a), by kind */
  float gain;               /* multiplies r, g, b (not alpha) after interpolation: HDR lights */
} rc2dgi_gradient;          /* 48 bytes, twelve 32-bit words */
enum { RC2DGI_GRAD_RECT = 0, RC2DGI_GRAD_CIRCLE = 1, RC2DGI_GRAD_TRIANGLE = 2, RC2DGI_GRAD_LINE = 3,
       RC2DGI_GRAD_ELLIPSE = 4 };
int rc2dgi_gradients_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const void *grads_dev, int n,
                            const void *count_dev, void *status_dev);

/* ---- a tile map: a regular grid of cell words in device memory, each an index into a tile set (an atlas image), drawn
 * as one layer.  (What most 2-D levels are made of: the layers Tiled and LDtk write and every raylib tile-map loader
 * draws with one DrawTextureRec a cell.)  A grid needs none of the list machinery: a pixel's cell is a division of its
 * own coordinates and cells never overlap, so there is no draw order, no batch, no working memory; scrolling is the
 * two integers ox, oy.  `which`, `clear_rgba` and `atlas` are rc2dgi_sprites_device's; `map` is a host struct, read
 * during the call.
 *   The grid   cells_dev is rows x cols 32-bit cell words on the context's device, aligned to 4 bytes, row 0 the TOP
 *              row, the word of cell (c, r) at cells_dev[r * pitch + c] with pitch = pitch_cells, or cols where
 *              pitch_cells == 0 (a window of a larger world is a pointer to its first cell and the world's pitch).
 *              cols and rows are 0 .. 32768; an empty grid (cols * rows == 0) admits a null cells_dev.  Cell (c, r)
 *              covers the screen pixels dx <= X < dx + tile_w, dy <= Y < dy + tile_h with dx = ox + c * tile_w and
 *              dy = oy + r * tile_h (raylib screen coordinates, y down), clipped to the W x H target.
 *   Cell word  Tiled's global tile id as it is: a Tiled layer uploaded as uint32 needs no conversion.  g == 0 is an
 *              empty cell: it draws nothing and is not refused.  Otherwise id = g & 0x0FFFFFFF, t = id - 1,
 *              tx = t % set_cols, ty = t / set_cols; bit 31 flips the tile horizontally and bit 30 vertically
 *              (RC2DGI_SPRITE_FLIP_X / _FLIP_Y of the tile); bits 29 (diagonal) and 28 (hexagonal) are not supported.
 *              The tile's rectangle of the atlas is sx = margin + tx * (tile_w + spacing),
 *              sy = margin + ty * (tile_h + spacing), tile_w x tile_h pixels (Tiled's margin and spacing).
 *   Refused    the device cannot fail a call, so a refused cell draws nothing and is counted; the other cells are
 *              unaffected.  With AW x AH the atlas size, max_tx = (AW - margin - tile_w) / (tile_w + spacing) and
 *              max_ty = (AH - margin - tile_h) / (tile_h + spacing) (computed once on the host, in this form, so
 *              nothing overflows), a non-empty cell is refused when
 *                bit 29 or bit 28 of g is set, or
 *                id == 0 (a word of flag bits alone), or
 *                tx > max_tx or ty > max_ty: the tile's rectangle would not lie in the atlas.
 *   Pixels and values   cell (c, r) is the sprite {sx, sy, tile_w, tile_h, dx, dy, the tint r, g, b, a,
 *              flip bits | (flags & RC2DGI_SPRITE_REPLACE)} of rc2dgi_sprites_device, whose "Pixels" and "Values"
 *              paragraphs apply unchanged: 1:1, POINT, rc2dgi_write's value of the atlas pixel, one multiply a channel
 *              by the tint, and the blend or the replacement in the context's storage.  So after the call the texture
 *              holds the bits rc2dgi_sprites_device leaves for the list of the non-empty, accepted cells that meet
 *              the target, in any order, with the same clear.  (Every such cell has -tile_w < dx < W and
 *              -tile_h < dy < H, so dx and dy are always admissible there.)  With a clear colour every texel that no
 *              such cell covers becomes the clear's value; without one it keeps its bits.
 *   Status     status_dev is NULL or two int32 on the device, aligned to 4 bytes, that receive {drawn, refused} on the
 *              stream on every call.  Both count the VISIBLE cells only, those with at least one pixel inside the
 *              target (a 32768 x 32768 world is not walked for a 1200 x 900 window): `drawn` the visible non-empty
 *              accepted cells, `refused` the visible refused cells.  The sums are integer and independent of order.
 *              With NULL nothing is counted.
 *   Garbage    nothing read from cells_dev becomes an address or an index before the refusal test: the cell index comes
 *              from the pixel's own coordinates, clipped to the grid, the atlas index from a tile the test found inside
 *              the atlas.  A grid of random words draws what the rule accepts and faults nothing.
 *   Order      as rc2dgi_sprites_device: the call is enqueued behind whatever is in flight on the context stream and
 *              returns without waiting (the first call with a status allocates the context's counters, 8 KiB, the one
 *              exception; the painters' working memory is not touched).  Without a clear the work covers only the
 *              map's pixel box clipped to the target; a map scrolled off the target costs nothing and still writes
 *              {0, 0} to a non-null status.  The grid, the atlas and the status stay alive until rc2dgi_sync(); the
 *              grid and the atlas must not overlap the context's textures.  Drawing into COLOR makes COLOR the input
 *              again.  Row-strip shards accept the call: the inputs are replicated whole on every rank.
 * Errors, each leaving the context valid and the texture untouched: RC2DGI_E_ARG, checked in this order, for a null
 * context, a bad `which`, a null atlas or atlas->dev or a bad atlas size, format, pitch or alignment (the checks and the
 * messages of rc2dgi_sprites_device), a null map, flags & ~4, cols or rows out of range, pitch_cells neither 0 nor in
 * cols .. 1 << 20, tile_w or tile_h out of range, ox or oy outside [-2^22, 2^22], set_cols, margin or spacing out of
 * range, margin + tile_w > AW or margin + tile_h > AH (tile 0 does not fit), a null cells_dev with cols * rows > 0,
 * cells_dev or status_dev not aligned to 4 bytes.  The call only adds an export: RC2DGI_ABI_VERSION stays 5. */
typedef struct rc2dgi_tilemap {
  const void *cells_dev;    /* rows x cols 32-bit cell words on the context's device, aligned to 4 bytes, row 0 the TOP row */
  int cols, rows;           /* 0 .. 32768 each; an empty grid admits a null cells_dev */
  int pitch_cells;          /* words from one cell row to the next; 0 = cols; otherwise cols .. 1 << 20 */
  int tile_w, tile_h;       /* 1 .. 32768: a cell's size on the screen and a tile's size in the atlas, pixels */
  int ox, oy;               /* screen position (raylib, y down) of the top-left pixel of cell (0, 0); |.| <= 2^22: the scroll */
  int set_cols;             /* tiles per row of the tile set, 1 .. 32768 */
  int margin, spacing;      /* Tiled's: pixels around the set and between tiles, 0 .. 32768 each */
  unsigned char r, g, b, a; /* tint of the whole layer */
  unsigned flags;           /* RC2DGI_SPRITE_REPLACE (4) or 0 */
} rc2dgi_tilemap;           /* 56 bytes */
int rc2dgi_tilemap_device(rc2dgi_ctx *ctx, int which, const unsigned char *clear_rgba, const rc2dgi_atlas *atlas,
                          const rc2dgi_tilemap *map, void *status_dev);

/* ---- row-strip sharding of one frame over `world` ranks.
 * rc2dgi_set_shard: the context computes screen rows [rank*H/world, (rank+1)*H/world) of the
 * merged colorRT / tempRT and exactly what they depend on (world = 1: the whole frame again).
 * Other rows of its render textures are not meaningful.  Color / emissive inputs are uploaded
 * whole to every rank.  The one exchange is distRT: after phase 1 (ScreenUV, JumpFlood,
 * DistanceField) every rank's distRT strip goes to every other rank, then phase 2 (cascades,
 * blur, merge) runs.  Inside phase 1 the JumpFlood steps compute the own strip only and exchange
 * the rows their taps reach (ring halos for short steps, strip-sized blocks at +-offset for long
 * ones; rc2dgi_plan_jfa_exchange), into strip-sized jumpRT windows.  With strip tables (tuning
 * "strip_tables", square power-of-two screens >= 4096 whose strips fall on the 64 x 64 bound-table cell rows)
 * the exchange after phase 1 is instead row 0 of distRT (to every rank: the REPEAT wrap of the last cell row),
 * then, after each rank's side pass over its own cell rows, its rows of the march field, bound table, hit flags
 * and surface palettes to every rank; distRT then holds the own rows only.  Ways to run a sharded frame:
 *   - rc2dgi_shard_connect: an RCCL communicator owned by the context (one process per GPU,
 *     ranks = shards); rc2dgi_do then runs the frame with the exchange (ncclBroadcast of each
 *     strip, grouped) on the context stream.  rc2dgi_shard_unique_id makes the id on rank 0;
 *     the host passes it to the other ranks.  The transport library is librccl.so.1, opened at the
 *     first of these calls in the process; the environment variable RC2DGI_RCCL_LIB, read once at that
 *     moment, names a library to open instead (it must export the nine nccl* entry points used here;
 *     the tests name a stand-in, tests/fake_rccl.cpp).  A named library that does not load or lacks a
 *     symbol makes these calls return RC2DGI_E_UNSUPPORTED: there is no fallback to librccl.
 *   - rc2dgi_do_group: n contexts of one process, context k = shard k of n (any devices):
 *     phase 1 on each, strips exchanged by device copies, phase 2 on each.
 *   - rc2dgi_do_phase(ctx, 1 | 2) on an unsharded context (world 1) runs the two halves of a
 *     frame; phase 1 of a shard returns RC2DGI_E_STATE (its JumpFlood exchanges between steps).
 * rc2dgi_do on a sharded context without a communicator returns RC2DGI_E_STATE. */
#define RC2DGI_UNIQUE_ID_BYTES 128
int rc2dgi_set_shard(rc2dgi_ctx *ctx, int rank, int world);
int rc2dgi_shard_rows(rc2dgi_ctx *ctx, int *y0, int *y1);
int rc2dgi_shard_unique_id(void *id, int nbytes);
int rc2dgi_shard_connect(rc2dgi_ctx *ctx, const void *id, int nbytes);
int rc2dgi_do_phase(rc2dgi_ctx *ctx, int phase);
int rc2dgi_do_group(rc2dgi_ctx **ctxs, int n);
/* raw device storage of a render texture: float4 texels (COLOR = merged output after a frame,
 * else the input; GI1/GI2/BLUR/TEMP/EMISSIVE), uint16 q (DIST), uint32 packed seeds (JUMP1/2; on
 * a row-strip shard its window: row 0 = global row y0 - m, see rc2dgi_plan_jfa_exchange).  On a row-strip
 * shard TEMP and the merged COLOR hold the shard's own rows only (row 0 = global row y0); so do BLUR and, after a
 * frame, FINAL_GI when the blur runs fused with the merge (power-of-two cascades the size of the screen, a dyadic
 * _BlurRadius below 3, blur_path 0, no LINUX_MERGE flag): the blurred copy-back then stays in a strip-sized texture
 * of its own, and GI1 / GI2 keep the cascade's unblurred level 0 (rc2dgi_download of FINAL_GI / BLUR: the own
 * rows, the others NaN).  With strip tables on top of that (f32, no variant 25, no rc_chain or kept levels) GI1 / GI2
 * are banded: the texture of level L holds, for each of its 2^L block rows in turn, the block-local probe rows the
 * shard computes (one cyclic range per level, rc2dgi_plan_rows), so it is a fraction of CW x CH; rc2dgi_download maps
 * the band back (other rows NaN).  These textures are resized before a frame when the blur settings change. */
int rc2dgi_device_buffer(rc2dgi_ctx *ctx, int which, void **dev, int *pitch_bytes);

/* host-only planner (no device needed): the rows a shard computes for one pass.
 *   pass = RC2DGI_PLAN_JFA + step (screen rows; the last step also writes distRT)
 *        | RC2DGI_PLAN_LEVEL + level (probe rows of every direction block)
 *        | RC2DGI_PLAN_BLUR (cascade rows) | RC2DGI_PLAN_MERGE (screen rows)
 * writes up to max_intervals [begin, end) pairs into `intervals`; returns the count. */
enum { RC2DGI_PLAN_JFA = 0, RC2DGI_PLAN_LEVEL = 1000, RC2DGI_PLAN_BLUR = 2000, RC2DGI_PLAN_MERGE = 2001 };
int rc2dgi_plan_rows(const rc2dgi_config *cfg, float blur_radius, int rank, int world, int pass, int *intervals,
                     int max_intervals);

/* host-only JumpFlood exchange plan of row-strip shards (world >= 2): for JFA step
 * `step` (1 .. S-1, the step that reads J_{step-1}) writes info[9] = {m (halo rows of a window),
 * hmax (tallest strip), mg_max, halo (1 halo step, 0 block step), sh[3] (tap row shifts), mg
 * (rounding margin), same_block} and up to max_xfers transfers of 6 ints {src shard, src window
 * row, rows, dst shard, dst buffer (0 window, 1 block A, 2 block B), dst row}; returns the
 * number of transfers.  A shard's window holds global rows [y0 - m, y1 + m) modulo H. */
int rc2dgi_plan_jfa_exchange(const rc2dgi_config *cfg, int world, int step, int *info, int *xfers, int max_xfers);
/* host-only: the peers shard `rank` awaits (their step step-1 done) before JFA step `step` of a group frame
 * (rc2dgi_do_group): the readers of its J_{step-2} (the ping-pong buffer step `step` overwrites) as their
 * shard index, then the senders of the rows of J_{step-1} it copies as -1 - shard; up to max_peers written,
 * returns the count. */
int rc2dgi_plan_group_waits(const rc2dgi_config *cfg, int world, int rank, int step, int *peers, int max_peers);
/* where shard `rank` reads tap y (dy = -1, 0, +1) of step `step`: buffer buf[y] (0 window, 1 A,
 * 2 B) whose local row 0 is global row row0[y] (modulo H) */
int rc2dgi_plan_jfa_window(const rc2dgi_config *cfg, int rank, int world, int step, int *buf, int *row0);

/* Schedule introspection (no GPU): the RC workgroup order `code` (tuning key rc_order_L<n>:
 * px | py << 8 | dg << 16 | mode << 24 | lc << 26, mode 0 patches, 1 oriented patches, 2 bands along
 * the rays; lc the XCD interleave of rc2dgi_plan_wg_map) over a grid of tiles_x x tiles_y probe tiles of tile_w x tile_h probes and ngrp direction
 * groups.  Writes, for logical workgroups 0..n-1, the probe tile and direction group each one
 * traces; returns 0, or a negative status for bad arguments. */
int rc2dgi_plan_order(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                      int n);
/* The device's workgroup map for the same geometry: for dispatched workgroups 0..n-1 (n = tiles_x * tiles_y *
 * ngrp; the hardware deals them round-robin to the 8 XCDs), the probe tile and direction group each one traces,
 * after the XCD split of the logical order -- each XCD one contiguous eighth of it, or with code bits 26-30
 * = lc > 0 chunks of 2^lc consecutive logical workgroups dealt round-robin to the XCDs. */
int rc2dgi_plan_wg_map(int code, int tiles_x, int tiles_y, int tile_w, int tile_h, int ngrp, int *tiles, int *groups,
                       int n);

#ifdef __cplusplus
}
#endif
#endif /* RC2DGI_H */
