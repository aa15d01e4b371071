/* query_ref.c -- the semantics of rc2dgi_sample and rc2dgi_raycast (include/rc2dgi.h, "queries") restated in plain C
 * for tests/test_query_gpu.py and tests/test_query_cpu.py, over the textures as rc2dgi_download returns them.  Built
 * by the tests with gcc -O1 -ffp-contract=off and loaded with ctypes; the LINEAR lerp is libm's fmaf (one rounding).
 * Written from the header's prose: the structure (the NaN rule, the step rules in their order, what each output field
 * holds) owes nothing to the kernels.  The wrap and weight arithmetic is the one the header names, so those few
 * expressions read as tests/present_ref.c states them.
 *
 * A texture is its float download (GL row order: row j of the array is texel row j) and, for the byte filter of the
 * rgba8 storage, its uint8 download.  distRT is its uint8 download: q = hi << 8 | lo. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

static int is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

/* NEAREST + REPEAT */
static int wrap_nearest(float u, int n) {
  if (is_pow2(n)) return ((int)floorf(u * (float)n)) & (n - 1);
  const float fr = fminf(u - floorf(u), 0.99999994f);
  const int i = (int)(fr * (float)n);
  return i < n - 1 ? i : n - 1;
}

/* LINEAR + REPEAT: taps and weight along one axis */
static void wrap_linear(float u, int n, int *i0, int *i1, float *w) {
  const float x = is_pow2(n) ? u * (float)n - 0.5f : (u - floorf(u)) * (float)n - 0.5f;
  const float fl = floorf(x);
  *w = x - fl;
  const int t0 = (int)fl, t1 = t0 + 1;
  if (is_pow2(n)) {
    *i0 = t0 & (n - 1);
    *i1 = t1 & (n - 1);
  } else {
    *i0 = t0 < 0 ? t0 + n : (t0 >= n ? t0 - n : t0);
    *i1 = t1 < 0 ? t1 + n : (t1 >= n ? t1 - n : t1);
  }
}

static float lerp_f(float a, float b, float w) { return fmaf(w, b - a, a); }
static unsigned lerp_b(unsigned a, unsigned b, int w) {
  return (unsigned)((int)(a * 256u) + ((int)b - (int)a) * w + 128) >> 8;
}

/* filter: 0 POINT, 1 LINEAR on floats, 2 LINEAR on bytes (8.8 fixed point).  f: w * h * 4 floats; b: w * h * 4 bytes
 * (filter 2 only).  uv: n * 2 floats in, rgba: n * 4 floats out.  Returns 0. */
int query_ref_sample(const float *f, const unsigned char *b, int w, int h, int filter, const float *uv, int n,
                     float *rgba) {
  for (int k = 0; k < n; ++k) {
    const float u = uv[2 * k], v = uv[2 * k + 1];
    float *o = rgba + 4 * (size_t)k;
    if (!isfinite(u) || !isfinite(v)) {
      const uint32_t qnan = 0x7FC00000u;
      for (int c = 0; c < 4; ++c) memcpy(o + c, &qnan, 4);
      continue;
    }
    if (filter == 0) {
      memcpy(o, f + 4 * ((size_t)wrap_nearest(v, h) * w + wrap_nearest(u, w)), 16);
      continue;
    }
    int x0, x1, y0, y1;
    float wx, wy;
    wrap_linear(u, w, &x0, &x1, &wx);
    wrap_linear(v, h, &y0, &y1, &wy);
    const size_t o00 = 4 * ((size_t)y0 * w + x0), o10 = 4 * ((size_t)y0 * w + x1);
    const size_t o01 = 4 * ((size_t)y1 * w + x0), o11 = 4 * ((size_t)y1 * w + x1);
    for (int c = 0; c < 4; ++c) {
      if (filter == 2) {
        const int w8x = (int)rintf(wx * 256.0f), w8y = (int)rintf(wy * 256.0f);
        const unsigned q = lerp_b(lerp_b(b[o00 + c], b[o10 + c], w8x), lerp_b(b[o01 + c], b[o11 + c], w8x), w8y);
        o[c] = (float)q * (1.0f / 255.0f);
      } else {
        o[c] = lerp_f(lerp_f(f[o00 + c], f[o10 + c], wx), lerp_f(f[o01 + c], f[o11 + c], wx), wy);
      }
    }
  }
  return 0;
}

typedef struct ref_ray { float ox, oy, dx, dy, t0, t1; } ref_ray;
typedef struct ref_hit { int status, steps, ix, iy; float t, u, v, r, g, b, a; } ref_hit;
enum { INVALID = -1, RANGE = 0, EDGE = 1, EMISSIVE = 2, SURFACE = 3, STEPS = 4 };

static int field_ok(float x) { return isfinite(x) && fabsf(x) <= 1048576.0f; }

/* dist8: the RGBA8 download of distRT (W * H * 4 bytes); color, emissive: the painted inputs (W * H * 4 floats).
 * Returns 0. */
int query_ref_raycast(const unsigned char *dist8, const float *color, const float *emissive, int W, int H,
                      float reflectivity, const ref_ray *rays, int n, ref_hit *hits) {
  const float mx = (float)(W > H ? W : H);
  const float aspx = (float)W / mx, aspy = (float)H / mx;
  for (int k = 0; k < n; ++k) {
    const ref_ray r = rays[k];
    ref_hit *o = &hits[k];
    memset(o, 0, sizeof *o);
    o->ix = o->iy = -1;
    if (!field_ok(r.ox) || !field_ok(r.oy) || !field_ok(r.dx) || !field_ok(r.dy) || !field_ok(r.t0) ||
        !field_ok(r.t1)) {
      o->status = INVALID;
      continue;
    }
    o->a = 1.0f; /* the shader's initial hit, (0, 0, 0, 1) */
    o->status = STEPS;
    float t = r.t0;
    while (o->steps < 32) {
      const float sx = t * r.dx, sy = t * r.dy; /* each operation on its own */
      const float mxs = sx * aspy, mys = sy * aspx;
      o->u = r.ox + mxs;
      o->v = r.oy + mys;
      if (t > r.t1) {
        o->status = RANGE;
        break;
      }
      if (o->u < 0.0f || o->v < 0.0f || o->u > 1.0f || o->v > 1.0f) {
        o->status = EDGE;
        break;
      }
      const int ix = wrap_nearest(o->u, W), iy = wrap_nearest(o->v, H);
      const size_t at = (size_t)iy * W + ix;
      const unsigned q = ((unsigned)dist8[4 * at] << 8) | dist8[4 * at + 1];
      const float d = (float)q / 65535.0f;
      o->steps++;
      if (d < 0.001f) {
        const float *e = emissive + 4 * at;
        o->ix = ix;
        o->iy = iy;
        const float xx = e[0] * e[0], yy = e[1] * e[1], zz = e[2] * e[2];
        if (sqrtf((xx + yy) + zz) > 0.0f) {
          o->status = EMISSIVE;
          o->r = e[0]; o->g = e[1]; o->b = e[2]; o->a = 1.0f;
        } else {
          o->status = SURFACE;
          o->r = color[4 * at]; o->g = color[4 * at + 1]; o->b = color[4 * at + 2]; o->a = reflectivity;
        }
        break;
      }
      t += d;
    }
    o->t = t;
  }
  return 0;
}
