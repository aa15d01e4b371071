/* present_ref.c -- the display frame's semantics (include/rc2dgi.h, "the display frame") restated in
 * plain C for tests/test_present_gpu.py: the textures as rc2dgi_download returns them, plus a view list, give the
 * RGBA8 window.  Built by the test with gcc -O1 -ffp-contract=off and loaded with ctypes; the LINEAR lerp is libm's
 * fmaf (one rounding).  Written from the header's prose: the structure (view walk, decode, flip, blend order, border)
 * owes nothing to the kernel.  The wrap and weight arithmetic (wrap_nearest, wrap_linear, the 8.8 lerp) is the one
 * the semantics name, so those few expressions read as rc2dgi_device.h states them.
 *
 * A texture is its float download (GL row order: row j of the array is texel row j) and, for the byte filter of the
 * rgba8 storage, its uint8 download. */
#include <math.h>
#include <stddef.h>

typedef struct present_tex {
  const float *f;          /* w * h * 4 floats */
  const unsigned char *b;  /* w * h * 4 bytes, or NULL */
  int w, h;
} present_tex;

typedef struct present_view {
  int tex;                   /* index into the texture array */
  int x, y, w, h;            /* window rectangle, y down */
  int filter;                /* 0 POINT, 1 LINEAR on floats, 2 LINEAR on bytes (8.8 fixed point) */
  unsigned char r, g, b, a;  /* border, a == 0: none */
} present_view;

static int is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

static unsigned q8(float x) { return (unsigned)rintf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }
static unsigned mul8(unsigned x, unsigned y) { return (x * y * 257u + 32768u) >> 16; }

/* one draw: the four source bytes s over the framebuffer pixel d */
static void blend8(const unsigned s[4], unsigned char *d) {
  const unsigned a8 = s[3];
  for (int c = 0; c < 4; ++c) {
    const unsigned v = mul8(s[c], a8) + mul8(d[c], 255u - a8);
    d[c] = (unsigned char)(v < 255u ? v : 255u);
  }
}

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

static void sample(const present_tex *t, int filter, float u, float v, unsigned s[4]) {
  if (filter == 0) {
    const float *p = t->f + 4 * ((size_t)wrap_nearest(v, t->h) * t->w + wrap_nearest(u, t->w));
    for (int c = 0; c < 4; ++c) s[c] = q8(p[c]);
    return;
  }
  int x0, x1, y0, y1;
  float wx, wy;
  wrap_linear(u, t->w, &x0, &x1, &wx);
  wrap_linear(v, t->h, &y0, &y1, &wy);
  const size_t o00 = 4 * ((size_t)y0 * t->w + x0), o10 = 4 * ((size_t)y0 * t->w + x1);
  const size_t o01 = 4 * ((size_t)y1 * t->w + x0), o11 = 4 * ((size_t)y1 * t->w + x1);
  if (filter == 2) {
    const int w8x = (int)rintf(wx * 256.0f), w8y = (int)rintf(wy * 256.0f);
    for (int c = 0; c < 4; ++c) {
      const unsigned k = lerp_b(lerp_b(t->b[o00 + c], t->b[o10 + c], w8x), lerp_b(t->b[o01 + c], t->b[o11 + c], w8x), w8y);
      s[c] = q8((float)k * (1.0f / 255.0f));
    }
    return;
  }
  for (int c = 0; c < 4; ++c)
    s[c] = q8(lerp_f(lerp_f(t->f[o00 + c], t->f[o10 + c], wx), lerp_f(t->f[o01 + c], t->f[o11 + c], wx), wy));
}

/* out: out_w * out_h * 4 bytes, row 0 = top.  Returns 0. */
int present_ref(const present_tex *tex, const present_view *views, int n, int out_w, int out_h,
                const unsigned char *clear, unsigned char *out) {
  for (int py = 0; py < out_h; ++py)
    for (int px = 0; px < out_w; ++px) {
      unsigned char *d = out + 4 * ((size_t)py * out_w + px);
      for (int c = 0; c < 4; ++c) d[c] = clear[c];
      for (int k = 0; k < n; ++k) {
        const present_view *q = &views[k];
        if (px < q->x || px >= q->x + q->w || py < q->y || py >= q->y + q->h) continue;
        const int i = px - q->x, j = q->h - 1 - (py - q->y);
        const float u = ((float)i + 0.5f) / (float)q->w, v = ((float)j + 0.5f) / (float)q->h;
        unsigned s[4];
        sample(&tex[q->tex], q->filter, u, v, s);
        blend8(s, d);
        if (q->a && (px == q->x || px == q->x + q->w - 1 || py == q->y || py == q->y + q->h - 1)) {
          const unsigned bs[4] = {q->r, q->g, q->b, q->a};
          blend8(bs, d);
        }
      }
    }
  return 0;
}
