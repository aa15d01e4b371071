/* tone_ref.c -- the semantics of the edge tables (include/rc2dgi.h: "edge tables", "toned views", "histograms of
 * rectangles") restated in plain C for tests/test_tone_cpu.py and tests/test_tone_gpu.py.  Built by the tests with
 * gcc -O1 -ffp-contract=off and loaded with ctypes, as present_ref.c is.
 * Written from the header's prose, literally: bin(v) is a linear scan that counts the edges e[i] <= v -- no binary
 * search, no tree, no early exit -- and the luma is the five operations in the order the header gives.  The toned
 * compositor is the display frame of present_ref.c (the view walk, the decode, the flip, the blend, the border) with
 * the one step the header changes: the 8-bit source of a draw.  A texture is its float download (GL row order) and,
 * for the byte filter of the rgba8 storage, its uint8 download. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* ------------------------------------------------------------------ the primitive */
int tone_bin(const float *e, int m, float v) {
  int n = 0;
  for (int i = 0; i < m; ++i) n += e[i] <= v ? 1 : 0;
  return n;
}

unsigned tone_q8(float x) { return (unsigned)rintf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }

/* T of a view: q8 without a curve, else isnan(v) ? 0 : bin(v) over its 255 edges */
static unsigned tone_T(const float *curve, float v) {
  if (!curve) return tone_q8(v);
  return isnan(v) ? 0u : (unsigned)tone_bin(curve, 255, v);
}

static float bits_float(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

/* bin(v) == q8(v) under the curve, for a v that is no NaN; bin(NaN) is undefined at that level, and a view's T makes
 * it 0 (what q8 makes of a quiet NaN; a signalling one goes through the C library's fmaxf, which is not the table's
 * business) */
static int agrees(const float *curve, float v) {
  if (isnan(v)) return tone_T(curve, v) == 0u;
  return (unsigned)tone_bin(curve, 255, v) == tone_q8(v);
}

/* how many of the `count` bit patterns first, first + stride, .. (modulo 2^32) disagree */
long long tone_sweep(const float *curve, uint32_t first, uint32_t stride, long long count) {
  long long bad = 0;
  uint32_t b = first;
  for (long long i = 0; i < count; ++i, b += stride) bad += !agrees(curve, bits_float(b));
  return bad;
}

/* the same over a list of bit patterns */
long long tone_sweep_list(const float *curve, const uint32_t *bits, long long count) {
  long long bad = 0;
  for (long long i = 0; i < count; ++i) bad += !agrees(curve, bits_float(bits[i]));
  return bad;
}

float tone_luma(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }

/* ------------------------------------------------------------------ toned views */
typedef struct tone_tex {
  const float *f;          /* w * h * 4 floats */
  const unsigned char *b;  /* w * h * 4 bytes, or NULL */
  int w, h;
} tone_tex;

typedef struct tone_view {
  int tex;                   /* index into the texture array */
  int x, y, w, h;            /* window rectangle, y down */
  int filter;                /* 0 POINT, 1 LINEAR on floats, 2 LINEAR on bytes (8.8 fixed point) */
  unsigned char r, g, b, a;  /* border, a == 0: none */
  float exposure;
  int curve;                 /* 0: q8; s: the 255 edges at curves + (s - 1) * 255 */
} tone_view;

static int is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
static unsigned mul8(unsigned x, unsigned y) { return (x * y * 257u + 32768u) >> 16; }

static void blend8(const unsigned s[4], unsigned char *d) {
  const unsigned a8 = s[3];
  for (int c = 0; c < 4; ++c) {
    const unsigned v = mul8(s[c], a8) + mul8(d[c], 255u - a8);
    d[c] = (unsigned char)(v < 255u ? v : 255u);
  }
}

static int wrap_nearest(float u, int n) {
  if (is_pow2(n)) return ((int)floorf(u * (float)n)) & (n - 1);
  const float fr = fminf(u - floorf(u), 0.99999994f);
  const int i = (int)(fr * (float)n);
  return i < n - 1 ? i : n - 1;
}

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

/* the sampled float4 of a view at (u, v) */
static void sample(const tone_tex *t, int filter, float u, float v, float s[4]) {
  if (filter == 0) {
    const float *p = t->f + 4 * ((size_t)wrap_nearest(v, t->h) * t->w + wrap_nearest(u, t->w));
    for (int c = 0; c < 4; ++c) s[c] = p[c];
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
      s[c] = (float)k * (1.0f / 255.0f);
    }
    return;
  }
  for (int c = 0; c < 4; ++c)
    s[c] = lerp_f(lerp_f(t->f[o00 + c], t->f[o10 + c], wx), lerp_f(t->f[o01 + c], t->f[o11 + c], wx), wy);
}

/* out: out_w * out_h * 4 bytes, row 0 = top.  curves: RC2DGI_MAX_CURVES tables of 255 edges.  Returns 0. */
int tone_compose_ref(const tone_tex *tex, const tone_view *views, int n, const float *curves, int out_w, int out_h,
                     const unsigned char *clear, unsigned char *out) {
  for (int py = 0; py < out_h; ++py)
    for (int px = 0; px < out_w; ++px) {
      unsigned char *d = out + 4 * ((size_t)py * out_w + px);
      for (int c = 0; c < 4; ++c) d[c] = clear[c];
      for (int k = 0; k < n; ++k) {
        const tone_view *q = &views[k];
        if (px < q->x || px >= q->x + q->w || py < q->y || py >= q->y + q->h) continue;
        const int i = px - q->x, j = q->h - 1 - (py - q->y);
        const float u = ((float)i + 0.5f) / (float)q->w, v = ((float)j + 0.5f) / (float)q->h;
        float f[4];
        sample(&tex[q->tex], q->filter, u, v, f);
        const float *curve = q->curve ? curves + (size_t)(q->curve - 1) * 255 : NULL;
        unsigned s[4];
        for (int c = 0; c < 3; ++c) {
          const float scaled = f[c] * q->exposure; /* one fp32 multiply */
          s[c] = tone_T(curve, scaled);
        }
        s[3] = tone_q8(f[3]);
        blend8(s, d);
        if (q->a && (px == q->x || px == q->x + q->w - 1 || py == q->y || py == q->y + q->h - 1)) {
          const unsigned bs[4] = {q->r, q->g, q->b, q->a};
          blend8(bs, d);
        }
      }
    }
  return 0;
}

/* ------------------------------------------------------------------ histograms of rectangles */
typedef struct tone_rect { int x, y, w, h; } tone_rect;

/* n rectangles of the tw x th texture `tex` (RGBA floats, GL row order) into counts: record k is m + 4 words
 * {status, texels, nan, bin[0] .. bin[m]} at counts + k * (m + 4).  channel 0 .. 3, or 4 for the luma.  Returns 0. */
int tone_hist_ref(const float *tex, int tw, int th, int channel, const tone_rect *rects, int n, const float *edges, int m,
                  uint32_t *counts) {
  for (int k = 0; k < n; ++k) {
    const tone_rect r = rects[k];
    uint32_t *o = counts + (size_t)k * (size_t)(m + 4);
    memset(o, 0, (size_t)(m + 4) * 4);
    if (!(r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && r.w <= tw - r.x && r.h <= th - r.y)) {
      o[0] = (uint32_t)-1;
      continue;
    }
    o[1] = (uint32_t)(r.w * r.h);
    for (int j = 0; j < r.h; ++j)
      for (int i = 0; i < r.w; ++i) {
        const float *p = tex + (((size_t)r.y + (size_t)j) * (size_t)tw + (size_t)r.x + (size_t)i) * 4;
        const float s = channel == 4 ? tone_luma(p[0], p[1], p[2]) : p[channel];
        if (isnan(s)) o[2] += 1;
        else o[3 + tone_bin(edges, m, s)] += 1;
      }
  }
  return 0;
}
