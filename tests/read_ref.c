/* read_ref.c -- rc2dgi_read (include/rc2dgi.h) restated on the host for tests/test_read_cpu.py and
 * tests/test_read_gpu.py: the crop of a texture given as floats (what rc2dgi_download returns), the flip, q8, and the
 * float32 -> binary16 conversion with round to nearest even written in integer arithmetic.  Compiled by the tests
 * with gcc -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { FMT_RGBA8 = 0, FMT_RGBA32F = 1, FMT_RGBA16F = 2 };

/* float32 bits -> binary16 bits, round to nearest, ties to even */
uint16_t read_half_bits(uint32_t u) {
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u); /* a NaN (the payload is not part of the contract) */
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u); /* 65520 = the midpoint of 65504 and 2^16, and up: inf */
  if (a >= 0x38800000u) {                                  /* 2^-14 and up: a normal half */
    const uint32_t v = a - 0x38000000u;                    /* exponent rebiased from 127 to 15 */
    return (uint16_t)(sign | ((v + 0x0FFFu + ((v >> 13) & 1u)) >> 13)); /* (a carry into the exponent is right) */
  }
  if (a < 0x33000000u) return (uint16_t)sign; /* below 2^-25, float subnormals included: zero */
  /* a subnormal half, k * 2^-24: k = m * 2^(e - 126) rounded, with m the 24-bit significand and e = 102 .. 112 */
  const uint32_t e = a >> 23, m = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e; /* 14 .. 24 */
  uint32_t k = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
  if (rem > halfway || (rem == halfway && (k & 1u))) ++k; /* (1024 is 0x0400, the smallest normal half) */
  return (uint16_t)(sign | k);
}

uint16_t read_half(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return read_half_bits(u);
}

void read_half_array(const float *in, uint16_t *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = read_half(in[k]);
}

/* q8 as rc2dgi_device.h states it: rint(clamp(x, 0, 1) * 255), NaN -> 0.  The clamp is written with comparisons: the
 * C library's fmaxf answers a NaN for a signalling NaN, where the rule is 0 for every NaN. */
unsigned read_q8(float x) {
  if (!(x > 0.0f)) return 0u; /* a NaN compares false */
  return (unsigned)rintf((x > 1.0f ? 1.0f : x) * 255.0f);
}

void read_q8_array(const float *in, unsigned char *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = (unsigned char)read_q8(in[k]);
}

/* The image of rectangle (x, y, w, h) of tex (th rows of tw RGBA float texels, row 0 = the bottom) into out, rows of
 * `pitch` bytes: only the bytes of the w pixels of each of the h rows are written.  Returns 0, or -1 for a rectangle
 * that does not lie inside the texture, a bad format or a pitch smaller than a row (nothing is written). */
int read_image_ref(const float *tex, int tw, int th, int x, int y, int w, int h, int format, int flip,
                   unsigned char *out, long long pitch) {
  if (!(w >= 1 && h >= 1 && x >= 0 && y >= 0 && w <= tw - x && h <= th - y)) return -1;
  if (format != FMT_RGBA8 && format != FMT_RGBA32F && format != FMT_RGBA16F) return -1;
  const int pxb = format == FMT_RGBA32F ? 16 : (format == FMT_RGBA16F ? 8 : 4);
  if (pitch < (long long)w * pxb) return -1;
  for (int j = 0; j < h; ++j) {
    const int ty = flip ? y + h - 1 - j : y + j;
    for (int i = 0; i < w; ++i) {
      const float *p = tex + ((size_t)ty * (size_t)tw + (size_t)(x + i)) * 4;
      unsigned char *o = out + (size_t)j * (size_t)pitch + (size_t)i * (size_t)pxb;
      if (format == FMT_RGBA32F) {
        memcpy(o, p, 16);
      } else if (format == FMT_RGBA16F) {
        for (int c = 0; c < 4; ++c) {
          const uint16_t hb = read_half(p[c]);
          memcpy(o + 2 * c, &hb, 2);
        }
      } else {
        for (int c = 0; c < 4; ++c) o[c] = (unsigned char)read_q8(p[c]);
      }
    }
  }
  return 0;
}
