/* write_ref.c -- rc2dgi_write (include/rc2dgi.h) restated on the host for tests/test_write_cpu.py and
 * tests/test_write_gpu.py: the binary16 -> float32 widening written in integer arithmetic, the two byte conversions,
 * the RGBA8_COMPAT quantization, the float blend, the 8-bit blend, and the placement of an image in a texture given
 * as floats (what rc2dgi_download returns), flipped or not.  Compiled by the tests with gcc -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { FMT_RGBA8 = 0, FMT_RGBA32F = 1, FMT_RGBA16F = 2 };
enum { WRITE_FLIP = 1, WRITE_BLEND = 2 };

/* binary16 bits -> float32 bits, exact: every half is a float */
uint32_t write_widen_bits(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 31u) return sign | 0x7F800000u | (m ? 0x00400000u | (m << 13) : 0u); /* inf; a NaN, made quiet */
  if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);                    /* normal: rebias 15 -> 127 */
  if (m == 0u) return sign;                                                     /* +-0 */
  /* a subnormal half, m * 2^-24: shift the leading one of m up to bit 10, the hidden bit */
  uint32_t mm = m, ee = 113u; /* m * 2^-24 = (m / 2^10) * 2^(113 - 127) */
  while (!(mm & 0x400u)) {
    mm <<= 1;
    --ee;
  }
  return sign | (ee << 23) | ((mm & 0x3FFu) << 13);
}

void write_widen_array(const uint16_t *in, uint32_t *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = write_widen_bits(in[k]);
}

/* a byte in float storage: one IEEE division; in RGBA8_COMPAT storage: one multiply by the float 1/255 */
float write_unorm_div(unsigned k) { return (float)k / 255.0f; }
float write_unorm_mul(unsigned k) { return (float)k * (1.0f / 255.0f); }

void write_unorm_tables(float *div256, float *mul256) {
  for (unsigned k = 0; k < 256u; ++k) {
    div256[k] = write_unorm_div(k);
    mul256[k] = write_unorm_mul(k);
  }
}

/* q8 as rc2dgi_device.h states it: rint(clamp(x, 0, 1) * 255), NaN -> 0 (with comparisons, as tests/read_ref.c) */
unsigned write_q8(float x) {
  if (!(x > 0.0f)) return 0u;
  return (unsigned)rintf((x > 1.0f ? 1.0f : x) * 255.0f);
}

/* a float in RGBA8_COMPAT storage: GiU8::unpack(GiU8::pack(v)) */
float write_quant(float x) { return write_unorm_mul(write_q8(x)); }

void write_quant_array(const float *in, float *out, long long n) {
  for (long long k = 0; k < n; ++k) out[k] = write_quant(in[k]);
}

/* rc2dgi::blend (rc2dgi_device.h): SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels, every operation single and
 * unfused.  volatile keeps each product and the sum a rounded float whatever the compiler would like to do. */
void write_blend_f32(const float *src, const float *dst, float *out) {
  const float a = src[3];
  volatile float ia = 1.0f - a;
  float r[4];
  for (int c = 0; c < 4; ++c) {
    volatile float s = src[c] * a, d = dst[c] * ia;
    r[c] = s + d;
  }
  memcpy(out, r, 16);
}

unsigned write_mul8(unsigned x, unsigned y) { return (x * y * 257u + 32768u) >> 16; }

/* the 8-bit blend of one channel: bytes in, byte out */
unsigned write_blend8(unsigned s8, unsigned a8, unsigned d8) {
  const unsigned v = write_mul8(s8, a8) + write_mul8(d8, 255u - a8);
  return v < 255u ? v : 255u;
}

/* every (s, a, d) for one a: out[s * 256 + d] */
void write_blend8_plane(unsigned a8, unsigned char *out65536) {
  for (unsigned s = 0; s < 256u; ++s)
    for (unsigned d = 0; d < 256u; ++d) out65536[s * 256u + d] = (unsigned char)write_blend8(s, a8, d);
}

/* GiU8::blend (rc2dgi_device.h) */
void write_blend_u8(const float *src, const float *dst, float *out) {
  const unsigned a8 = write_q8(src[3]);
  float r[4];
  for (int c = 0; c < 4; ++c) r[c] = write_unorm_mul(write_blend8(write_q8(src[c]), a8, write_q8(dst[c])));
  memcpy(out, r, 16);
}

/* The image at img (rows of `pitch` bytes, h rows of w pixels of `format`) written into rectangle (x, y, w, h) of tex
 * (th rows of tw RGBA float texels, row 0 = the bottom) in place; u8: the texture's storage is RGBA8_COMPAT.  Returns
 * 0, or -1 for a rectangle that does not lie inside the texture, a bad format, a flag that is not defined or a pitch
 * smaller than a row (nothing is written). */
int write_image_ref(float *tex, int tw, int th, int x, int y, int w, int h, int format, int flags, int u8,
                    const unsigned char *img, long long pitch) {
  if (format != FMT_RGBA8 && format != FMT_RGBA32F && format != FMT_RGBA16F) return -1;
  if (flags & ~(WRITE_FLIP | WRITE_BLEND)) return -1;
  if (!(w >= 1 && h >= 1 && x >= 0 && y >= 0 && w <= tw - x && h <= th - y)) return -1;
  const int pxb = format == FMT_RGBA32F ? 16 : (format == FMT_RGBA16F ? 8 : 4);
  if (pitch < (long long)w * pxb) return -1;
  for (int j = 0; j < h; ++j) {
    const int ty = (flags & WRITE_FLIP) ? y + h - 1 - j : y + j;
    for (int i = 0; i < w; ++i) {
      float *t = tex + ((size_t)ty * (size_t)tw + (size_t)(x + i)) * 4;
      const unsigned char *p = img + (size_t)j * (size_t)pitch + (size_t)i * (size_t)pxb;
      float v[4];
      if (format == FMT_RGBA8) {
        for (int c = 0; c < 4; ++c) v[c] = u8 ? write_unorm_mul(p[c]) : write_unorm_div(p[c]);
      } else {
        if (format == FMT_RGBA32F) {
          memcpy(v, p, 16);
        } else {
          for (int c = 0; c < 4; ++c) {
            uint16_t hb;
            memcpy(&hb, p + 2 * c, 2);
            const uint32_t wb = write_widen_bits(hb);
            memcpy(&v[c], &wb, 4);
          }
        }
        if (u8)
          for (int c = 0; c < 4; ++c) v[c] = write_quant(v[c]);
      }
      if (flags & WRITE_BLEND) {
        if (u8) write_blend_u8(v, t, t);
        else write_blend_f32(v, t, t);
      } else {
        memcpy(t, v, 16);
      }
    }
  }
  return 0;
}
