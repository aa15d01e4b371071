/* reduce_ref.c -- the semantics of rc2dgi_reduce (include/rc2dgi.h, "region statistics") restated in plain C for
 * tests/test_reduce_gpu.py and tests/test_reduce_cpu.py, over a texture as rc2dgi_download returns it: tw x th RGBA
 * floats, row j of the array being texel row j (GL order).  Built by the tests with gcc -O1 -ffp-contract=off and
 * loaded with ctypes.
 * Written from the header's prose, literally: a row's leaves are laid out in an array of P doubles, the padding
 * +0.0, and halved level by level, s[i] = s[2i] + s[2i+1]; the row sums go through the same routine.  No skipped
 * padding, no stack, no swapped operands: the structure owes nothing to the kernels. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct ref_rect { int x, y, w, h; } ref_rect;
typedef struct ref_stats {
  int status, texels;
  int nonfinite[4];
  float min[4], max[4];
  double sum[4];
} ref_stats;

_Static_assert(sizeof(ref_rect) == 16 && sizeof(ref_stats) == 88, "the records are 16 and 88 bytes");

static size_t pow2_at_least(size_t n) {
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

/* the adjacent-pair tree over s[0 .. p), p a power of two; destroys s */
static double pair_tree(double *s, size_t p) {
  for (; p > 1; p >>= 1)
    for (size_t i = 0; i < p / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
  return s[0];
}

static int finite_bits(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return (b & 0x7F800000u) != 0x7F800000u;
}

/* n rectangles of the tw x th texture `tex` into out[0 .. n).  Returns 0, or -1 when memory runs out. */
int reduce_ref(const float *tex, int tw, int th, const ref_rect *rects, int n, ref_stats *out) {
  for (int k = 0; k < n; ++k) {
    const ref_rect r = rects[k];
    ref_stats *o = out + k;
    memset(o, 0, sizeof *o);
    if (!(r.w >= 1 && r.h >= 1 && r.x >= 0 && r.y >= 0 && r.w <= tw - r.x && r.h <= th - r.y)) {
      o->status = -1;
      continue;
    }
    o->texels = r.w * r.h;
    const size_t pw = pow2_at_least((size_t)r.w), ph = pow2_at_least((size_t)r.h);
    double *row = malloc(pw * sizeof(double)), *col = malloc(ph * sizeof(double));
    if (!row || !col) {
      free(row);
      free(col);
      return -1;
    }
    for (int c = 0; c < 4; ++c) {
      o->min[c] = INFINITY;
      o->max[c] = -INFINITY;
      for (size_t j = 0; j < ph; ++j) {
        if (j >= (size_t)r.h) {
          col[j] = 0.0;
          continue;
        }
        for (size_t i = 0; i < pw; ++i) {
          row[i] = 0.0;
          if (i >= (size_t)r.w) continue;
          const float v = tex[(((size_t)r.y + j) * (size_t)tw + (size_t)r.x + i) * 4 + (size_t)c] + 0.0f;
          if (!finite_bits(v)) {
            o->nonfinite[c] += 1;
            continue;
          }
          row[i] = (double)v;
          if (v < o->min[c]) o->min[c] = v;
          if (v > o->max[c]) o->max[c] = v;
        }
        col[j] = pair_tree(row, pw);
      }
      o->sum[c] = pair_tree(col, ph);
    }
    free(row);
    free(col);
  }
  return 0;
}
