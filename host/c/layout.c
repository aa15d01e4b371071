/* layout.c -- sizeof / offsetof of the ABI structs, as the C compiler lays them out, for
 * tests/test_host_cpu.py to compare with the C# StructLayout(Sequential) mirrors in
 * host/csharp/RC2DGINative.cs (Config, Prim; View: tests/test_present_cpu.py; Ray, RayHit: tests/test_query_cpu.py;
 * Rect, Stats: tests/test_reduce_cpu.py; Tone: tests/test_tone_cpu.py; Atlas, Sprite: tests/test_sprites_cpu.py;
 * SpriteXf: tests/test_sprites_xf_cpu.py; Shape: tests/test_shapes_cpu.py;
 * Gradient: tests/test_gradients_cpu.py). */
#include <stddef.h>
#include <stdio.h>

#include "rc2dgi.h"

#define F(S, m) printf("%s.%s %zu %zu\n", #S, #m, offsetof(S, m), sizeof(((S *)0)->m))

int main(void) {
  printf("rc2dgi_config %zu\n", sizeof(rc2dgi_config));
  F(rc2dgi_config, screen_width);
  F(rc2dgi_config, screen_height);
  F(rc2dgi_config, cascade_count);
  F(rc2dgi_config, render_scale);
  F(rc2dgi_config, ray_range);
  F(rc2dgi_config, storage);
  F(rc2dgi_config, device);
  F(rc2dgi_config, flags);
  F(rc2dgi_config, reserved);
  printf("rc2dgi_prim %zu\n", sizeof(rc2dgi_prim));
  F(rc2dgi_prim, kind);
  F(rc2dgi_prim, x);
  F(rc2dgi_prim, y);
  F(rc2dgi_prim, w);
  F(rc2dgi_prim, h);
  F(rc2dgi_prim, r);
  F(rc2dgi_prim, g);
  F(rc2dgi_prim, b);
  F(rc2dgi_prim, a);
  printf("rc2dgi_view %zu\n", sizeof(rc2dgi_view));
  F(rc2dgi_view, which);
  F(rc2dgi_view, x);
  F(rc2dgi_view, y);
  F(rc2dgi_view, w);
  F(rc2dgi_view, h);
  F(rc2dgi_view, filter);
  F(rc2dgi_view, r);
  F(rc2dgi_view, g);
  F(rc2dgi_view, b);
  F(rc2dgi_view, a);
  printf("rc2dgi_ray %zu\n", sizeof(rc2dgi_ray));
  F(rc2dgi_ray, ox);
  F(rc2dgi_ray, oy);
  F(rc2dgi_ray, dx);
  F(rc2dgi_ray, dy);
  F(rc2dgi_ray, t0);
  F(rc2dgi_ray, t1);
  printf("rc2dgi_rayhit %zu\n", sizeof(rc2dgi_rayhit));
  F(rc2dgi_rayhit, status);
  F(rc2dgi_rayhit, steps);
  F(rc2dgi_rayhit, ix);
  F(rc2dgi_rayhit, iy);
  F(rc2dgi_rayhit, t);
  F(rc2dgi_rayhit, u);
  F(rc2dgi_rayhit, v);
  F(rc2dgi_rayhit, r);
  F(rc2dgi_rayhit, g);
  F(rc2dgi_rayhit, b);
  F(rc2dgi_rayhit, a);
  printf("rc2dgi_rect %zu\n", sizeof(rc2dgi_rect));
  F(rc2dgi_rect, x);
  F(rc2dgi_rect, y);
  F(rc2dgi_rect, w);
  F(rc2dgi_rect, h);
  printf("rc2dgi_stats %zu\n", sizeof(rc2dgi_stats));
  F(rc2dgi_stats, status);
  F(rc2dgi_stats, texels);
  F(rc2dgi_stats, nonfinite);
  F(rc2dgi_stats, min);
  F(rc2dgi_stats, max);
  F(rc2dgi_stats, sum);
  printf("rc2dgi_tone %zu\n", sizeof(rc2dgi_tone));
  F(rc2dgi_tone, exposure);
  F(rc2dgi_tone, curve);
  printf("rc2dgi_atlas %zu\n", sizeof(rc2dgi_atlas));
  F(rc2dgi_atlas, dev);
  F(rc2dgi_atlas, w);
  F(rc2dgi_atlas, h);
  F(rc2dgi_atlas, pitch_bytes);
  F(rc2dgi_atlas, format);
  printf("rc2dgi_sprite %zu\n", sizeof(rc2dgi_sprite));
  F(rc2dgi_sprite, sx);
  F(rc2dgi_sprite, sy);
  F(rc2dgi_sprite, w);
  F(rc2dgi_sprite, h);
  F(rc2dgi_sprite, dx);
  F(rc2dgi_sprite, dy);
  F(rc2dgi_sprite, r);
  F(rc2dgi_sprite, g);
  F(rc2dgi_sprite, b);
  F(rc2dgi_sprite, a);
  F(rc2dgi_sprite, flags);
  printf("rc2dgi_sprite_xf %zu\n", sizeof(rc2dgi_sprite_xf));
  F(rc2dgi_sprite_xf, sx);
  F(rc2dgi_sprite_xf, sy);
  F(rc2dgi_sprite_xf, w);
  F(rc2dgi_sprite_xf, h);
  F(rc2dgi_sprite_xf, px);
  F(rc2dgi_sprite_xf, py);
  F(rc2dgi_sprite_xf, ax);
  F(rc2dgi_sprite_xf, ay);
  F(rc2dgi_sprite_xf, bx);
  F(rc2dgi_sprite_xf, by);
  F(rc2dgi_sprite_xf, r);
  F(rc2dgi_sprite_xf, g);
  F(rc2dgi_sprite_xf, b);
  F(rc2dgi_sprite_xf, a);
  F(rc2dgi_sprite_xf, flags);
  printf("rc2dgi_shape %zu\n", sizeof(rc2dgi_shape));
  F(rc2dgi_shape, kind);
  F(rc2dgi_shape, v);
  F(rc2dgi_shape, r);
  F(rc2dgi_shape, g);
  F(rc2dgi_shape, b);
  F(rc2dgi_shape, a);
  printf("rc2dgi_gradient %zu\n", sizeof(rc2dgi_gradient));
  F(rc2dgi_gradient, kind);
  F(rc2dgi_gradient, v);
  F(rc2dgi_gradient, c);
  F(rc2dgi_gradient, gain);
  return 0;
}
