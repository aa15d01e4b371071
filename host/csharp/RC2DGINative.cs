// RC2DGINative.cs -- P/Invoke binding of librc2dgi.so (include/rc2dgi.h) for the reference's
// C# host (RC2DGI.cs).  Drop this file next to RC2DGI.cs and apply the patch shown in
// INTEGRATION.md: DoRC2DGI() (RC2DGI.cs:267-406) becomes one native call, the uniform
// globals keep their names, and the debug thumbnails (RC2DGI.cs:156-163) are refreshed
// from the native render textures.
//
// Not compiled in this repository (no .NET SDK in the build image); the C ABI it binds is
// exercised by tests/ through the same entry points.
using System;
using System.Runtime.InteropServices;
using Raylib_cs;

static unsafe class RC2DGINative
{
    const string Lib = "rc2dgi"; // librc2dgi.so / rc2dgi.dll on the loader path

    public const int OK = 0;
    public enum RT { Color = 0, Emissive = 1, Jump1 = 2, Jump2 = 3, Dist = 4, GI1 = 5, GI2 = 6, Temp = 7, Blur = 8, FinalGI = 9 }
    public enum Format { RGBA8 = 0, RGBA32F = 1, RGBA16F = 2 }  // RGBA16F: rc2dgi_read* and rc2dgi_write* only
    public enum Storage { F32 = 0, RGBA8Compat = 1, F16 = 2 }  // RGBA8Compat: the shipped app's RGBA8 textures, byte-exact

    [StructLayout(LayoutKind.Sequential)]
    public struct Config
    {
        public int ScreenWidth, ScreenHeight, CascadeCount;
        public float RenderScale, RayRange;
        public int Storage, Device;
        public int Flags;              // 1 = Linux merge fallback (Merge.fs not found, RC2DGI.cs:62)
        public int R0, R1, R2, R3;     // reserved, zero
    }

    [DllImport(Lib)] public static extern int rc2dgi_create(ref Config cfg, out IntPtr ctx);
    [DllImport(Lib)] public static extern int rc2dgi_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern int rc2dgi_set_uniform(IntPtr ctx, [MarshalAs(UnmanagedType.LPUTF8Str)] string name, float* v, int n);
    [DllImport(Lib)] public static extern int rc2dgi_set_uniform_i(IntPtr ctx, [MarshalAs(UnmanagedType.LPUTF8Str)] string name, int v);
    [DllImport(Lib)] public static extern int rc2dgi_upload(IntPtr ctx, int which, void* host, int pitchBytes, int format);
    [DllImport(Lib)] public static extern int rc2dgi_do(IntPtr ctx);
    [DllImport(Lib)] public static extern int rc2dgi_sync(IntPtr ctx);
    [DllImport(Lib)] public static extern int rc2dgi_download(IntPtr ctx, int which, void* host, int pitchBytes, int format);
    [DllImport(Lib)] public static extern int rc2dgi_query(IntPtr ctx, out int cw, out int ch, out int jfaSteps, out int finalGi);
    [DllImport(Lib)] public static extern IntPtr rc2dgi_last_error(IntPtr ctx);

    // rc2dgi_prim: DrawRectangleRec (Kind 0) / DrawCircleV (Kind 1, W = radius), raylib screen coordinates
    [StructLayout(LayoutKind.Sequential)]
    public struct Prim
    {
        public int Kind;
        public float X, Y, W, H;
        public byte R, G, B, A;
    }
    [DllImport(Lib)] public static extern int rc2dgi_paint(IntPtr ctx, int which, byte* clearRgba, Prim* prims, int n);
    // The same painting from n Prim records in device memory (primsDev, aligned to 4 bytes; n up to 1 << 20), enqueued on
    // the context stream: nothing waits.  countDev: null, or one int on the device read when the work runs -- min(max(count,
    // 0), n) primitives are painted.  statusDev: null, or two ints that receive {painted, refused}: a primitive rc2dgi_paint
    // would refuse draws nothing and is counted.  rc2dgi_paint_device_limits (host-only): the primitives of one batch and
    // the bytes of working memory the context allocates at the first call, for a config.
    [DllImport(Lib)] public static extern int rc2dgi_paint_device(IntPtr ctx, int which, byte* clearRgba, void* primsDev, int n, void* countDev, void* statusDev);
    [DllImport(Lib)] public static extern int rc2dgi_paint_device_limits(ref Config cfg, out int batchPrims, out long workBytes);

    // rc2dgi_sprites_device: n Sprite records in device memory, each the rectangle (Sx, Sy, W, H) of one atlas image
    // (a device image whose row 0 is the top row) drawn 1:1 with its top-left pixel at (Dx, Dy), raylib screen
    // coordinates -- DrawTextureRec at an integer position -- tinted and blended over the texels (SpriteReplace:
    // replacing them) with rc2dgi_write's values.  List, count and status as for rc2dgi_paint_device; the working memory
    // is the one rc2dgi_paint_device_limits reports.  Keep the atlas alive until rc2dgi_sync.
    [StructLayout(LayoutKind.Sequential)]
    public struct Atlas
    {
        public void* Dev;
        public int W, H;
        public int PitchBytes;         // 0 = tight
        public int Format;             // 0 RGBA8, 1 RGBA32F, 2 RGBA16F
    }
    [StructLayout(LayoutKind.Sequential, Size = 32)]
    public struct Sprite
    {
        public int Sx, Sy, W, H;
        public int Dx, Dy;
        public byte R, G, B, A;        // tint
        public uint Flags;             // SpriteFlipX | SpriteFlipY | SpriteReplace
    }
    public const uint SpriteFlipX = 1, SpriteFlipY = 2, SpriteReplace = 4;
    [DllImport(Lib)] public static extern int rc2dgi_sprites_device(IntPtr ctx, int which, byte* clearRgba, Atlas* atlas, void* spritesDev, int n, void* countDev, void* statusDev);

    // rc2dgi_sprites_xf_device: the same list with every sprite scaled, rotated, sheared or mirrored -- DrawTexturePro.
    // The source rectangle's top-left corner lands on (Px, Py), its top edge becomes the vector (Ax, Ay), its left edge
    // (Bx, By), in screen pixels (y down); the producer computes them, the device does no trigonometry.  Flags:
    // SpriteReplace | SpriteLinear (the flips are refused: a mirrored sprite has a negative determinant).
    [StructLayout(LayoutKind.Sequential, Size = 48)]
    public struct SpriteXf
    {
        public int Sx, Sy, W, H;
        public float Px, Py;
        public float Ax, Ay;
        public float Bx, By;
        public byte R, G, B, A;        // tint
        public uint Flags;             // SpriteReplace | SpriteLinear
    }
    public const uint SpriteLinear = 8;
    [DllImport(Lib)] public static extern int rc2dgi_sprites_xf_device(IntPtr ctx, int which, byte* clearRgba, Atlas* atlas, void* spritesDev, int n, void* countDev, void* statusDev);

    // rc2dgi_shapes_device: rectangles, circles, triangles, thick lines and ellipses from a list in device memory,
    // mixed and painted in list order as rc2dgi_paint_device paints.  V0 .. V5 by Kind: Rect x, y, w, h; Circle x, y,
    // radius; Triangle x0, y0, x1, y1, x2, y2; Line x0, y0, x1, y1, thick; Ellipse cx, cy, rh, rv.
    [StructLayout(LayoutKind.Sequential, Size = 32)]
    public struct Shape
    {
        public int Kind;               // ShapeRect .. ShapeEllipse
        public float V0, V1, V2, V3, V4, V5;
        public byte R, G, B, A;        // raylib Color
    }
    public const int ShapeRect = 0, ShapeCircle = 1, ShapeTriangle = 2, ShapeLine = 3, ShapeEllipse = 4;
    [DllImport(Lib)] public static extern int rc2dgi_shapes_device(IntPtr ctx, int which, byte* clearRgba, void* shapesDev, int n, void* countDev, void* statusDev);

    // rc2dgi_gradients_device: the same five shapes with a colour a vertex and an HDR gain (soft round lights, beams,
    // washed walls).  V0 .. V5 by Kind as Shape's.  Colours by Kind: Triangle C0 .. C2, one a vertex; Rect C0 .. C3 =
    // TL, BL, BR, TR; Circle and Ellipse C0 the centre, C1 the rim; Line C0 the (x0, y0) end, C1 the other.  Each is
    // a raylib Color packed r | g << 8 | b << 16 | a << 24 (its bytes in memory order).  Gain multiplies r, g, b
    // after the interpolation.
    [StructLayout(LayoutKind.Sequential, Size = 48)]
    public struct Gradient
    {
        public int Kind;               // GradRect .. GradEllipse
        public float V0, V1, V2, V3, V4, V5;
        public uint C0, C1, C2, C3;    // raylib Colors, bytes r, g, b, a
        public float Gain;
    }
    public const int GradRect = 0, GradCircle = 1, GradTriangle = 2, GradLine = 3, GradEllipse = 4;
    [DllImport(Lib)] public static extern int rc2dgi_gradients_device(IntPtr ctx, int which, byte* clearRgba, void* gradsDev, int n, void* countDev, void* statusDev);

    // rc2dgi_tilemap_device: a tile map drawn as one layer -- a Rows x Cols grid of 32-bit cell words in device memory
    // (Tiled's global tile ids: 0 an empty cell, bit 31 / 30 the horizontal / vertical flip), cells of TileW x TileH
    // pixels from a tile set (the atlas) of SetCols tiles a row with Tiled's Margin and Spacing, cell (0, 0) at (Ox, Oy)
    // of the screen: scrolling is those two integers.  No list and no working memory; statusDev: null or two int32
    // that receive {drawn, refused} over the visible cells.  Flags: SpriteReplace or 0.
    [StructLayout(LayoutKind.Sequential, Size = 56)]
    public struct Tilemap
    {
        public void* CellsDev;         // Rows x Cols words on the context's device, row 0 the top row
        public int Cols, Rows;         // 0 .. 32768
        public int PitchCells;         // 0 = Cols
        public int TileW, TileH;       // 1 .. 32768
        public int Ox, Oy;             // the scroll, within 2^22 of zero
        public int SetCols;            // 1 .. 32768
        public int Margin, Spacing;    // 0 .. 32768
        public byte R, G, B, A;        // tint of the whole layer
        public uint Flags;             // SpriteReplace or 0
    }
    public const uint TileFlipX = 0x80000000, TileFlipY = 0x40000000;
    [DllImport(Lib)] public static extern int rc2dgi_tilemap_device(IntPtr ctx, int which, byte* clearRgba, Atlas* atlas, Tilemap* map, void* statusDev);

    // rc2dgi_view: one draw of the display frame (window rectangle, y down; Filter 0 = the texture's own,
    // 1 POINT, 2 LINEAR; border A == 0: none)
    [StructLayout(LayoutKind.Sequential)]
    public struct View
    {
        public int Which, X, Y, W, H;
        public int Filter;
        public byte R, G, B, A;
    }
    public const int MaxViews = 16;
    [DllImport(Lib)] public static extern int rc2dgi_display_layout(ref Config cfg, View* views, int maxViews);
    [DllImport(Lib)] public static extern int rc2dgi_compose(IntPtr ctx, View* views, int n, int outW, int outH, byte* clearRgba, void* host, int pitchBytes);
    [DllImport(Lib)] public static extern int rc2dgi_compose_device(IntPtr ctx, View* views, int n, int outW, int outH, byte* clearRgba, void* dev, int pitchBytes);

    // Queries: a few values of the frame without a Download.  rc2dgi_sample: texture(T, (u, v)) for n points
    // (uv: 2 floats a point, GL coordinates, v up -- the centre of y-down pixel (x, y) of a W x H texture is
    // ((x + 0.5f) / W, 1 - (y + 0.5f) / H); rgba: 4 floats a point; filter as View.Filter).  rc2dgi_raycast:
    // SampleRadianceSDF (RadianceCascades.fs:60-92) for n rays over the last frame.
    [StructLayout(LayoutKind.Sequential, Size = 24)]
    public struct Ray
    {
        public float Ox, Oy;           // origin, GL texture coordinates
        public float Dx, Dy;           // direction, used as given
        public float T0, T1;           // the interval marched
    }
    [StructLayout(LayoutKind.Sequential, Size = 44)]
    public struct RayHit
    {
        public int Status;             // RayStatus
        public int Steps;              // distRT texels read
        public int Ix, Iy;             // the hit texel (GL order), or (-1, -1)
        public float T, U, V;          // where the loop ended
        public float R, G, B, A;       // the shader's hit record
    }
    public enum RayStatus { Invalid = -1, Range = 0, Edge = 1, Emissive = 2, Surface = 3, Steps = 4 }
    [DllImport(Lib)] public static extern int rc2dgi_sample(IntPtr ctx, int which, int filter, float* uv, int n, float* rgba);
    [DllImport(Lib)] public static extern int rc2dgi_sample_device(IntPtr ctx, int which, int filter, void* uvDev, int n, void* rgbaDev);
    [DllImport(Lib)] public static extern int rc2dgi_raycast(IntPtr ctx, Ray* rays, int n, RayHit* hits);
    [DllImport(Lib)] public static extern int rc2dgi_raycast_device(IntPtr ctx, void* raysDev, int n, void* hitsDev);

    // Region statistics: rectangles of a render texture measured without a Download.  Per rectangle and channel the
    // count of NaN / infinite values, min and max of the finite ones and their double sum in the header's fixed order
    // (the same bits on every run).  rects is host memory in both variants.  (rc2dgi_rect is TexRect here: this class
    // already has a Rect, the primitive's constructor.)
    [StructLayout(LayoutKind.Sequential, Size = 16)]
    public struct TexRect
    {
        public int X, Y, W, H;         // texels of that texture, GL order (row 0 = bottom)
    }
    [StructLayout(LayoutKind.Sequential, Size = 88)]
    public struct Stats
    {
        public int Status;             // 0, or -1: the rectangle does not lie inside the texture (all else 0)
        public int Texels;             // w * h
        public fixed int Nonfinite[4]; // per channel r, g, b, a: values that are NaN or +-inf
        public fixed float Min[4], Max[4];
        public fixed double Sum[4];    // offset 56; Sum[c] / (Texels - Nonfinite[c]) is the mean
    }
    [DllImport(Lib)] public static extern int rc2dgi_reduce(IntPtr ctx, int which, TexRect* rects, int n, Stats* stats);
    [DllImport(Lib)] public static extern int rc2dgi_reduce_device(IntPtr ctx, int which, TexRect* rects, int n, void* statsDev);

    // Edge tables: bin(v) = the number of ascending float edges <= v, exact on any hardware.  With 255 edges a tone
    // curve (any monotone float -> byte map; the host computes the edges), with m edges a histogram's bin index.
    // A Tone is a view's exposure and curve slot (0: q8, the untoned conversion; 1 .. 8: rc2dgi_set_curve's tables);
    // a histogram record is m + 4 uints {status, texels, nan, bin[0] .. bin[m]}.  rects and edges are host memory.
    public const int CurveEdges = 255, MaxCurves = 8, HistMaxEdges = 1023;
    public enum Channel { R = 0, G = 1, B = 2, A = 3, Luma = 4 }
    [StructLayout(LayoutKind.Sequential, Size = 8)]
    public struct Tone
    {
        public float Exposure;         // >= 0, finite: each colour channel is multiplied by it (one float multiply)
        public int Curve;              // 0: q8; 1 .. MaxCurves: that slot's 255 edges
    }
    [DllImport(Lib)] public static extern int rc2dgi_check_edges(float* edges, int m);
    [DllImport(Lib)] public static extern int rc2dgi_curve_q8(float* edges255);
    [DllImport(Lib)] public static extern int rc2dgi_set_curve(IntPtr ctx, int slot, float* edges255);
    [DllImport(Lib)] public static extern int rc2dgi_compose_tone(IntPtr ctx, View* views, Tone* tones, int n, int outW, int outH, byte* clearRgba, void* host, int pitchBytes);
    [DllImport(Lib)] public static extern int rc2dgi_compose_tone_device(IntPtr ctx, View* views, Tone* tones, int n, int outW, int outH, byte* clearRgba, void* dev, int pitchBytes);
    [DllImport(Lib)] public static extern int rc2dgi_histogram(IntPtr ctx, int which, int channel, TexRect* rects, int n, float* edges, int m, uint* counts);
    [DllImport(Lib)] public static extern int rc2dgi_histogram_device(IntPtr ctx, int which, int channel, TexRect* rects, int n, float* edges, int m, void* countsDev);

    // A rectangle of a render texture as an image converted on the device (rect null: the whole texture): RGBA32F,
    // RGBA16F (round to nearest even) or RGBA8 (q8) pixels in rows of pitchBytes (0: tight).  With ReadFlip image row 0
    // is the rectangle's top row, the order rc2dgi_compose writes.  dev: aligned to a pixel, as pitchBytes is.
    public const int ReadFlip = 1;
    [DllImport(Lib)] public static extern int rc2dgi_read(IntPtr ctx, int which, TexRect* rect, int format, int flags, void* host, int pitchBytes);
    [DllImport(Lib)] public static extern int rc2dgi_read_device(IntPtr ctx, int which, TexRect* rect, int format, int flags, void* dev, int pitchBytes);

    // An image into a rectangle of an input (RT.Color or RT.Emissive; rect null: the whole texture), converted on the
    // device: RGBA32F, RGBA16F (widened exactly) or RGBA8 pixels in rows of pitchBytes (0: tight) become the texels
    // rc2dgi_upload would store.  WriteFlip: image row 0 is the rectangle's top row.  WriteBlend: the image is blended
    // over the texels (SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels, what DrawTextureRec into the render texture
    // does).  dev: aligned to a pixel, as pitchBytes is; a sprite of an atlas is a pointer and a pitch.
    public const int WriteFlip = 1;
    public const int WriteBlend = 2;
    [DllImport(Lib)] public static extern int rc2dgi_write(IntPtr ctx, int which, TexRect* rect, int format, int flags, void* host, int pitchBytes);
    [DllImport(Lib)] public static extern int rc2dgi_write_device(IntPtr ctx, int which, TexRect* rect, int format, int flags, void* dev, int pitchBytes);

    static IntPtr ctx;
    static Config config;
    static byte[] scratch = Array.Empty<byte>();

    static void Check(int rc, string what)
    {
        if (rc != OK)
            throw new InvalidOperationException($"{what}: rc2dgi error {rc}: {Marshal.PtrToStringUTF8(rc2dgi_last_error(ctx))}");
    }

    // RC2DGI.cs:65-98 (knobs + render-texture set)
    public static void Init(int screenWidth, int screenHeight, int cascadeCount, float renderScale, float rayRange)
    {
        var cfg = new Config { ScreenWidth = screenWidth, ScreenHeight = screenHeight, CascadeCount = cascadeCount,
                               RenderScale = renderScale, RayRange = rayRange };
        Check(rc2dgi_create(ref cfg, out ctx), "rc2dgi_create");
        config = cfg;
    }

    public static void Shutdown() { if (ctx != IntPtr.Zero) rc2dgi_destroy(ctx); ctx = IntPtr.Zero; }

    // SetGIShaderValues (RC2DGI.cs:408-433) + the blur radius (RC2DGI.cs:374): same names
    public static void SetUniform(string name, float v) => Check(rc2dgi_set_uniform(ctx, name, &v, 1), name);
    public static void SetUniform(string name, System.Numerics.Vector3 v)
    {
        float* p = stackalloc float[3] { v.X, v.Y, v.Z };
        Check(rc2dgi_set_uniform(ctx, name, p, 3), name);
    }

    // painted colorRT / emissiveRT -> device (RGBA8 in GL row order, as rlReadTexturePixels returns it)
    public static void Upload(RT which, RenderTexture2D rt)
    {
        Image img = Raylib.LoadImageFromTexture(rt.Texture);
        try { Check(rc2dgi_upload(ctx, (int)which, img.Data, rt.Texture.Width * 4, (int)Format.RGBA8), "upload"); }
        finally { Raylib.UnloadImage(img); }
    }

    // device render texture -> the raylib texture that displays it (debug views / final blit)
    public static void Download(RT which, RenderTexture2D rt)
    {
        int n = rt.Texture.Width * rt.Texture.Height * 4;
        if (scratch.Length < n) scratch = new byte[n];
        fixed (byte* p = scratch)
        {
            Check(rc2dgi_download(ctx, (int)which, p, rt.Texture.Width * 4, (int)Format.RGBA8), "download");
            Raylib.UpdateTexture(rt.Texture, p);
        }
    }

    // The display half of the main loop (RC2DGI.cs:135-165, 435-448) in one call: colorRT over the window and the
    // seven debug thumbnails, composed on the GPU into one RGBA8 image (row 0 = top) and uploaded into
    // windowTexture (a screen-sized RGBA8 texture from LoadTextureFromImage; draw it with DrawTexture(t, 0, 0,
    // Color.White), unflipped).  Replaces one Download per view.
    public static void Present(Texture2D windowTexture, bool thumbnails = true)
    {
        int w = windowTexture.Width, h = windowTexture.Height;
        if (scratch.Length < w * h * 4) scratch = new byte[w * h * 4];
        View* views = stackalloc View[8];
        Config cfg = config;
        cfg.ScreenWidth = w;   // (the layout follows the window: view 0 covers it, thumbnails at its right edge)
        cfg.ScreenHeight = h;
        int n = Math.Min(rc2dgi_display_layout(ref cfg, views, 8), 8);
        fixed (byte* p = scratch)
        {
            Check(rc2dgi_compose(ctx, views, thumbnails ? n : 1, w, h, null, p, w * 4), "compose");
            Raylib.UpdateTexture(windowTexture, p);
        }
    }

    // The light arriving at a window position (y down): one LINEAR sample of the final GI instead of a Download.
    public static System.Numerics.Vector4 LightAt(float x, float y)
    {
        float* uv = stackalloc float[2] { x / config.ScreenWidth, 1f - y / config.ScreenHeight };
        float* c = stackalloc float[4];
        Check(rc2dgi_sample(ctx, (int)RT.FinalGI, 0, uv, 1, c), "sample");
        return new System.Numerics.Vector4(c[0], c[1], c[2], c[3]);
    }

    // Do two window positions see each other?  One ray from a to b over distRT: it ends by range when nothing is hit.
    public static bool Visible(System.Numerics.Vector2 a, System.Numerics.Vector2 b)
    {
        float w = config.ScreenWidth, h = config.ScreenHeight, mx = Math.Max(w, h);
        // the march evaluates px = ox + t * dx * (h / mx), py = oy + t * dy * (w / mx) and advances t by distRT's
        // value, a length in texture coordinates: the direction below moves one such unit per unit of t (a longer one
        // would step through walls), and the ray reaches b at t = len
        float ux = (b.X - a.X) / w, uy = -(b.Y - a.Y) / h, len = MathF.Sqrt(ux * ux + uy * uy);
        if (len == 0f) return true;
        var ray = new Ray { Ox = a.X / w, Oy = 1f - a.Y / h, Dx = ux / len * (mx / h), Dy = uy / len * (mx / w), T0 = 0f, T1 = len };
        RayHit hit;
        Check(rc2dgi_raycast(ctx, &ray, 1, &hit), "raycast");
        return hit.Status == (int)RayStatus.Range;
    }

    // The light arriving at a sprite: the mean of the final GI over the window rectangle it covers (y down), from one
    // region reduction instead of a Download.  The rectangle is clipped to the texture; empty: zero.
    public static System.Numerics.Vector4 MeanLight(Rectangle sprite)
    {
        Check(rc2dgi_query(ctx, out int cw, out int ch, out _, out _), "query");
        float sx = cw / (float)config.ScreenWidth, sy = ch / (float)config.ScreenHeight;
        int x0 = Math.Clamp((int)MathF.Floor(sprite.X * sx), 0, cw), x1 = Math.Clamp((int)MathF.Ceiling((sprite.X + sprite.Width) * sx), 0, cw);
        int y0 = Math.Clamp((int)MathF.Floor(sprite.Y * sy), 0, ch), y1 = Math.Clamp((int)MathF.Ceiling((sprite.Y + sprite.Height) * sy), 0, ch);
        if (x1 <= x0 || y1 <= y0) return System.Numerics.Vector4.Zero;
        var rect = new TexRect { X = x0, Y = ch - y1, W = x1 - x0, H = y1 - y0 };  // row 0 of the texture is the bottom
        Stats st;
        Check(rc2dgi_reduce(ctx, (int)RT.FinalGI, &rect, 1, &st), "reduce");
        var m = new float[4];
        for (int c = 0; c < 4; ++c)
        {
            int finite = st.Texels - st.Nonfinite[c];
            m[c] = finite > 0 ? (float)(st.Sum[c] / finite) : 0f;
        }
        return new System.Numerics.Vector4(m[0], m[1], m[2], m[3]);
    }

    // Auto-exposure without a Download: the luminance histogram of the final GI over a texture rectangle (256
    // log-spaced edges from 2^-16 to 2^16), its 90th percentile, and the exposure that maps that luminance to `key`
    // (0.8: just below white).  Pass the result as the main view's Tone to rc2dgi_compose_tone; Curve names a slot set
    // with rc2dgi_set_curve (an sRGB table, say), 0 shows the scaled values through q8.
    public static Tone AutoExposure(TexRect rect, float key, int curve = 0)
    {
        const int m = 256;
        float* edges = stackalloc float[m];
        for (int i = 0; i < m; ++i) edges[i] = MathF.Pow(2f, -16f + 32f * i / (m - 1));
        uint* rec = stackalloc uint[m + 4];
        Check(rc2dgi_histogram(ctx, (int)RT.FinalGI, (int)Channel.Luma, &rect, 1, edges, m, rec), "histogram");
        long counted = (long)rec[1] - rec[2], run = 0;
        if (rec[0] != 0 || counted <= 0) return new Tone { Exposure = 1f, Curve = curve };
        int b = 0;
        for (; b <= m; ++b) { run += rec[3 + b]; if (run * 10 >= counted * 9) break; }
        float level = edges[Math.Min(b, m - 1)];   // the edge at which the running count reaches 90 %
        return new Tone { Exposure = key / level, Curve = curve };
    }

    public static Prim Rect(Rectangle r, Color c) => new Prim { Kind = 0, X = r.X, Y = r.Y, W = r.Width, H = r.Height, R = c.R, G = c.G, B = c.B, A = c.A };
    public static Prim Circle(System.Numerics.Vector2 p, float radius, Color c) => new Prim { Kind = 1, X = p.X, Y = p.Y, W = radius, R = c.R, G = c.G, B = c.B, A = c.A };

    // BeginTextureMode(rt); ClearBackground(clear); draw prims; EndTextureMode -- on the GPU
    // (RenderScene / RedrawSceneToRTs, RC2DGI.cs:224-264, 528-545)
    public static void Paint(RT which, Color? clear, System.Collections.Generic.List<Prim> prims)
    {
        Prim[] a = prims.ToArray();
        byte* cl = stackalloc byte[4];
        if (clear is Color c) { cl[0] = c.R; cl[1] = c.G; cl[2] = c.B; cl[3] = c.A; }
        fixed (Prim* p = a)
            Check(rc2dgi_paint(ctx, (int)which, clear.HasValue ? cl : null, p, a.Length), "paint");
    }

    // DoRC2DGI() (RC2DGI.cs:267-406)
    public static void DoRC2DGI() => Check(rc2dgi_do(ctx), "rc2dgi_do");
}
