// shs_canvas_rt.hip -- the Canvas render-target raster of the hello-render-target/ demos, for
// hello_shadow_mapping.cpp (paths relative to the reference's cpp-folders/src/hello-render-target/):
//   PASS0  draw_triangle_tile_shadow (:791-834): depth only from the light, ndc z in [0, 1];
//   PASS1  draw_triangle_tile_color_depth_motion_shadow (:854-1022) with vertex_shader_full (:602-620) and
//          fragment_shader_full (:699-750): near-plane clipping in clip space, no facing cull, view-z depth
//          in canvas rows, perspective-correct world position and UV, velocity, the shadow lookup.
// and for hello_shadow_mapping_soft.cpp ("soft :line"), whose PASS0 is the same depth raster and whose PASS1
// (draw_triangle_tile_color_depth_softshadow, soft :845-986) is the same clipped raster without the velocity:
//   shading 1  fragment_shader_softshadow (soft :991-1040) over pcss_shadow_factor (soft :333-445): a centre
//          lookup, a blocker search and a variable-radius PCF over a Poisson disc rotated per screen pixel.
//          The rotations' cos / sin come from a host table (RtParams::rot): the reference takes them from its
//          libm, which is not correctly rounded, and one ulp can move a tap to another texel.
//          k_rt_raster<false, 1> differs from k_rt_raster<false, 0> in the shade alone.
// and for hello_pbr.cpp ("pbr :line"), whose PASS0 / PASS1 rasters (pbr :827-870, :883-1045) are the hard demo's:
//   shading 2  fragment_shader_pbr (pbr :627-727): Cook-Torrance GGX under the 2x2-PCF shadow, plus image-based
//          lighting from an irradiance cubemap and a prefiltered-specular mip chain (shs/resources/ibl.hpp:215-286;
//          RtParams::ibl).  k_rt_raster<false, 2>, launched by shs_rt_render_pbr, again differs in the shade alone.
// and for hello_pbr_light_shafts.cpp ("shafts :line"), whose PASS1 raster (shafts :1015-1180) is hello_pbr.cpp's:
//   shading 3  its fragment_shader_pbr (shafts :768-850): the shader of shading 2 under pcss_shadow_factor (shafts
//          :650-762, the soft demo's text) instead of the 2x2 PCF, without the minimum-ambient term.
//          k_rt_raster<false, 3>, launched by shs_rt_render_pbr_soft, is shade_pixel_pbr<true>.
// and for hello_ibl_skybox.cpp ("ibl :line"), whose PASS0 / PASS1 rasters (ibl :646-686, :705-860) are the hard demo's:
//   shading 4  its fragment_shader_full (ibl :446-524): the hard demo's Blinn-Phong under the 2x2 PCF -- but for the specular
//          term, which does not take the base colour -- with the ambient term tinted by u.sky->sample(N) and a
//          Schlick-weighted u.sky->sample(reflect(-V, N)) added; u.sky is the sky of the background pass below.
//          k_rt_raster<false, 4 + sky model> (rt_variant below), launched by shs_rt_render_skybox_ibl, is shade_pixel_ibl<SKY>: three
//          instantiations (no sky, AnalyticSky, CubeMapSky), of which only the last has gathers.
// and for hello_water.cpp ("water :line"), whose PASS0 / PASS1 rasters, vertex shader, velocity and shadow_uvz_from_world
// are the hard demo's text (DESIGN.md section 8 lists the routines compared):
//   shading 5  two fragment shaders in one camera pass, chosen per draw (shs_rt_water_draw): fragment_shader_full
//          (water :938-994, the "atmosphere" shader: Blinn-Phong under a sky-coloured ambient term, fog, Reinhard, gamma)
//          and fragment_shader_water (water :1000-1097: a procedural flow normal and foam from water_flow_normal_and_foam
//          :862-930 over hash12 / noise2 / fbm2, Schlick's fresnel over a planar reflection read from the context's
//          reflection canvas, fog).  Both round to the byte where the other shadings truncate.  Their shadow lookup
//          (water :716-751) is not the hard demo's: shadow_factor_water.  k_rt_raster<false, 7> (rt_variant(5, .)),
//          launched by shs_rt_render_water, is shade_pixel_water.
// and for hello_multi_pass.cpp ("multi :line"; hello_camera_and_perobject_motion_blur.cpp carries the same text at
// :542-615 and :224-254) and hello_glowing_star.cpp ("star :line"), whose one raster is not the hard demo's:
//   draw_triangle_tile_color_depth_motion (multi :525-599) / draw_triangle_color_depth_velocity_spec (star :354-435): no
//          near-plane clip and no w test, back faces culled (area <= 0), every varying screen-linear, the velocity clamp's
//          second threshold 0.0001, and a fragment that wins the depth test always writes its colour.
//          k_rt_setup_motion is the setup without the clip; the raster's candidate walk drops the invw_sum rule.
//   shading 6  blinn_phong_fragment_shader (multi :207-237): k_rt_raster<false, 8>, shade_pixel_motion<false>.
//   shading 7  star_fragment_shader (star :269-308), which returns spec01 beside the colour: k_rt_raster<false, 9>,
//          shade_pixel_motion<true>, the one instantiation that stores a fourth plane (RtParams::spec).  The star's
//          single job is the whole frame (its host passes ref_tile = the frame's size).
//          Both launched by shs_rt_render_motion.
// and for the three plain demos, whose rasters are that unclipped one again -- hello_per_object_motion_blur.cpp
// ("per :line") draw_triangle_velocity_tile :391-455, hello_depth_of_field.cpp ("dof :line") draw_triangle_tile :524-574,
// hello_ping_pong.cpp ("ping :line") draw_triangle_tile :352-400 -- with the Blinn-Phong body of shading 6 under an
// ambient term of 0.15 and a depth plane in SCREEN rows (all three hand test_and_set_depth the screen py):
//   shading 8  velocity_fragment_shader (per :139-177): the velocity per pixel from the interpolated clip positions, no
//          clamp.  k_rt_raster<false, 10>.
//   shading 9  dof :60-120 and shading 10 ping :65-98: no velocity; k_rt_raster<false, 11> for both.  Shading 10's depth is
//          clip z / clip w per corner (ping :389): k_rt_setup_motion<true>.
//          All launched by shs_rt_render_plain.
// and for hello_ibl_skybox_optimized.cpp ("opt :line") and hello_ibl_skybox_xsimd.cpp ("xsimd :line"), whose camera raster
// (opt :1125-1291) is the hard demo's and whose shader is one text in both files:
//   shading 11 fragment_shader_full (opt :875-958): Blinn-Phong with a per-object exponent under the 2x2 PCF on the direct
//          term alone, plus the irradiance cubemap along N and the prefiltered-specular mips along reflect(-V, N) at a lod
//          taken from the exponent (RtParams::ibl, as shading 2).  k_rt_raster<false, 12>, launched by
//          shs_rt_render_ibl_phong, is shade_pixel_ibl_phong.
//   the xsimd demo's PASS0  draw_triangle_tile_shadow_xsimd (xsimd :1016-1191): edge functions with inclusive tests, back
//          faces dropped, a floor / ceil box, and two associations of the edge sum within a row (the SIMD body and the
//          scalar tail).  k_rt_setup_edge and k_rt_raster<true, RT_SHADOW_EDGE>, launched by shs_rt_render_shadow_edge.
//          The optimized demo's PASS0 (opt :1065-1108) is the hard demo's.
//   the background  skybox_background_pass (pbr :733-799; the same routine in hello_pbr_light_shafts.cpp and
//          hello_ibl_skybox.cpp) over the legacy AnalyticSky / CubeMapSky of hello-shs-renderer/shs_renderer.hpp:
//          k_rt_sky<MODEL, ENCODE>, a pass of its own after k_rt_raster when a sky is bound (shs_rt_set_sky), which
//          colours the pixels whose id is -1.  The reference draws the sky first and the triangles over it.
//
// One translation unit in three files:
//   shs_canvas_rt_frag.hpp     what every fragment shader does before its lighting, once: the fragment's inputs and
//                              interpolations (Frag), the velocity, the base colour, the two shadow lookups from a world
//                              position (2x2 PCF, PCSS), the byte packing, and the x86-64 conversions they need;
//   shs_canvas_rt_shaders.hpp  the fragment shaders shade_pixel* on top of it, each with its own samplers (IBL levels,
//                              legacy sky models, water noise);
//   this file                  the setup, the raster, the *_samples kernels, the background pass and the launchers.
//
// Two kernels per pass, the same two for both (template <bool SHADOW>):
//   k_rt_setup   one lane per input triangle: the vertex shader once per corner (the reference re-runs it
//                per tile job; it is pure), the Sutherland-Hodgman clip against z >= 0 in the reference's
//                push order (an unclipped triangle leaves it as {v1, v2, v0}), the fan (0, i, i + 1), and per
//                sub-triangle a raster record (RtRec, id 2 t + k) plus the corners' varyings (RtVary).
//   k_rt_raster  one workgroup per 32x8 tile, one pixel per lane.  Rounds of RT_CHUNK records in
//                submission order: every lane tests one record against the tile, the passing ones are
//                compacted into LDS in order, then each lane walks them in order and keeps (best depth,
//                shading id, u, v, w) in registers -- the strict '<' of ZBuffer::test_and_set_depth with the
//                first of equal depths winning, and the rule that a fragment with invw_sum <= 1e-8 keeps its
//                depth but not its colour, both without atomics.  Then the lane shades its pixel and stores
//                colour, depth and velocity once; the clear is the value of a pixel nothing covered.
//
// Tile-clamp semantics.  The reference clamps a sub-triangle's bbox to the tile job
// that runs it, so it also tests pixels outside the bbox: the clamped edge columns, rows and corners of
// every job.  Here a pixel evaluates the reference's own visit test for the job it lies in -- (int) of the
// clamped float bbox, per axis -- before the barycentric, so whatever a tile stages is tested exactly.  A
// record is staged for a tile when that visited set meets the tile and the tile meets the record's cull
// box: the legacy raster's error bound (danger_margin) proves every pixel outside it rejected.  Without the
// cull box a tile holding a job's corner pixel would stage every record (each is visited there).  A sliver
// with no usable bound has the whole target as its cull box: exact, not fast.
//
// Arithmetic: no contraction, correctly rounded '/' and sqrt (Makefile), GLM's operation order; the
// x86-64 float -> int conversions of the reference build are spelled out where a value can leave int's
// range; pow(x, 64.0f) by six squarings in double (as the legacy shaders' pow2k).
#include <utility>

#include "shs_canvas_rt_shaders.hpp"

namespace shs_dev {
namespace {

struct Vy {            // VaryingsFull :588-596
    float p[4], q[4];  // position, prev_position
    float wp[3], n[3];
    float uv[2];
    float vz;
};

__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + (b - a) * t; }

// lerp_vary :866-875
__device__ void lerp_vary(const Vy &a, const Vy &b, float t, Vy &o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { o.p[k] = lerp1(a.p[k], b.p[k], t); o.q[k] = lerp1(a.q[k], b.q[k], t); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { o.wp[k] = lerp1(a.wp[k], b.wp[k], t); o.n[k] = lerp1(a.n[k], b.n[k], t); }
    o.uv[0] = lerp1(a.uv[0], b.uv[0], t);
    o.uv[1] = lerp1(a.uv[1], b.uv[1], t);
    o.vz = lerp1(a.vz, b.vz, t);
}

// intersect :885-893
__device__ void intersect(const Vy &a, const Vy &b, Vy &o) {
    const float az = a.p[2], bz = b.p[2];
    const float denom = bz - az;
    float t = (fabsf(denom) < 1e-8f) ? 0.0f : ((0.0f - az) / denom);
    t = (t < 0.0f) ? 0.0f : (t > 1.0f ? 1.0f : t);   // clampf :86-91
    lerp_vary(a, b, t, o);
}

__device__ __forceinline__ bool inside(const Vy &v) { return (v.p[3] > 1e-6f) && (v.p[2] >= 0.0f); }

__device__ __forceinline__ bool finitef(float x) { return fabsf(x) <= FLT_MAX; }
// floor of a float, clamped into [lo, hi] before the conversion (a NaN gives lo)
__device__ __forceinline__ int floor_clamped(float x, int lo, int hi) {
    return (int)fminf(fmaxf(floorf(x), (float)lo), (float)hi);
}

// The legacy raster's error bound (shs_legacy.hip danger_margin) over this record: the
// barycentric arithmetic is the same, and the bound is orientation-independent.  A pixel whose centre lies
// rx / ry px outside the float bbox has a minimal exact barycentric <= -max(rx / 2Wx, ry / 2Wy); the float
// evaluation's error is at most E = e0 + ex rx + ey ry (u = 2^-24; dot products 2u, the two-product
// differences 6u, the divide and 1 - v - w a few u more; 25 % slack), so the pixel is provably rejected
// outside the bbox grown by (dgx, dgy) = 2 W m0, m0 = e0 / (1 - 2 (ex Wx + ey Wy)).  (-1, -1): no bound.
__device__ double2 danger_margin(const RtRec &r) {
    const double2 none = make_double2(-1.0, -1.0);
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double a = fabs((double)r.v0x), b = fabs((double)r.v0y);
    const double c = fabs((double)r.v1x), d = fabs((double)r.v1y);
    const double Wx = (double)r.maxx - (double)r.minx, Wy = (double)r.maxy - (double)r.miny;
    if (!(Wx > 0.0) || !(Wy > 0.0)) return none;
    const double A00 = a * a + b * b, A11 = c * c + d * d, A01 = a * c + b * d;
    const double Dabs = fabs((double)r.denom);
    const double ED = 6.1 * u * (A00 * A11 + A01 * A01);
    const double Dlow = Dabs - ED;
    if (!(Dlow > 0.0) || !(Dabs < 1e300)) return none;
    const double iDlow = 1.0 / Dlow, iDabs = 1.0 / Dabs;
    const double K1 = 7.2 * u + ED * iDlow;
    const double p0 = Wx + 0.01, q0 = Wy + 0.01;
    const double A20 = p0 * a + q0 * b, A21 = p0 * c + q0 * d;
    const double Nv0 = A11 * A20 + A01 * A21, Nvx = A11 * a + A01 * c, Nvy = A11 * b + A01 * d;
    const double Nw0 = A00 * A21 + A01 * A20, Nwx = A00 * c + A01 * a, Nwy = A00 * d + A01 * b;
    const double s = K1 * iDabs * (2.0 + 2.0 * u);
    const double e0 = 1.25 * ((Nv0 + Nw0) * s + u * (2.0 + (2.0 * Nv0 + Nw0) * iDlow));
    const double ex = 1.25 * ((Nvx + Nwx) * s + u * (2.0 * Nvx + Nwx) * iDlow);
    const double ey = 1.25 * ((Nvy + Nwy) * s + u * (2.0 * Nvy + Nwy) * iDlow);
    const double S = ex * Wx + ey * Wy;
    if (!(S < 0.5)) return none;
    const double m0 = e0 / (1.0 - 2.0 * S);
    const double dgx = 2.0 * Wx * m0, dgy = 2.0 * Wy * m0;
    return (dgx < 1e6 && dgy < 1e6) ? make_double2(dgx, dgy) : none;
}

// The pixel-independent part of barycentric_coordinate (shs_renderer.hpp:802-815), the area test and the
// bbox over the corners that are not NaN.  false: the sub-triangle draws nothing.  CULL_BACK: the area rule of the
// unclipped raster (multi :560, star :392), which draws positive areas only and does not reject a NaN; every
// barycentric of such a triangle is NaN, its depth is NaN and the pixel loop's depth test fails.
template <bool CULL_BACK = false>
__device__ bool rec_geometry(RtRec &r, const float (&sx)[3], const float (&sy)[3], int W, int H) {
    r.ax = sx[0]; r.ay = sy[0];
    r.v0x = sx[1] - sx[0]; r.v0y = sy[1] - sy[0];
    r.v1x = sx[2] - sx[0]; r.v1y = sy[2] - sy[0];
    r.d00 = r.v0x * r.v0x + r.v0y * r.v0y;
    r.d01 = r.v0x * r.v1x + r.v0y * r.v1y;
    r.d11 = r.v1x * r.v1x + r.v1y * r.v1y;
    r.denom = r.d00 * r.d11 - r.d01 * r.d01;
    const float area = r.v0x * r.v1y - r.v0y * r.v1x;
    float mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        mnx = g_min(mnx, sx[i]); mxx = g_max(mxx, sx[i]);
        mny = g_min(mny, sy[i]); mxy = g_max(mxy, sy[i]);
    }
    r.minx = mnx; r.maxx = mxx; r.miny = mny; r.maxy = mxy;
    // the cull box: the integer bbox, for a sliver grown by its danger margin + 1 px; the whole target where
    // there is no bound (or a large one): every pixel the reference visits is then tested
    const bool dfin = finitef(r.d00) && finitef(r.d01) && finitef(r.d11) && finitef(r.denom);
    const double2 dg = dfin ? danger_margin(r) : make_double2(-1.0, -1.0);
    const bool unbounded = !(dg.x >= 0.0) || dg.x > GHOST_MAX_EXPAND || dg.y > GHOST_MAX_EXPAND;
    const bool ghost = dg.x >= 0.49 || dg.y >= 0.49;
    const double exx = ghost ? dg.x + 1.0 : 0.0, exy = ghost ? dg.y + 1.0 : 0.0;
    const int cx0 = unbounded ? 0 : floor_clamped((float)((double)mnx - exx), 0, W);
    const int cx1 = unbounded ? W - 1 : floor_clamped((float)((double)mxx + exx), -1, W - 1);
    const int cy0 = unbounded ? 0 : floor_clamped((float)((double)mny - exy), 0, H);
    const int cy1 = unbounded ? H - 1 : floor_clamped((float)((double)mxy + exy), -1, H - 1);
    r.gbx = pack16(cx0, cx1);
    r.gby = pack16(cy0, cy1);
    if constexpr (CULL_BACK) {
        if (area <= 0.0f) return false;
    } else {
        if (fabsf(area) < 1e-8f) return false;
    }
    r.flags = RT_VALID | (area < 0.0f ? RT_NEG_AREA : 0u);
    // |denom| < 1e-5 (a double comparison): every barycentric is -1, nothing passes -- not staged
    if ((double)fabsf(r.denom) < 1e-5) r.flags = 0u;
    return true;
}

__device__ __forceinline__ void store_rec(RtRec *dst, const RtRec &r) {
    const float4 *s = reinterpret_cast<const float4 *>(&r);
    float4 *d = reinterpret_cast<float4 *>(dst);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = s[k];
}

// The corners' varyings of a camera-pass sub-triangle as the shaded pixels read them
__device__ __forceinline__ void store_vary(RtVary &v, const Vy *const (&tv)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { v.pos[4 * i + k] = tv[i]->p[k]; v.prev[4 * i + k] = tv[i]->q[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { v.world[3 * i + k] = tv[i]->wp[k]; v.nrm[3 * i + k] = tv[i]->n[k]; }
        v.uv[2 * i] = tv[i]->uv[0];
        v.uv[2 * i + 1] = tv[i]->uv[1];
    }
}

// One camera-pass sub-triangle {a, b, c} (:931-959 up to the pixel loops): its record and varyings.  Returns
// whether it reaches the raster (the w and area tests passed).
__device__ bool emit_camera(const RtParams &p, int32_t id, int32_t draw, const Vy &a, const Vy &b, const Vy &c) {
    RtRec r{};
    r.draw = draw;
    const Vy *tv[3] = {&a, &b, &c};
    bool ok = true;
    float sx[3], sy[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float w = tv[i]->p[3];
        if (w <= 1e-6f) ok = false;
        // Canvas::clip_to_screen (shs_renderer.hpp:823-831)
        const float nx = tv[i]->p[0] / w, ny = tv[i]->p[1] / w;
        sx[i] = (nx + 1.0f) * 0.5f * (float)(p.W - 1);
        sy[i] = (1.0f - ny) * 0.5f * (float)(p.H - 1);
    }
    if (ok) ok = rec_geometry(r, sx, sy, p.W, p.H);
    if (!ok) {
        r.flags = 0u;
    } else {
        r.z0 = a.vz; r.z1 = b.vz; r.z2 = c.vz;
        r.iw0 = (fabsf(a.p[3]) < 1e-6f) ? 0.0f : 1.0f / a.p[3];
        r.iw1 = (fabsf(b.p[3]) < 1e-6f) ? 0.0f : 1.0f / b.p[3];
        r.iw2 = (fabsf(c.p[3]) < 1e-6f) ? 0.0f : 1.0f / c.p[3];
        store_vary(p.vary[id], tv);
    }
    store_rec(&p.recs[id], r);
    return ok;
}

// The unclipped raster's triangle (multi :536-560; star :364-392): the corners in their own order, straight through
// Canvas::clip_to_screen with no w test (a corner behind the camera projects mirrored; w = 0 gives Inf or NaN screen
// coordinates, which the bbox fold and the barycentrics take as the reference's do), positive areas only.
// NDC_Z: the corners' depth is clip_to_screen's third component, clip z / clip w (hello_ping_pong.cpp:389), where the
// other demos interpolate the vertex shader's view z.
template <bool NDC_Z>
__device__ bool emit_motion(const RtParams &p, int32_t id, int32_t draw, const Vy (&in)[3]) {
    RtRec r{};
    r.draw = draw;
    float sx[3], sy[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float w = in[i].p[3];
        const float nx = in[i].p[0] / w, ny = in[i].p[1] / w;
        sx[i] = (nx + 1.0f) * 0.5f * (float)(p.W - 1);
        sy[i] = (1.0f - ny) * 0.5f * (float)(p.H - 1);
    }
    const bool ok = rec_geometry<true>(r, sx, sy, p.W, p.H);
    if (!ok) {
        r.flags = 0u;
    } else {
        if constexpr (NDC_Z) {
            r.z0 = in[0].p[2] / in[0].p[3]; r.z1 = in[1].p[2] / in[1].p[3]; r.z2 = in[2].p[2] / in[2].p[3];
        } else {
            r.z0 = in[0].vz; r.z1 = in[1].vz; r.z2 = in[2].vz;
        }
        const Vy *tv[3] = {&in[0], &in[1], &in[2]};
        store_vary(p.vary[id], tv);
    }
    store_rec(&p.recs[id], r);
    return ok;
}

// One atomic per wave and counter: the wave's lanes that are here, counted by ballot.
__device__ __forceinline__ void wave_count(unsigned long long *counter, bool mine) {
    const unsigned long long here = __ballot(1), m = __ballot(mine);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (m && lane == __ffsll((long long)here) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// The draw of triangle t (draws are few: the demo has three).
__device__ __forceinline__ int find_draw(const RtParams &p, int t) {
    int d = 0;
    while (d + 1 < p.n_draws && t >= p.draws[d + 1].base) ++d;
    return d;
}

// vertex_shader_full :602-620 at the three corners of the draw's triangle `local`; blinn_phong_vertex_shader_mb
// (multi :191-205) and star_vertex_shader (star :254-267) are the same operations with uv = vec2(0)
__device__ __forceinline__ void vertex_shader_full(const RtDrawGPU &dr, int local, Vy (&in)[3]) {
    const float *pos = dr.pos + 9 * (size_t)local;
    const float *nrm = dr.nrm + 9 * (size_t)local;
    const float *uv = dr.uv ? dr.uv + 6 * (size_t)local : nullptr;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
        m4p(dr.mvp, x, y, z, in[i].p[0], in[i].p[1], in[i].p[2], in[i].p[3]);
        m4p(dr.prev_mvp, x, y, z, in[i].q[0], in[i].q[1], in[i].q[2], in[i].q[3]);
        float ww, vx, vy, vw;
        m4p(dr.model, x, y, z, in[i].wp[0], in[i].wp[1], in[i].wp[2], ww);
        const f3 n = normalize3(m3v(dr.n3, f3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]}));
        in[i].n[0] = n.x; in[i].n[1] = n.y; in[i].n[2] = n.z;
        in[i].uv[0] = uv ? uv[2 * i] : 0.0f;
        in[i].uv[1] = uv ? uv[2 * i + 1] : 0.0f;
        m4p(dr.zm, x, y, z, vx, vy, in[i].vz, vw);
    }
}

template <bool SHADOW>
__global__ __launch_bounds__(256) void k_rt_setup(const RtParams p) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_tris) return;
    const int d = find_draw(p, t);
    const RtDrawGPU &dr = p.draws[d];
    const int local = t - dr.base;
    const float *pos = dr.pos + 9 * (size_t)local;
    if (SHADOW) {
        // shadow_vertex_shader :761-766, clip_to_shadow_screen :774-783, :797-820
        RtRec r{};
        r.draw = d;
        bool ok = true;
        float sx[3], sy[3], sz[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float cx, cy, cz, cw;
            m4p(dr.zm, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], cx, cy, cz, cw);
            if (fabsf(cw) < 1e-6f) ok = false;
            const float nx = cx / cw, ny = cy / cw;
            sx[i] = (nx * 0.5f + 0.5f) * (float)(p.W - 1);
            sy[i] = (1.0f - (ny * 0.5f + 0.5f)) * (float)(p.H - 1);
            sz[i] = cz / cw;
        }
        if (ok) ok = rec_geometry(r, sx, sy, p.W, p.H);
        if (!ok) r.flags = 0u;
        r.z0 = sz[0]; r.z1 = sz[1]; r.z2 = sz[2];
        store_rec(&p.recs[t], r);
        return;
    }
    Vy in[3];
    vertex_shader_full(dr, local, in);
    // clip_poly_near_z :877-913: at most four vertices leave a triangle
    Vy poly[4];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const Vy &A = in[i];
        const Vy &B = in[(i + 1) % 3];
        const bool a_in = inside(A), b_in = inside(B);
        if (a_in && b_in) {
            if (n < 4) poly[n] = B;
            ++n;
        } else if (a_in && !b_in) {
            if (n < 4) intersect(A, B, poly[n]);
            ++n;
        } else if (!a_in && b_in) {
            if (n < 4) intersect(A, B, poly[n]);
            ++n;
            if (n < 4) poly[n] = B;
            ++n;
        }
    }
    RtRec none{};
    bool r0 = false, r1 = false;
    if (n >= 3) r0 = emit_camera(p, 2 * t, d, poly[0], poly[1], poly[2]);
    else store_rec(&p.recs[2 * t], none);
    if (n >= 4) r1 = emit_camera(p, 2 * t + 1, d, poly[0], poly[2], poly[3]);
    else store_rec(&p.recs[2 * t + 1], none);
    wave_count(&p.stats[1], n == 3);
    wave_count(&p.stats[2], n == 4);
    wave_count(&p.stats[3], r0);
    wave_count(&p.stats[3], r1);
}

// The setup of shadings 6 and 7: one lane per input triangle, the vertex shader, no clip.  One record per triangle at
// id 2 t, so that a pixel's id reads as for every other camera pass; slot 2 t + 1 is empty.  Counter 3 is the number of
// triangles the area rule keeps; there are no clipped polygons to count.  It is also the setup of shadings 8 to 10, the
// same raster; NDC_Z (shading 10): the per-corner depth is clip z / clip w and the view-z product is not read.
template <bool NDC_Z>
__global__ __launch_bounds__(256) void k_rt_setup_motion(const RtParams p) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_tris) return;
    const int d = find_draw(p, t);
    const RtDrawGPU &dr = p.draws[d];
    Vy in[3];
    vertex_shader_full(dr, t - dr.base, in);
    const bool ok = emit_motion<NDC_Z>(p, 2 * t, d, in);
    RtRec none{};
    store_rec(&p.recs[2 * t + 1], none);
    wave_count(&p.stats[3], ok);
}

// The setup of the edge-function shadow pass: one lane per caster triangle, shadow_vertex_shader (xsimd :995-1000),
// clip_to_shadow_screen (:1006-1014) and what build_shadow_tri (:1031-1076) forms without the job: the area rule (back
// faces dropped), 1 / area, the edge functions and (int)floor / (int)ceil of the extent.  Those two conversions are
// undefined in the reference for a value that is not finite or does not fit an int: a triangle with such a screen
// corner is dropped here (include/shs_gpu.h says so).
__global__ __launch_bounds__(256) void k_rt_setup_edge(const RtParams p) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_tris) return;
    const int d = find_draw(p, t);
    const RtDrawGPU &dr = p.draws[d];
    const float *pos = dr.pos + 9 * (size_t)(t - dr.base);
    RtEdgeRec r{};
    r.draw = d;
    bool ok = true;
    float sx[3], sy[3], sz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float cx, cy, cz, cw;
        m4p(dr.zm, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], cx, cy, cz, cw);
        if (fabsf(cw) < 1e-6f) ok = false;
        const float nx = cx / cw, ny = cy / cw;
        sx[i] = (nx * 0.5f + 0.5f) * (float)(p.W - 1);
        sy[i] = (1.0f - (ny * 0.5f + 0.5f)) * (float)(p.H - 1);
        sz[i] = cz / cw;
        if (!(fabsf(sx[i]) < 2147483648.0f) || !(fabsf(sy[i]) < 2147483648.0f)) ok = false;   // (a NaN fails both)
    }
    if (ok) {
        const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
        if (fabsf(area) < 1e-8f || area <= 0.0f) ok = false;
        r.inv_area = 1.0f / area;
    }
    if (ok) {
        r.fminx = (int)floorf(fminf(fminf(sx[0], sx[1]), sx[2]));
        r.cmaxx = (int)ceilf(fmaxf(fmaxf(sx[0], sx[1]), sx[2]));
        r.fminy = (int)floorf(fminf(fminf(sy[0], sy[1]), sy[2]));
        r.cmaxy = (int)ceilf(fmaxf(fmaxf(sy[0], sy[1]), sy[2]));
        r.gbx = pack16(clampi(r.fminx, 0, p.W - 1), clampi(r.cmaxx, 0, p.W - 1));
        r.gby = pack16(clampi(r.fminy, 0, p.H - 1), clampi(r.cmaxy, 0, p.H - 1));
        r.A0 = sy[0] - sy[1]; r.B0 = sx[1] - sx[0]; r.C0 = sx[0] * sy[1] - sy[0] * sx[1];
        r.A1 = sy[1] - sy[2]; r.B1 = sx[2] - sx[1]; r.C1 = sx[1] * sy[2] - sy[1] * sx[2];
        r.A2 = sy[2] - sy[0]; r.B2 = sx[0] - sx[2]; r.C2 = sx[2] * sy[0] - sy[2] * sx[0];
        r.z0 = sz[0]; r.z1 = sz[1]; r.z2 = sz[2];
        r.flags = RT_VALID;
    }
    store_rec(&p.recs[t], reinterpret_cast<const RtRec &>(r));
}

// ---- k_rt_raster -----------------------------------------------------------------------------------

// The reference's visited interval of one axis inside the job [tmin, tmax] (:806-815, :822): the float bbox
// clamped to the job, empty when min > max, then (int) of both ends.
__device__ __forceinline__ bool visit_axis(float mn, float mx, float tmin, float tmax, int &lo, int &hi) {
    const float bmin = g_max(tmin, g_min(tmax, mn));
    const float bmax = g_min(tmax, g_max(tmin, mx));
    lo = (int)bmin;
    hi = (int)bmax;
    return !(bmin > bmax);
}

// Does the reference visit any pixel of [g0, g1] on this axis?  The jobs j0 .. j1 that overlap the range (the
// same for every record: the caller divides once), each with its own clamp (n: the axis' size, tile: the job size).
__device__ __forceinline__ bool axis_meets(float mn, float mx, int g0, int g1, int j0, int j1, int tile, int n) {
    for (int j = j0; j <= j1; ++j) {
        const int tmin = j * tile, tmax = min((j + 1) * tile, n) - 1;
        int lo, hi;
        if (!visit_axis(mn, mx, (float)tmin, (float)tmax, lo, hi)) continue;
        if (lo <= min(g1, tmax) && hi >= max(g0, tmin)) return true;
    }
    return false;
}

// The camera pass's instantiation k_rt_raster<false, rt_variant(shading, sky model)> of shs_rt_frame::shading: shadings 0
// to 3 are their own number, shading 4 is three instantiations, one per sky model its shader samples (RT_SKY_*: 4 to 6),
// and shadings 5 to 8 follow them; shadings 9 and 10 share one instantiation (they differ in the setup's depth alone).
// Shading 11 follows them: it does not read the sky, so it is one instantiation.
// The kernel's ladder and the launcher both go through this one mapping.
constexpr int RT_VARIANTS = 13;
constexpr int rt_variant(int shading, int sky_model) {
    return shading == 11 ? 12 : shading >= 9 ? 11 : shading >= 5 ? shading + 2 : shading == 4 ? 4 + sky_model : shading;
}
// Shadings 6 to 10 sit behind the unclipped raster: screen-linear varyings, so no fragment loses its colour to invw_sum
constexpr bool rt_unclipped(int variant) { return variant >= rt_variant(6, 0) && variant <= rt_variant(10, 0); }
// Shadings 8 to 10 (the three plain demos) hand the ZBuffer the screen row: their depth plane is stored at py * W + px
constexpr bool rt_screen_depth(int variant) { return variant >= rt_variant(8, 0) && variant <= rt_variant(10, 0); }
// k_rt_raster<true, RT_SHADOW_EDGE>: the edge-function shadow pass (<true, 0> is the barycentric one)
constexpr int RT_SHADOW_EDGE = 1;

// draw_triangle_tile_shadow_xsimd (xsimd :1078-1191) at one texel (x, y) of the job [tminx, tmaxx] x [tminy, tmaxy], over a staged RtEdgeRec:
// the depth the triangle offers the texel, or FLT_MAX (no write: the map holds at most FLT_MAX) where the job's box, an edge
// or the z range rejects it.  The box is the extent clamped to the job and then to the map (:1040-1050); inside it a row
// is walked from the box's min_x in groups of simd_lanes while a whole group fits, whose texels sum an edge function as
// A fx + (B fy + C) (:1125-1141); the row's remaining texels sum it as (A fx + B fy) + C (:1173-1175).
__device__ __forceinline__ float edge_texel(const float4 *rec, const RtParams &p, int x, int y, int tminx, int tmaxx, int tminy, int tmaxy) {
    const float4 a3 = rec[3], a4 = rec[4];   // (z2, flags, fminx, cmaxx) (fminy, cmaxy, gbx, gby)
    const int min_x = clampi(max(tminx, (int)__float_as_uint(a3.z)), 0, p.W - 1);
    const int max_x = clampi(min(tmaxx, (int)__float_as_uint(a3.w)), 0, p.W - 1);
    const int min_y = clampi(max(tminy, (int)__float_as_uint(a4.x)), 0, p.H - 1);
    const int max_y = clampi(min(tmaxy, (int)__float_as_uint(a4.y)), 0, p.H - 1);
    if (x < min_x || x > max_x || y < min_y || y > max_y) return FLT_MAX;   // (an empty box holds no texel)
    const float4 a0 = rec[0], a1 = rec[1], a2 = rec[2];   // (A0 B0 C0 A1) (B1 C1 A2 B2) (C2 inv_area z0 z1)
    // the texel's lane group starts at xs; simd_lanes is a power of two
    const int xs = min_x + ((x - min_x) & ~(p.simd_lanes - 1));
    const bool body = xs + p.simd_lanes - 1 <= max_x;
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const float e0 = body ? a0.x * fx + (a0.y * fy + a0.z) : (a0.x * fx + a0.y * fy) + a0.z;
    const float e1 = body ? a0.w * fx + (a1.x * fy + a1.y) : (a0.w * fx + a1.x * fy) + a1.y;
    const float e2 = body ? a1.z * fx + (a1.w * fy + a2.x) : (a1.z * fx + a1.w * fy) + a2.x;
    if (!(e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f)) return FLT_MAX;
    const float w0 = e1 * a2.y, w1 = e2 * a2.y, w2 = e0 * a2.y;
    const float z = (w0 * a2.z + w1 * a2.w) + w2 * a3.x;
    return (z >= 0.0f && z <= 1.0f) ? z : FLT_MAX;
}

// VARIANT: the fragment shader, a compile-time choice; of the shadow pass, the raster rule (0: the barycentric one of
// draw_triangle_tile_shadow, RT_SHADOW_EDGE: the edge functions above)
template <bool SHADOW, int VARIANT = 0>
__global__ __launch_bounds__(256) void k_rt_raster(const RtParams p) {
    constexpr bool EDGE = SHADOW && VARIANT == RT_SHADOW_EDGE;
    __shared__ float4 s_rec[RT_CHUNK * 6];
    __shared__ int32_t s_id[RT_CHUNK];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (p.W + RT_TW - 1) / RT_TW;
    const int gx0 = (int)(blockIdx.x % tiles_x) * RT_TW, gy0 = (int)(blockIdx.x / tiles_x) * RT_TH;   // screen space, y down
    const int gx1 = min(gx0 + RT_TW, p.W) - 1, gy1 = min(gy0 + RT_TH, p.H) - 1;
    const int px = gx0 + (tid & (RT_TW - 1)), py = gy0 + tid / RT_TW;
    const bool live = px < p.W && py < p.H;
    // the reference tile job this pixel lies in
    const int jx = px / p.tile_w, jy = py / p.tile_h;
    const float tminx = (float)(jx * p.tile_w), tmaxx = (float)(min((jx + 1) * p.tile_w, p.W) - 1);
    const float tminy = (float)(jy * p.tile_h), tmaxy = (float)(min((jy + 1) * p.tile_h, p.H) - 1);
    const float Px = (float)px + 0.5f, Py = (float)py + 0.5f;
    // the jobs this tile overlaps
    const int j0x = gx0 / p.tile_w, j1x = gx1 / p.tile_w, j0y = gy0 / p.tile_h, j1y = gy1 / p.tile_h;

    float best = FLT_MAX;
    int32_t sid = -1;
    float su = 0.0f, sv = 0.0f, sw = 0.0f;

    for (int base = 0; base < p.n_recs; base += RT_CHUNK) {
        // one record per lane: is any pixel of this tile visited?
        const int ri = base + tid;
        bool cand = false;
        if (ri < p.n_recs) {
            const float4 *g = reinterpret_cast<const float4 *>(&p.recs[ri]);
            const float4 q3 = g[3], q4 = g[4];   // (z2, flags, minx, maxx) (miny, maxy, gbx, gby)
            const uint32_t gbx = __float_as_uint(q4.z), gby = __float_as_uint(q4.w);
            if constexpr (EDGE) {
                // every job's box lies in the extent clamped to the map (RtEdgeRec::gbx, gby): a superset of the visits
                cand = (__float_as_uint(q3.y) & RT_VALID) && lo16(gbx) <= gx1 && hi16(gbx) >= gx0 && lo16(gby) <= gy1 && hi16(gby) >= gy0;
            } else {
                cand = (__float_as_uint(q3.y) & RT_VALID) && lo16(gbx) <= gx1 && hi16(gbx) >= gx0 && lo16(gby) <= gy1 &&
                       hi16(gby) >= gy0 && axis_meets(q3.z, q3.w, gx0, gx1, j0x, j1x, p.tile_w, p.W) &&
                       axis_meets(q4.x, q4.y, gy0, gy1, j0y, j1y, p.tile_h, p.H);
            }
        }
        const unsigned long long m = __ballot(cand);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int slot = __popcll(m & ((1ull << lane) - 1ull));
        int n_c = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) slot += s_wave[k];
            n_c += s_wave[k];
        }
        if (cand) {
            const float4 *g = reinterpret_cast<const float4 *>(&p.recs[ri]);
#pragma unroll
            for (int k = 0; k < 6; ++k) s_rec[slot * 6 + k] = g[k];
            s_id[slot] = ri;
        }
        __syncthreads();
        if constexpr (EDGE) {
            if (live) {
                // the texel's job, inclusive (xsimd :1726-1728): the same for every record
                const int jx0 = jx * p.tile_w, jx1 = min((jx + 1) * p.tile_w, p.W) - 1;
                const int jy0 = jy * p.tile_h, jy1 = min((jy + 1) * p.tile_h, p.H) - 1;
                for (int c = 0; c < n_c; ++c) {
                    const float z = edge_texel(&s_rec[c * 6], p, px, py, jx0, jx1, jy0, jy1);
                    if (z < best) best = z;
                }
            }
        } else if (live) {
            for (int c = 0; c < n_c; ++c) {
                const float4 a3 = s_rec[c * 6 + 3], a4 = s_rec[c * 6 + 4];
                int lo, hi;
                if (!visit_axis(a3.z, a3.w, tminx, tmaxx, lo, hi) || px < lo || px > hi) continue;
                if (!visit_axis(a4.x, a4.y, tminy, tmaxy, lo, hi) || py < lo || py > hi) continue;
                const float4 a0 = s_rec[c * 6 + 0], a1 = s_rec[c * 6 + 1], a2 = s_rec[c * 6 + 2];
                // barycentric_coordinate (shs_renderer.hpp:809-820)
                const float vpx = Px - a0.x, vpy = Py - a0.y;
                const float d20 = vpx * a0.z + vpy * a0.w;
                const float d21 = vpx * a1.x + vpy * a1.y;
                const float v = (a2.x * d20 - a1.w * d21) / a2.y;
                const float w = (a1.z * d21 - a1.w * d20) / a2.y;
                const float u = 1.0f - v - w;
                if (u < 0 || v < 0 || w < 0) continue;
                const float z = (u * a2.z + v * a2.w) + w * a3.x;
                if (SHADOW) {
                    if (z < 0.0f || z > 1.0f) continue;
                    if (z < best) best = z;
                } else {
                    if (!(z < best)) continue;
                    best = z;
                    if constexpr (!rt_unclipped(VARIANT)) {
                        const float4 a5 = s_rec[c * 6 + 5];   // (iw0, iw1, iw2, draw)
                        const float invw_sum = (u * a5.x + v * a5.y) + w * a5.z;
                        if (invw_sum <= 1e-8f) continue;
                    }
                    sid = s_id[c];
                    su = u; sv = v; sw = w;
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (SHADOW) {
        p.depth[(size_t)py * p.W + px] = best;
        return;
    }
    uint32_t rgba = p.clear_rgba;
    float2 vel = make_float2(0.0f, 0.0f);
    float4 pq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float spec01 = 0.0f;   // (shading 7 alone stores it)
    if constexpr (VARIANT == rt_variant(6, 0)) {
        if (sid >= 0) shade_pixel_motion<false>(p, sid, su, sv, sw, rgba, vel, pq, spec01);
    } else if constexpr (VARIANT == rt_variant(7, 0)) {
        if (sid >= 0) shade_pixel_motion<true, RtAmbient20>(p, sid, su, sv, sw, rgba, vel, pq, spec01);
    } else if constexpr (VARIANT == rt_variant(8, 0)) {
        if (sid >= 0) shade_pixel_motion<false, RtAmbient15, RT_VEL_PER_PIXEL>(p, sid, su, sv, sw, rgba, vel, pq, spec01);
    } else if constexpr (VARIANT == rt_variant(9, 0)) {
        if (sid >= 0) shade_pixel_motion<false, RtAmbient15, RT_VEL_NONE>(p, sid, su, sv, sw, rgba, vel, pq, spec01);
    } else if constexpr (VARIANT == rt_variant(1, 0)) {
        if (sid >= 0) shade_pixel_soft(p, sid, su, sv, sw, px, py, rgba, pq);   // the velocity plane stays zero
    } else if constexpr (VARIANT == rt_variant(2, 0)) {
        if (sid >= 0) shade_pixel_pbr<false>(p, sid, su, sv, sw, px, py, rgba, vel, pq);
    } else if constexpr (VARIANT == rt_variant(3, 0)) {
        if (sid >= 0) shade_pixel_pbr<true>(p, sid, su, sv, sw, px, py, rgba, vel, pq);
    } else if constexpr (VARIANT == rt_variant(11, 0)) {
        if (sid >= 0) shade_pixel_ibl_phong(p, sid, su, sv, sw, rgba, vel, pq);
    } else if constexpr (VARIANT == rt_variant(5, 0)) {
        if (sid >= 0) shade_pixel_water(p, sid, su, sv, sw, rgba, vel, pq);
    } else if constexpr (VARIANT >= rt_variant(4, RT_SKY_NONE)) {
        if (sid >= 0) shade_pixel_ibl<VARIANT - rt_variant(4, RT_SKY_NONE)>(p, sid, su, sv, sw, rgba, vel, pq);
    } else {
        if (sid >= 0) shade_pixel(p, sid, su, sv, sw, rgba, vel, pq);
    }
    const size_t o = (size_t)(p.H - 1 - py) * p.W + px;   // canvas rows
    p.color[o] = rgba;
    // the depth row: the canvas row, or for the three plain demos the screen row their test_and_set_depth(px, py, z) is
    // given (per :432, dof :563, ping :390)
    if constexpr (rt_screen_depth(VARIANT)) p.depth[(size_t)py * p.W + px] = best;
    else p.depth[o] = best;
    p.velocity[o] = vel;
    p.ids[o] = sid;
    if (p.prequant) p.prequant[o] = pq;
    if constexpr (VARIANT == rt_variant(7, 0)) p.spec[o] = spec01;
}

// shs_rt_pcss_samples: one lane per sample through the device function the raster calls
__global__ __launch_bounds__(256) void k_rt_pcss_samples(const RtPcssSamples q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    q.out[i] = pcss_shadow_factor(pcss_map(q.map, q.w, q.h, q), q.uv[2 * i], q.uv[2 * i + 1], q.z[i], q.bias[i], q.rot[i]);
}

// shs_rt_ibl_samples: one lane per direction through the device functions the raster calls
__global__ __launch_bounds__(256) void k_rt_ibl_samples(const RtIblSamples q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    const f3 d = {q.dirs[3 * i], q.dirs[3 * i + 1], q.dirs[3 * i + 2]};
    const f3 a = ibl_sample_cube(q.ibl, 0, d);
    const f3 b = ibl_sample_trilinear(q.ibl, q.ibl_mips, d, q.lod[i]);
    q.irr[3 * i] = a.x; q.irr[3 * i + 1] = a.y; q.irr[3 * i + 2] = a.z;
    q.spec[3 * i] = b.x; q.spec[3 * i + 1] = b.y; q.spec[3 * i + 2] = b.z;
}

// shs_rt_water_samples: one lane per point through the device function the raster calls
__global__ __launch_bounds__(256) void k_rt_water_samples(const RtWaterSamples q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    f3 n;
    float foam;
    water_normal_foam(q.water, f3{q.world[3 * (size_t)i], q.world[3 * (size_t)i + 1], q.world[3 * (size_t)i + 2]}, n, foam);
    q.normal[3 * (size_t)i] = n.x; q.normal[3 * (size_t)i + 1] = n.y; q.normal[3 * (size_t)i + 2] = n.z;
    q.foam[i] = foam;
}

// ---- skybox_background_pass (pbr :733-799) over the legacy sky models (sky_sample, shs_canvas_rt_shaders.hpp) ----

// One lane per pixel of the canvas rows: where the raster showed no fragment (id < 0), the sky through the pixel's
// centre (pbr :769-789, canvas x and y, y up) into the colour plane and, if there is one, the prequant plane.  Depth,
// velocity and ids are not touched.  MODEL and ENCODE are compile-time: the analytic instantiations have no gathers.
template <int MODEL, int ENCODE>
__global__ __launch_bounds__(256) void k_rt_sky(const RtSkyParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // (W, H <= 32767: W * H < 2^30)
    if (i >= (uint32_t)p.W * (uint32_t)p.H) return;
    if (p.ids[i] >= 0) return;
    const int x = (int)(i % (uint32_t)p.W), y = (int)(i / (uint32_t)p.W);
    const float fx = ((float)x + 0.5f) / (float)p.W;
    const float fy = ((float)y + 0.5f) / (float)p.H;
    const float ndc_x = fx * 2.0f - 1.0f;
    const float ndc_y = fy * 2.0f - 1.0f;
    const float kr = (ndc_x * p.aspect) * p.tan_half_fov, ku = ndc_y * p.tan_half_fov;
    const f3 dir = add3(add3(ld3(p.forward), sc3(ld3(p.right), kr)), sc3(ld3(p.up), ku));
    const f3 c = sky_sample<MODEL>(p.sky, normalize3(dir));
    float out[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if constexpr (ENCODE == RT_SKY_CLAMP) {
            // glm::clamp(c_lin, 0, 1), linear_to_srgb (whose own clamp then changes nothing), rgb01_to_color
            // (hello_ibl_skybox.cpp:598-601)
            const float s = powf(g_clamp01(out[k]), 1.0f / 2.2f);
            out[k] = g_clamp01(s) * 255.0f;
        } else {
            out[k] = encode_reinhard(out[k], p.exposure);
        }
    }
    p.color[i] = byte_x86(out[0]) | (byte_x86(out[1]) << 8) | (byte_x86(out[2]) << 16) | 0xff000000u;
    if (p.prequant) p.prequant[i] = make_float4(out[0], out[1], out[2], 1.0f);
}

// shs_rt_sky_samples: one lane per direction through the device function the background pass calls
template <int MODEL>
__global__ __launch_bounds__(256) void k_rt_sky_samples(const RtSkySamples q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    const f3 c = sky_sample<MODEL>(q.sky, ld3(q.dirs + 3 * (size_t)i));
    q.out[3 * (size_t)i] = c.x; q.out[3 * (size_t)i + 1] = c.y; q.out[3 * (size_t)i + 2] = c.z;
}

}  // namespace
}  // namespace shs_dev

namespace shs_internal {

hipError_t launch_pcss_samples(const shs_dev::RtPcssSamples &q, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(shs_dev::k_rt_pcss_samples, dim3((q.n + 255) / 256), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_ibl_samples(const shs_dev::RtIblSamples &q, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(shs_dev::k_rt_ibl_samples, dim3((q.n + 255) / 256), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_water_samples(const shs_dev::RtWaterSamples &q, hipStream_t s) {
    if (q.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(shs_dev::k_rt_water_samples, dim3((q.n + 255) / 256), dim3(256), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_canvas_rt_sky(const shs_dev::RtSkyParams &p, int model, int encode, hipStream_t s) {
    using namespace shs_dev;
    const dim3 grid(((uint32_t)p.W * (uint32_t)p.H + 255u) / 256u), block(256);
    const bool clamp = encode == RT_SKY_CLAMP;
    if (model == RT_SKY_CUBEMAP) {
        if (clamp) hipLaunchKernelGGL((k_rt_sky<RT_SKY_CUBEMAP, RT_SKY_CLAMP>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_rt_sky<RT_SKY_CUBEMAP, RT_SKY_REINHARD>), grid, block, 0, s, p);
    } else {
        if (clamp) hipLaunchKernelGGL((k_rt_sky<RT_SKY_ANALYTIC, RT_SKY_CLAMP>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((k_rt_sky<RT_SKY_ANALYTIC, RT_SKY_REINHARD>), grid, block, 0, s, p);
    }
    return hipGetLastError();
}

hipError_t launch_sky_samples(const shs_dev::RtSkySamples &q, int model, hipStream_t s) {
    using namespace shs_dev;
    if (q.n <= 0) return hipSuccess;
    const dim3 grid((q.n + 255) / 256), block(256);
    if (model == RT_SKY_CUBEMAP) hipLaunchKernelGGL(k_rt_sky_samples<RT_SKY_CUBEMAP>, grid, block, 0, s, q);
    else hipLaunchKernelGGL(k_rt_sky_samples<RT_SKY_ANALYTIC>, grid, block, 0, s, q);
    return hipGetLastError();
}

// k_rt_raster<false, variant> for a run-time variant: every V of the list is instantiated, the one that matches is
// launched.  false: none matched.
template <int V>
static void launch_camera_variant(int tiles, hipStream_t s, const shs_dev::RtParams &p) {
    hipLaunchKernelGGL((shs_dev::k_rt_raster<false, V>), dim3(tiles), dim3(256), 0, s, p);
}
template <int... V>
static bool launch_camera_raster(int variant, std::integer_sequence<int, V...>, int tiles, hipStream_t s, const shs_dev::RtParams &p) {
    return ((variant == V ? (launch_camera_variant<V>(tiles, s, p), true) : false) || ...);
}

hipError_t launch_canvas_rt(const shs_dev::RtParams &p, bool shadow_pass, int shading, hipStream_t s, int sky_model, bool edge_shadow) {
    using namespace shs_dev;
    if (p.n_tris > 0) {
        const int grid = (p.n_tris + 255) / 256;
        if (shadow_pass && edge_shadow) hipLaunchKernelGGL(k_rt_setup_edge, dim3(grid), dim3(256), 0, s, p);
        else if (shadow_pass) hipLaunchKernelGGL(k_rt_setup<true>, dim3(grid), dim3(256), 0, s, p);
        else if (shading == 10) hipLaunchKernelGGL(k_rt_setup_motion<true>, dim3(grid), dim3(256), 0, s, p);
        else if (rt_unclipped(rt_variant(shading, sky_model))) hipLaunchKernelGGL(k_rt_setup_motion<false>, dim3(grid), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(k_rt_setup<false>, dim3(grid), dim3(256), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int tiles = ((p.W + RT_TW - 1) / RT_TW) * ((p.H + RT_TH - 1) / RT_TH);
    if (shadow_pass && edge_shadow) hipLaunchKernelGGL((k_rt_raster<true, RT_SHADOW_EDGE>), dim3(tiles), dim3(256), 0, s, p);
    else if (shadow_pass) hipLaunchKernelGGL(k_rt_raster<true>, dim3(tiles), dim3(256), 0, s, p);
    else if (!launch_camera_raster(rt_variant(shading, sky_model), std::make_integer_sequence<int, RT_VARIANTS>{}, tiles, s, p))
        return hipErrorInvalidValue;   // (no such instantiation: the entries of shs_abi_canvas_rt.cpp reject the shading)
    return hipGetLastError();
}

}  // namespace shs_internal
