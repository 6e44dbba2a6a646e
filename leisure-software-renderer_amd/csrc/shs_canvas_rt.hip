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
//          k_rt_raster<false, 4 + sky model>, launched by shs_rt_render_skybox_ibl, is shade_pixel_ibl<SKY>: three
//          instantiations (no sky, AnalyticSky, CubeMapSky), of which only the last has gathers.
// and for hello_water.cpp ("water :line"), whose PASS0 / PASS1 rasters, vertex shader, velocity and shadow_uvz_from_world
// are the hard demo's text (DESIGN.md section 8 lists the routines compared):
//   shading 5  two fragment shaders in one camera pass, chosen per draw (shs_rt_water_draw): fragment_shader_full
//          (water :938-994, the "atmosphere" shader: Blinn-Phong under a sky-coloured ambient term, fog, Reinhard, gamma)
//          and fragment_shader_water (water :1000-1097: a procedural flow normal and foam from water_flow_normal_and_foam
//          :862-930 over hash12 / noise2 / fbm2, Schlick's fresnel over a planar reflection read from the context's
//          reflection canvas, fog).  Both round to the byte where the other shadings truncate.  Their shadow lookup
//          (water :716-751) is not the hard demo's: shadow_factor_water.  k_rt_raster<false, RT_SHADING_WATER>,
//          launched by shs_rt_render_water, is shade_pixel_water.
//   the background  skybox_background_pass (pbr :733-799; the same routine in hello_pbr_light_shafts.cpp and
//          hello_ibl_skybox.cpp) over the legacy AnalyticSky / CubeMapSky of hello-shs-renderer/shs_renderer.hpp:
//          k_rt_sky<MODEL, ENCODE>, a pass of its own after k_rt_raster when a sky is bound (shs_rt_set_sky), which
//          colours the pixels whose id is -1.  The reference draws the sky first and the triangles over it.
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
#include <float.h>
#include <limits.h>

#include "shs_canvas_rt_internal.hpp"
#include "shs_device.hpp"
#include "../../include/shs_gpu.h"

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
// bbox over the corners that are not NaN.  false: the sub-triangle draws nothing.
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
    if (fabsf(area) < 1e-8f) return false;
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
        RtVary &v = p.vary[id];
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
    const float *nrm = dr.nrm + 9 * (size_t)local;
    const float *uv = dr.uv ? dr.uv + 6 * (size_t)local : nullptr;
    Vy in[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // vertex_shader_full :602-620
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

// ---- k_rt_raster -----------------------------------------------------------------------------------

// (int)f as the reference's x86-64 build converts it (cvttss2si: NaN and out-of-range give INT_MIN)
__device__ __forceinline__ int int_x86(float f) {
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (int)std::lround(x) of a product that is NaN or lies in [0, n - 1] (as the legacy
// texture path's nearest_coord): halves away from zero; glibc's lroundf(NaN) is LONG_MIN, whose (int) is 0
__device__ __forceinline__ int lround_x86(float x) {
    if (!(x == x)) return 0;
    const float t = truncf(x);
    return (int)t + ((x - t >= 0.5f) ? 1 : 0);
}
__device__ __forceinline__ float pow64(float x) {
    double d = (double)x;
#pragma unroll
    for (int i = 0; i < 6; ++i) d = d * d;
    return (float)d;
}
__device__ __forceinline__ uint32_t byte_x86(float x) { return x == x ? (uint32_t)(int32_t)x & 0xffu : 0u; }

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

__device__ __forceinline__ float sm_sample(const RtParams &p, int x, int y) {   // ShadowMap::sample :637-640
    if (x < 0 || x >= p.sw || y < 0 || y >= p.sh) return FLT_MAX;
    return p.shadow[(size_t)y * p.sw + x];
}

// shadow_uvz_from_world, shadow_compare / shadow_factor_pcf_2x2 (:628-693) as fragment_shader_full calls them
__device__ float shadow_factor(const RtParams &p, f3 wp, float ndotl) {
    float cx, cy, cz, cw;
    m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
    if (fabsf(cw) < 1e-6f) return 1.0f;
    const float nx = cx / cw, ny = cy / cw, z = cz / cw;
    if (z < 0.0f || z > 1.0f) return 1.0f;
    const float u = nx * 0.5f + 0.5f;
    const float v = 1.0f - (ny * 0.5f + 0.5f);
    const float slope = 1.0f - g_clamp01(ndotl);
    const float bias = p.bias_base + p.bias_slope * slope;
    if (!(p.flags & SHS_RT_PCF)) {
        if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
        const int x = lround_x86(u * (float)(p.sw - 1));
        const int y = lround_x86(v * (float)(p.sh - 1));
        const float d = sm_sample(p, x, y);
        if (d == FLT_MAX) return 1.0f;
        return (z <= d + bias) ? 1.0f : 0.0f;
    }
    const float fx = u * (float)(p.sw - 1);
    const float fy = v * (float)(p.sh - 1);
    const int x0 = clampi(int_x86(floorf(fx)), 0, p.sw - 1);
    const int y0 = clampi(int_x86(floorf(fy)), 0, p.sh - 1);
    const int x1 = clampi(x0 + 1, 0, p.sw - 1);
    const int y1 = clampi(y0 + 1, 0, p.sh - 1);
    const float s00 = (z <= sm_sample(p, x0, y0) + bias) ? 1.0f : 0.0f;
    const float s10 = (z <= sm_sample(p, x1, y0) + bias) ? 1.0f : 0.0f;
    const float s01 = (z <= sm_sample(p, x0, y1) + bias) ? 1.0f : 0.0f;
    const float s11 = (z <= sm_sample(p, x1, y1) + bias) ? 1.0f : 0.0f;
    return 0.25f * (((s00 + s10) + s01) + s11);
}

// ---- hello_shadow_mapping_soft.cpp: the PCSS shadow factor ------------------------------------------

// POISSON_32 (soft :267-301); a tap's index is wave-uniform, so these are scalar loads
__constant__ float2 c_poisson32[32] = {
    {-0.613392f, 0.617481f},  {0.170019f, -0.040254f},  {-0.299417f, 0.791925f},  {0.645680f, 0.493210f},
    {-0.651784f, 0.717887f},  {0.421003f, 0.027070f},   {-0.817194f, -0.271096f}, {-0.705374f, -0.668203f},
    {0.977050f, -0.108615f},  {0.063326f, 0.142369f},   {0.203528f, 0.214331f},   {-0.667531f, 0.326090f},
    {-0.098422f, -0.295755f}, {-0.885922f, 0.215369f},  {0.566637f, 0.605213f},   {0.039766f, -0.396100f},
    {0.751946f, 0.453352f},   {0.078707f, -0.715323f},  {-0.075838f, -0.529344f}, {0.724479f, -0.580798f},
    {0.222999f, -0.215125f},  {-0.467574f, -0.405438f}, {-0.248268f, -0.814753f}, {0.354411f, -0.887570f},
    {0.175817f, 0.382366f},   {0.487472f, -0.063082f},  {-0.084078f, 0.898312f},  {0.488876f, -0.783441f},
    {0.470016f, 0.217933f},   {-0.696890f, -0.549791f}, {-0.149693f, 0.605762f},  {0.034211f, 0.979980f}};

struct PcssMap {   // the soft demo's file-local ShadowMap (:191-225) and the constants of shs_rt_pcss
    const float *depth;
    int w, h;
    float light, search, fmin, fmax, eps;
    int blockers, taps;
};

// shadow_sample_depth_uv (soft :252-261) over ShadowMap::sample (:219-224), which clamps: a uv outside [0, 1]
// is FLT_MAX (empty) without a read; a NaN passes the range test and reads texel 0 of its axis.  The load is
// unconditional at a clamped address, so the taps of a loop are independent gathers the compiler may batch.
__device__ __forceinline__ float pcss_tap(const PcssMap &m, float u, float v) {
    const bool off = u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f;
    const int x = clampi(lround_x86(u * (float)(m.w - 1)), 0, m.w - 1);
    const int y = clampi(lround_x86(v * (float)(m.h - 1)), 0, m.h - 1);
    const float d = m.depth[(size_t)y * m.w + x];
    return off ? FLT_MAX : d;
}

// pcss_shadow_factor (soft :333-445).  rot: {cos(ang), sin(ang), cos(ang2), sin(ang2)} of the screen pixel, the
// host libm's values; rotate2's multiplies and add / subtract run here.
__device__ float pcss_shadow_factor(const PcssMap &m, float u, float v, float z, float bias, float4 rot) {
    if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
    if (pcss_tap(m, u, v) == FLT_MAX) return 1.0f;
    const float tsu = 1.0f / (float)m.w, tsv = 1.0f / (float)m.h;
    const float sru = m.search * tsu, srv = m.search * tsv;
    const float ztest = z - bias;
    float bsum = 0.0f;
    int bcnt = 0;
#pragma unroll 4
    for (int i = 0; i < m.blockers; ++i) {
        const float2 o = c_poisson32[i & 31];
        const float ox = rot.x * o.x - rot.y * o.y, oy = rot.y * o.x + rot.x * o.y;
        const float d = pcss_tap(m, u + ox * sru, v + oy * srv);
        const bool blocks = d != FLT_MAX && d < ztest;
        bsum = blocks ? bsum + d : bsum;
        bcnt += blocks ? 1 : 0;
    }
    if (bcnt <= 0) return 1.0f;
    const float avg = bsum / (float)bcnt;
    const float zb = g_max(m.eps, avg), zr = g_max(m.eps, z);   // std::max(a, b): (a < b) ? b : a
    const float ratio = g_max(0.0f, (zr - zb) / zb);
    const float fuu = m.light * ratio, fuv = m.light * ratio;
    float ft = 0.5f * (fuu / tsu + fuv / tsv);
    ft = (ft < m.fmin) ? m.fmin : (ft > m.fmax ? m.fmax : ft);  // clampf :127-132
    const float fru = ft * tsu, frv = ft * tsv;
    if (m.taps <= 0) return 1.0f;
    float lit = 0.0f;
#pragma unroll 4
    for (int i = 0; i < m.taps; ++i) {
        const float2 o = c_poisson32[i & 31];
        const float ox = rot.z * o.x - rot.w * o.y, oy = rot.w * o.x + rot.z * o.y;
        const float d = pcss_tap(m, u + ox * fru, v + oy * frv);
        lit += (d == FLT_MAX || z <= d + bias) ? 1.0f : 0.0f;   // empty and off-map taps count as lit
    }
    return lit / (float)m.taps;
}

// Canvas::clip_to_screen's x and y of an interpolated clip position
__device__ __forceinline__ void to_screen(const RtParams &p, float x, float y, float w, float &sx, float &sy) {
    const float nx = x / w, ny = y / w;
    sx = (nx + 1.0f) * 0.5f * (float)(p.W - 1);
    sy = (1.0f - ny) * 0.5f * (float)(p.H - 1);
}

// The shown fragment of a camera-pass pixel (:971-1013) at the shading sub-triangle's barycentrics.
__device__ void shade_pixel(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const RtRec &r = p.recs[id];
    const RtVary &y = p.vary[id];
    const RtDrawGPU &dr = p.draws[r.draw];
    const float iw0 = r.iw0, iw1 = r.iw1, iw2 = r.iw2;
    const float invw_sum = (u * iw0 + v * iw1) + w * iw2;
    float pos[4], prev[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pos[k] = (u * y.pos[k] + v * y.pos[4 + k]) + w * y.pos[8 + k];
        prev[k] = (u * y.prev[k] + v * y.prev[4 + k]) + w * y.prev[8 + k];
    }
    const f3 nsum = {(u * y.nrm[0] + v * y.nrm[3]) + w * y.nrm[6], (u * y.nrm[1] + v * y.nrm[4]) + w * y.nrm[7],
                     (u * y.nrm[2] + v * y.nrm[5]) + w * y.nrm[8]};
    const f3 in_normal = normalize3(nsum);
    f3 wp;
    wp.x = ((u * (y.world[0] * iw0) + v * (y.world[3] * iw1)) + w * (y.world[6] * iw2)) / invw_sum;
    wp.y = ((u * (y.world[1] * iw0) + v * (y.world[4] * iw1)) + w * (y.world[7] * iw2)) / invw_sum;
    wp.z = ((u * (y.world[2] * iw0) + v * (y.world[5] * iw1)) + w * (y.world[8] * iw2)) / invw_sum;
    const float tu = ((u * (y.uv[0] * iw0) + v * (y.uv[2] * iw1)) + w * (y.uv[4] * iw2)) / invw_sum;
    const float tv = ((u * (y.uv[1] * iw0) + v * (y.uv[3] * iw1)) + w * (y.uv[5] * iw2)) / invw_sum;
    // velocity :1002-1011
    float csx, csy, psx, psy;
    to_screen(p, pos[0], pos[1], pos[3], csx, csy);
    to_screen(p, prev[0], prev[1], prev[3], psx, psy);
    float vx = csx - psx, vy = -(csy - psy);
    const float len = sqrtf(vx * vx + vy * vy);
    if (len > p.max_velocity && len > 1e-6f) {
        const float s = p.max_velocity / len;
        vx *= s;
        vy *= s;
    }
    vel = make_float2(vx, vy);
    // fragment_shader_full :699-750
    const f3 N = normalize3(in_normal);
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float ambient = 0.18f * 1.0f;
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    f3 base = {dr.colf[0] / 255.0f, dr.colf[1] / 255.0f, dr.colf[2] / 255.0f};
    if (dr.texels) {
        // sample_nearest (shs_renderer.hpp:367-377)
        const float su = (tu < 0.0f) ? 0.0f : (tu > 1.0f ? 1.0f : tu);
        const float sv = (tv < 0.0f) ? 0.0f : (tv > 1.0f ? 1.0f : tv);
        const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
        const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
        const uint32_t tc = dr.texels[(size_t)yy * dr.tw + x];
        base = f3{(float)(tc & 0xffu) / 255.0f, (float)((tc >> 8) & 0xffu) / 255.0f, (float)((tc >> 16) & 0xffu) / 255.0f};
    }
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    const float lit = ambient + shadow * (diffuse + specular);
    const float pr = g_clamp01(lit * base.x) * 255, pg = g_clamp01(lit * base.y) * 255, pb = g_clamp01(lit * base.z) * 255;
    rgba = byte_x86(pr) | (byte_x86(pg) << 8) | (byte_x86(pb) << 16) | 0xff000000u;
    pq = make_float4(pr, pg, pb, shadow);
}

// The shown fragment of hello_shadow_mapping_soft.cpp's camera pass (soft :961-979) at screen pixel (px, py):
// the same interpolation without position / prev_position (that demo has no motion buffer), then
// fragment_shader_softshadow (soft :991-1040) -- not the hard shader with other constants: the ambient and the
// diffuse term are multiplied by the base colour, the specular term is not.
__device__ void shade_pixel_soft(const RtParams &p, int32_t id, float u, float v, float w, int px, int py, uint32_t &rgba, float4 &pq) {
    const RtRec &r = p.recs[id];
    const RtVary &y = p.vary[id];
    const RtDrawGPU &dr = p.draws[r.draw];
    const float iw0 = r.iw0, iw1 = r.iw1, iw2 = r.iw2;
    const float invw_sum = (u * iw0 + v * iw1) + w * iw2;
    const f3 nsum = {(u * y.nrm[0] + v * y.nrm[3]) + w * y.nrm[6], (u * y.nrm[1] + v * y.nrm[4]) + w * y.nrm[7],
                     (u * y.nrm[2] + v * y.nrm[5]) + w * y.nrm[8]};
    const f3 in_normal = normalize3(nsum);
    f3 wp;
    wp.x = ((u * (y.world[0] * iw0) + v * (y.world[3] * iw1)) + w * (y.world[6] * iw2)) / invw_sum;
    wp.y = ((u * (y.world[1] * iw0) + v * (y.world[4] * iw1)) + w * (y.world[7] * iw2)) / invw_sum;
    wp.z = ((u * (y.world[2] * iw0) + v * (y.world[5] * iw1)) + w * (y.world[8] * iw2)) / invw_sum;
    const float tu = ((u * (y.uv[0] * iw0) + v * (y.uv[2] * iw1)) + w * (y.uv[4] * iw2)) / invw_sum;
    const float tv = ((u * (y.uv[1] * iw0) + v * (y.uv[3] * iw1)) + w * (y.uv[5] * iw2)) / invw_sum;
    const f3 N = normalize3(in_normal);
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    f3 base = {dr.colf[0] / 255.0f, dr.colf[1] / 255.0f, dr.colf[2] / 255.0f};
    if (dr.texels) {
        // sample_nearest (soft :167-186)
        const float su = (tu < 0.0f) ? 0.0f : (tu > 1.0f ? 1.0f : tu);
        const float sv = (tv < 0.0f) ? 0.0f : (tv > 1.0f ? 1.0f : tv);
        const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
        const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
        const uint32_t tc = dr.texels[(size_t)yy * dr.tw + x];
        base = f3{(float)(tc & 0xffu) / 255.0f, (float)((tc >> 8) & 0xffu) / 255.0f, (float)((tc >> 16) & 0xffu) / 255.0f};
    }
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    float shadow = 1.0f;
    if (p.shadow) {
        // shadow_uvz_from_world (soft :231-250)
        float cx, cy, cz, cw;
        m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
        if (!(fabsf(cw) < 1e-6f)) {
            const float nx = cx / cw, ny = cy / cw, z = cz / cw;
            if (!(z < 0.0f || z > 1.0f)) {
                const float su = nx * 0.5f + 0.5f;
                const float sv = 1.0f - (ny * 0.5f + 0.5f);
                const float slope = 1.0f - g_clamp01(ndotl);
                const float bias = p.bias_base + p.bias_slope * slope;
                const PcssMap m = {p.shadow, p.sw, p.sh, p.pcss_light, p.pcss_search, p.pcss_min, p.pcss_max, p.pcss_eps,
                                   p.pcss_blockers, p.pcss_taps};
                shadow = pcss_shadow_factor(m, su, sv, z, bias, p.rot[(size_t)py * p.W + px]);
            }
        }
    }
    // amb = 0.22 * baseColor; direct = shadow * (diffuse * baseColor + specular); clamp(amb + direct)
    const float pr = g_clamp01(0.22f * base.x + shadow * (diffuse * base.x + specular)) * 255;
    const float pg = g_clamp01(0.22f * base.y + shadow * (diffuse * base.y + specular)) * 255;
    const float pb = g_clamp01(0.22f * base.z + shadow * (diffuse * base.z + specular)) * 255;
    rgba = byte_x86(pr) | (byte_x86(pg) << 8) | (byte_x86(pb) << 16) | 0xff000000u;
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_pbr.cpp: image-based lighting and the GGX fragment shader ("pbr :line") ------------------

// sample_face_bilinear_linear_vec (shs/resources/ibl.hpp:215-234) over a level of the IBL allocation (RtParams::ibl).
// std::clamp keeps a NaN; (int)std::floor is the x86-64 conversion, so a NaN coordinate reads texel 0 and 1.
__device__ f3 ibl_sample_face(const float4 *ibl, int first, int size, int face, float u, float v) {
    u = (u < 0.0f) ? 0.0f : (1.0f < u ? 1.0f : u);
    v = (v < 0.0f) ? 0.0f : (1.0f < v ? 1.0f : v);
    const float fx = u * (float)(size - 1);
    const float fy = v * (float)(size - 1);
    const int x0 = clampi(int_x86(floorf(fx)), 0, size - 1);
    const int y0 = clampi(int_x86(floorf(fy)), 0, size - 1);
    const int x1 = clampi(x0 + 1, 0, size - 1);
    const int y1 = clampi(y0 + 1, 0, size - 1);
    const float tx = fx - (float)x0;
    const float ty = fy - (float)y0;
    const float4 *f = ibl + first + (size_t)face * size * size;
    const float4 c00 = f[y0 * size + x0], c10 = f[y0 * size + x1], c01 = f[y1 * size + x0], c11 = f[y1 * size + x1];
    // glm::mix(x, y, a): x * (1 - a) + y * a
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const f3 cx0 = {c00.x * ux + c10.x * tx, c00.y * ux + c10.y * tx, c00.z * ux + c10.z * tx};
    const f3 cx1 = {c01.x * ux + c11.x * tx, c01.y * ux + c11.y * tx, c01.z * ux + c11.z * tx};
    return {cx0.x * uy + cx1.x * ty, cx0.y * uy + cx1.y * ty, cx0.z * uy + cx1.z * ty};
}

// sample_cubemap_linear_vec (ibl.hpp:236-270) of level `level` (0: irradiance, 1 + m: specular mip m)
__device__ f3 ibl_sample_cube(const float4 *ibl, int level, f3 d) {
    const int4 hd = reinterpret_cast<const int4 *>(ibl)[level];   // {first texel, size}
    const float len = sqrtf(dot3(d, d));
    if (len < 1e-8f) return {0.0f, 0.0f, 0.0f};
    d = {d.x / len, d.y / len, d.z / len};
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float u, v;
    if (ax >= ay && ax >= az) {
        if (d.x > 0.0f) { face = 0; u = -d.z / ax; v = d.y / ax; }
        else            { face = 1; u = d.z / ax; v = d.y / ax; }
    } else if (ay >= ax && ay >= az) {
        if (d.y > 0.0f) { face = 2; u = d.x / ay; v = -d.z / ay; }
        else            { face = 3; u = d.x / ay; v = d.z / ay; }
    } else {
        if (d.z > 0.0f) { face = 4; u = d.x / az; v = d.y / az; }
        else            { face = 5; u = -d.x / az; v = d.y / az; }
    }
    u = 0.5f * (u + 1.0f);
    v = 0.5f * (v + 1.0f);
    return ibl_sample_face(ibl, hd.x, hd.y, face, u, v);
}

// sample_prefiltered_spec_trilinear (ibl.hpp:272-286); a NaN lod passes std::clamp and converts to INT_MIN, whose
// mip index is clamped here (the reference would index out of its vector)
__device__ f3 ibl_sample_trilinear(const float4 *ibl, int mips, f3 d, float lod) {
    const float mmax = (float)(mips - 1);
    lod = (lod < 0.0f) ? 0.0f : (mmax < lod ? mmax : lod);
    const int m0 = clampi(int_x86(floorf(lod)), 0, mips - 1);
    const int m1 = min(m0 + 1, mips - 1);
    const float t = lod - (float)m0;
    const f3 c0 = ibl_sample_cube(ibl, 1 + m0, d);
    const f3 c1 = ibl_sample_cube(ibl, 1 + m1, d);
    const float s = 1.0f - t;
    return {c0.x * s + c1.x * t, c0.y * s + c1.y * t, c0.z * s + c1.z * t};
}

__device__ __forceinline__ float saturate(float v) { return (v < 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v); }

// One channel's way to the screen in hello_pbr.cpp (fragment_shader_pbr :722-726, skybox_background_pass :785-789):
// the exposure, tonemap_reinhard, linear_to_srgb, and rgb01_to_color up to the truncation: the channel * 255.
__device__ __forceinline__ float encode_reinhard(float x, float exposure) {
    x = x * exposure;
    x = x / (1.0f + x);                        // tonemap_reinhard
    x = powf(g_clamp01(x), 1.0f / 2.2f);       // linear_to_srgb
    return g_clamp01(x) * 255.0f;              // rgb01_to_color
}

// The shown fragment of hello_pbr.cpp's camera pass (pbr :986-1035, the hard demo's interpolation and velocity)
// through fragment_shader_pbr (pbr :627-727): Cook-Torrance GGX under the hard demo's shadow lookup, plus the
// irradiance and prefiltered-specular IBL.  The direct term is finished before the IBL gathers start.
// SOFT: hello_pbr_light_shafts.cpp's fragment_shader_pbr (shafts :768-850) at screen pixel (px, py) instead -- the same
// text but for the shadow factor, which is pcss_shadow_factor over the bias of shafts :814-815 (SHS_RT_PCF is not read),
// and the missing minimum ambient.  Its ShadowMap is the legacy one, FLT_MAX outside, where the soft demo's clamps:
// pcss_tap never looks outside.
template <bool SOFT>
__device__ void shade_pixel_pbr(const RtParams &p, int32_t id, float u, float v, float w, int px, int py, uint32_t &rgba, float2 &vel,
                                float4 &pq) {
    const RtRec &r = p.recs[id];
    const RtVary &y = p.vary[id];
    const RtDrawGPU &dr = p.draws[r.draw];
    const float iw0 = r.iw0, iw1 = r.iw1, iw2 = r.iw2;
    const float invw_sum = (u * iw0 + v * iw1) + w * iw2;
    {   // velocity (pbr :1017-1026)
        float pos[4], prev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pos[k] = (u * y.pos[k] + v * y.pos[4 + k]) + w * y.pos[8 + k];
            prev[k] = (u * y.prev[k] + v * y.prev[4 + k]) + w * y.prev[8 + k];
        }
        float csx, csy, psx, psy;
        to_screen(p, pos[0], pos[1], pos[3], csx, csy);
        to_screen(p, prev[0], prev[1], prev[3], psx, psy);
        float vx = csx - psx, vy = -(csy - psy);
        const float len = sqrtf(vx * vx + vy * vy);
        if (len > p.max_velocity && len > 1e-6f) {
            const float s = p.max_velocity / len;
            vx *= s;
            vy *= s;
        }
        vel = make_float2(vx, vy);
    }
    const f3 nsum = {(u * y.nrm[0] + v * y.nrm[3]) + w * y.nrm[6], (u * y.nrm[1] + v * y.nrm[4]) + w * y.nrm[7],
                     (u * y.nrm[2] + v * y.nrm[5]) + w * y.nrm[8]};
    const f3 in_normal = normalize3(nsum);
    f3 wp;
    wp.x = ((u * (y.world[0] * iw0) + v * (y.world[3] * iw1)) + w * (y.world[6] * iw2)) / invw_sum;
    wp.y = ((u * (y.world[1] * iw0) + v * (y.world[4] * iw1)) + w * (y.world[7] * iw2)) / invw_sum;
    wp.z = ((u * (y.world[2] * iw0) + v * (y.world[5] * iw1)) + w * (y.world[8] * iw2)) / invw_sum;
    const f3 N = normalize3(in_normal);
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 H = normalize3(add3(V, L));
    const float ndotl = dot3(N, L);
    const float NoV = g_max(0.0f, dot3(N, V)), NoL = g_max(0.0f, ndotl), NoH = g_max(0.0f, dot3(N, H));
    const float4 m0 = reinterpret_cast<const float4 *>(&p.pbr_draws[r.draw])[0];   // base rgb, metallic
    const float4 m1 = reinterpret_cast<const float4 *>(&p.pbr_draws[r.draw])[1];   // roughness, ao, ibl diffuse, ibl specular
    f3 base = {m0.x, m0.y, m0.z};
    if (dr.texels) {
        // sample_nearest_srgb = sample_nearest (shs_renderer.hpp:367-381), then srgb_to_linear of the bytes
        const float tu = ((u * (y.uv[0] * iw0) + v * (y.uv[2] * iw1)) + w * (y.uv[4] * iw2)) / invw_sum;
        const float tv = ((u * (y.uv[1] * iw0) + v * (y.uv[3] * iw1)) + w * (y.uv[5] * iw2)) / invw_sum;
        const float su = saturate(tu), sv = saturate(tv);
        const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
        const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
        const uint32_t tc = dr.texels[(size_t)yy * dr.tw + x];
        base = f3{p.srgb_lut[tc & 0xffu], p.srgb_lut[(tc >> 8) & 0xffu], p.srgb_lut[(tc >> 16) & 0xffu]};
    }
    const float metallic = m0.w, roughness = m1.x, ao = m1.y;
    const float om = 1.0f - metallic;
    const f3 F0 = {0.04f * om + base.x * metallic, 0.04f * om + base.y * metallic, 0.04f * om + base.z * metallic};
    // fresnel_schlick (pbr :242-249), then the blue attenuation
    const float fx = 1.0f - saturate(NoV);
    const float fx2 = fx * fx;
    const float fx5 = fx2 * fx2 * fx;
    const f3 Fr = {(F0.x + (1.0f - F0.x) * fx5) * 1.0f, (F0.y + (1.0f - F0.y) * fx5) * 0.96f, (F0.z + (1.0f - F0.z) * fx5) * 0.90f};
    const f3 kd = {(1.0f - Fr.x) * om, (1.0f - Fr.y) * om, (1.0f - Fr.z) * om};
    // ndf_ggx (:251-257), g_smith over g_schlick_ggx (:259-277; its second clamp of the roughness changes nothing)
    const float PI = 3.14159265358979323846f;
    const float alpha = roughness * roughness;
    const float sh = saturate(NoH);
    const float a2 = alpha * alpha;
    const float dd = (sh * sh) * (a2 - 1.0f) + 1.0f;
    const float D = a2 / (PI * dd * dd);
    const float r1 = roughness + 1.0f;
    const float k = (r1 * r1) / 8.0f;
    const float sv_ = saturate(NoV), sl_ = saturate(NoL);
    const float G = (sv_ / (sv_ * (1.0f - k) + k)) * (sl_ / (sl_ * (1.0f - k) + k));
    const float DG = D * G;
    const float den = g_max(1e-6f, 4.0f * NoV * NoL);
    float shadow = 1.0f;
    if constexpr (SOFT) {
        if (p.shadow) {
            // shadow_uvz_from_world (shafts :558-576)
            float cx, cy, cz, cw;
            m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
            if (!(fabsf(cw) < 1e-6f)) {
                const float nx = cx / cw, ny = cy / cw, z = cz / cw;
                if (!(z < 0.0f || z > 1.0f)) {
                    const float su = nx * 0.5f + 0.5f;
                    const float sv = 1.0f - (ny * 0.5f + 0.5f);
                    const float slope = 1.0f - g_clamp01(ndotl);
                    const float bias = p.bias_base + p.bias_slope * slope;
                    const PcssMap m = {p.shadow, p.sw, p.sh, p.pcss_light, p.pcss_search, p.pcss_min, p.pcss_max, p.pcss_eps,
                                       p.pcss_blockers, p.pcss_taps};
                    shadow = pcss_shadow_factor(m, su, sv, z, bias, p.rot[(size_t)py * p.W + px]);
                }
            }
        }
    } else {
        if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    }
    f3 c;
    {
        const float ipi = 1.0f / PI;
        const float I = p.pbr_intensity;
        c.x = ((((kd.x * base.x) * ipi + (DG * Fr.x) / den) * I) * NoL) * shadow;
        c.y = ((((kd.y * base.y) * ipi + (DG * Fr.y) / den) * I) * NoL) * shadow;
        c.z = ((((kd.z * base.z) * ipi + (DG * Fr.z) / den) * I) * NoL) * shadow;
    }
    f3 ibl = {0.0f, 0.0f, 0.0f};
    if (p.ibl) {
        const f3 irr = ibl_sample_cube(p.ibl, 0, N);
        // glm::reflect(-V, N): I - N * dot(N, I) * 2
        const f3 I = {-V.x, -V.y, -V.z};
        const float ni = dot3(N, I);
        const f3 R = {I.x - N.x * ni * 2.0f, I.y - N.y * ni * 2.0f, I.z - N.z * ni * 2.0f};
        const float lod = roughness * (float)(p.ibl_mips - 1);
        const f3 pre = ibl_sample_trilinear(p.ibl, p.ibl_mips, R, lod);
        ibl.x = ((irr.x * base.x) * kd.x) * m1.z + (pre.x * Fr.x) * m1.w;
        ibl.y = ((irr.y * base.y) * kd.y) * m1.z + (pre.y * Fr.y) * m1.w;
        ibl.z = ((irr.z * base.z) * kd.z) * m1.z + (pre.z * Fr.z) * m1.w;
    }
    float out[3] = {c.x + ibl.x * ao, c.y + ibl.y * ao, c.z + ibl.z * ao};
    const float bs[3] = {base.x, base.y, base.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float x = out[i];
        if constexpr (!SOFT) x = x + (bs[i] * 0.03f) * ao;   // the minimum ambient (hello_pbr.cpp alone)
        out[i] = encode_reinhard(x, p.pbr_exposure);
    }
    rgba = byte_x86(out[0]) | (byte_x86(out[1]) << 8) | (byte_x86(out[2]) << 16) | 0xff000000u;
    pq = make_float4(out[0], out[1], out[2], shadow);
}

// ---- hello_ibl_skybox.cpp: the sky-lit Blinn-Phong fragment shader ("ibl :line") --------------------

// AbstractSky::sample of the legacy sky models, defined with the background pass below
template <int MODEL>
__device__ __forceinline__ f3 sky_sample(const RtSkyModel &m, f3 d);

__device__ __forceinline__ f3 mix3(f3 x, f3 y, float a) {   // glm::mix(x, y, a): x * (1 - a) + y * a
    const float b = 1.0f - a;
    return {x.x * b + y.x * a, x.y * b + y.y * a, x.z * b + y.z * a};
}
// glm::reflect(I, N) (detail/func_geometric.inl compute_reflect): I - N * dot(N, I) * 2, the vector scaled by the dot
// product and then by two
__device__ __forceinline__ f3 reflect3(f3 I, f3 N) {
    const float ni = dot3(N, I);
    return {I.x - N.x * ni * 2.0f, I.y - N.y * ni * 2.0f, I.z - N.z * ni * 2.0f};
}

// The shown fragment of hello_ibl_skybox.cpp's camera pass (ibl :810-852, the hard demo's interpolation and velocity)
// through its fragment_shader_full (ibl :446-524): the hard demo's Blinn-Phong under the same shadow lookup, with the
// ambient term tinted by u.sky->sample(N) and a Schlick-weighted u.sky->sample(reflect(-V, N)) added.  Not the hard
// shader plus two terms: the base colour multiplies the ambient and the diffuse term, not the specular one.
// SKY: u.sky, a compile-time choice (RT_SKY_NONE: u.sky == nullptr, envN = 1 and envR = 0; no gathers but the cubemap's).
// Everything of the direct term is reduced to seven floats (base, shadow, diffuse, specular, F) before the sky is
// sampled: N and V are all the two samples need.
template <int SKY>
__device__ void shade_pixel_ibl(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const RtRec &r = p.recs[id];
    const RtVary &y = p.vary[id];
    const RtDrawGPU &dr = p.draws[r.draw];
    const float iw0 = r.iw0, iw1 = r.iw1, iw2 = r.iw2;
    const float invw_sum = (u * iw0 + v * iw1) + w * iw2;
    {   // velocity (ibl :841-850)
        float pos[4], prev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pos[k] = (u * y.pos[k] + v * y.pos[4 + k]) + w * y.pos[8 + k];
            prev[k] = (u * y.prev[k] + v * y.prev[4 + k]) + w * y.prev[8 + k];
        }
        float csx, csy, psx, psy;
        to_screen(p, pos[0], pos[1], pos[3], csx, csy);
        to_screen(p, prev[0], prev[1], prev[3], psx, psy);
        float vx = csx - psx, vy = -(csy - psy);
        const float len = sqrtf(vx * vx + vy * vy);
        if (len > p.max_velocity && len > 1e-6f) {
            const float s = p.max_velocity / len;
            vx *= s;
            vy *= s;
        }
        vel = make_float2(vx, vy);
    }
    const f3 nsum = {(u * y.nrm[0] + v * y.nrm[3]) + w * y.nrm[6], (u * y.nrm[1] + v * y.nrm[4]) + w * y.nrm[7],
                     (u * y.nrm[2] + v * y.nrm[5]) + w * y.nrm[8]};
    const f3 in_normal = normalize3(nsum);
    f3 wp;
    wp.x = ((u * (y.world[0] * iw0) + v * (y.world[3] * iw1)) + w * (y.world[6] * iw2)) / invw_sum;
    wp.y = ((u * (y.world[1] * iw0) + v * (y.world[4] * iw1)) + w * (y.world[7] * iw2)) / invw_sum;
    wp.z = ((u * (y.world[2] * iw0) + v * (y.world[5] * iw1)) + w * (y.world[8] * iw2)) / invw_sum;
    const f3 N = normalize3(in_normal);
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 V = normalize3(sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp));
    const float ndotl = dot3(N, L);
    const float diffuse = g_max(ndotl, 0.0f) * 1.0f;
    const f3 H = normalize3(add3(L, V));
    const float spec = pow64(g_max(dot3(N, H), 0.0f));
    const float specular = (0.45f * spec) * 1.0f;
    f3 base = {dr.colf[0] / 255.0f, dr.colf[1] / 255.0f, dr.colf[2] / 255.0f};
    if (dr.texels) {
        // sample_nearest (shs_renderer.hpp:367-377)
        const float tu = ((u * (y.uv[0] * iw0) + v * (y.uv[2] * iw1)) + w * (y.uv[4] * iw2)) / invw_sum;
        const float tv = ((u * (y.uv[1] * iw0) + v * (y.uv[3] * iw1)) + w * (y.uv[5] * iw2)) / invw_sum;
        const float su = saturate(tu), sv = saturate(tv);
        const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
        const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
        const uint32_t tc = dr.texels[(size_t)yy * dr.tw + x];
        base = f3{(float)(tc & 0xffu) / 255.0f, (float)((tc >> 8) & 0xffu) / 255.0f, (float)((tc >> 16) & 0xffu) / 255.0f};
    }
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor(p, wp, ndotl);
    const float4 kn = *reinterpret_cast<const float4 *>(&p.ibl_draws[r.draw]);   // ambient, refl, f0, refl_mix
    // Math::schlick_fresnel(u.ibl_f0, max(0, N.V)) (shs_renderer.hpp:164-169)
    const float fx = 1.0f - saturate(g_max(0.0f, dot3(N, V)));
    const float fx2 = fx * fx;
    const float fx5 = fx2 * fx2 * fx;
    const float F = kn.z + (1.0f - kn.z) * fx5;
    const float rk = (F * kn.y) * kn.w;
    f3 envN = {1.0f, 1.0f, 1.0f}, envR = {0.0f, 0.0f, 0.0f};
    if constexpr (SKY != RT_SKY_NONE) {
        envN = sky_sample<SKY>(p.sky, N);
        envR = sky_sample<SKY>(p.sky, reflect3(f3{-V.x, -V.y, -V.z}, N));
    }
    // ambient = 0.18 * mix(vec3(1), envN, a); amb = ambient * base; direct = shadow * (diffuse * base + specular);
    // refl = envR * rk; clamp((amb + direct) + refl)
    const f3 tint = mix3(f3{1.0f, 1.0f, 1.0f}, envN, kn.x);
    const float pr = g_clamp01(((0.18f * tint.x) * base.x + shadow * (diffuse * base.x + specular)) + envR.x * rk) * 255;
    const float pg = g_clamp01(((0.18f * tint.y) * base.y + shadow * (diffuse * base.y + specular)) + envR.y * rk) * 255;
    const float pb = g_clamp01(((0.18f * tint.z) * base.z + shadow * (diffuse * base.z + specular)) + envR.z * rk) * 255;
    rgba = byte_x86(pr) | (byte_x86(pg) << 8) | (byte_x86(pb) << 16) | 0xff000000u;
    pq = make_float4(pr, pg, pb, shadow);
}

// ---- hello_water.cpp: the atmosphere shader, the water shader and the planar reflection ("water :line") ----

// fractf :759
__device__ __forceinline__ float fractf1(float x) { return x - floorf(x); }

// hash12 :771-777: q = fract2(p * vec2(123.34, 456.21)); q += dot(q, q + 34.345); fract(q.x * q.y).  Chaotic: every
// operation below is the reference's, in its order, and rounds once.
__device__ __forceinline__ float water_hash12(float px, float py) {
    float qx = fractf1(px * 123.34f), qy = fractf1(py * 456.21f);
    const float d = qx * (qx + 34.345f) + qy * (qy + 34.345f);
    qx = qx + d;
    qy = qy + d;
    return fractf1(qx * qy);
}

// noise2 :798-814 (i + vec2(0, 0) leaves every value hash12 can tell apart as it was)
__device__ __forceinline__ float water_noise2(float px, float py) {
    const float ix = floorf(px), iy = floorf(py);
    const float fx = px - ix, fy = py - iy;
    const float a = water_hash12(ix, iy);
    const float b = water_hash12(ix + 1.0f, iy);
    const float c = water_hash12(ix, iy + 1.0f);
    const float d = water_hash12(ix + 1.0f, iy + 1.0f);
    const float ux = (fx * fx) * (3.0f - 2.0f * fx), uy = (fy * fy) * (3.0f - 2.0f * fy);
    const float x1 = a + (b - a) * ux;
    const float x2 = c + (d - c) * ux;
    return x1 + (x2 - x1) * uy;
}

// fbm2 :816-826
__device__ __forceinline__ float water_fbm2(float px, float py) {
    float f = 0.0f, a = 0.5f;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        f += a * water_noise2(px, py);
        px *= 2.02f;
        py *= 2.02f;
        a *= 0.5f;
    }
    return f;
}

// sampleN :902-917.  Its h0 and h1 are dead.  The four fbm2 arguments are (p +- vec2(e, 0)) * 1.2 and (p +- vec2(0, e)) * 1.2:
// a subtraction is the addition of the negated operand, signed zeros included, so one loop serves the four.
__device__ __forceinline__ f3 water_sample_n(float px, float py) {
    const float e = 0.18f;
    float hx = 0.0f, hz = 0.0f, prev = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const float ox = (k == 0) ? e : (k == 1) ? -e : (k == 2) ? 0.0f : -0.0f;
        const float oy = (k == 0) ? 0.0f : (k == 1) ? -0.0f : (k == 2) ? e : -e;
        const float f = water_fbm2((px + ox) * 1.2f, (py + oy) * 1.2f);
        if (k == 1) hx = prev - f;
        if (k == 3) hz = prev - f;
        prev = f;
    }
    return normalize3(f3{-hx * 2.4f, 1.0f, -hz * 2.4f});
}

// water_flow_normal_and_foam :862-930 after the host's part (RtWaterModel)
__device__ void water_normal_foam(const RtWaterModel &m, f3 wp, f3 &N, float &foam) {
    const float uvx = wp.x * m.perp[0] + wp.z * m.perp[1];
    const float uvy = (wp.x * m.fd[0] + wp.z * m.fd[1]) * 2.8f;
    const float bx = uvx * 0.055f, by = uvy * 0.055f;
    const f3 nA = water_sample_n((bx + m.j0[0]) + m.off0[0], (by + m.j0[1]) + m.off0[1]);
    const f3 nB = water_sample_n((bx + m.j1[0]) + m.off1[0], (by + m.j1[1]) + m.off1[1]);
    f3 n = normalize3(mix3(nA, nB, m.w));
    n = normalize3(f3{n.x + m.tilt[0], n.y + 0.0f, n.z + m.tilt[1]});
    N = n;
    const float curvature = sqrtf(n.x * n.x + n.z * n.z);
    foam = saturate((curvature - 0.55f) * 1.6f);
}

// (int)std::lround(x) for any x that is NaN or whose rounded value fits an int: halves away from zero on both sides
// of zero (lround_x86 above covers [0, n - 1] only; the reflection lookup reaches -0.75 and n - 0.25)
__device__ __forceinline__ int lround_away_x86(float x) {
    if (!(x == x)) return 0;
    const float t = truncf(x);
    const float d = x - t;   // exact
    return (int)t + ((d >= 0.5f) ? 1 : ((d <= -0.5f) ? -1 : 0));
}

// shadow_uvz_from_world and shadow_factor_pcf_2x2 as hello_water.cpp has them (water :696-751).  Not the hard demo's
// lookup: a uv outside [0, 1] is lit before the PCF taps (the hard demo clamps the taps to the edge), and an empty
// texel (FLT_MAX) counts as lit whatever z is (the hard demo compares, which differs for a NaN z).
__device__ float shadow_factor_water(const RtParams &p, f3 wp, float ndotl) {
    float cx, cy, cz, cw;
    m4p(p.light_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
    if (fabsf(cw) < 1e-6f) return 1.0f;
    const float nx = cx / cw, ny = cy / cw, z = cz / cw;
    if (z < 0.0f || z > 1.0f) return 1.0f;
    const float u = nx * 0.5f + 0.5f;
    const float v = 1.0f - (ny * 0.5f + 0.5f);
    const float slope = 1.0f - g_clamp01(ndotl);
    const float bias = p.bias_base + p.bias_slope * slope;
    if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return 1.0f;
    if (!(p.flags & SHS_RT_PCF)) {
        const int x = lround_x86(u * (float)(p.sw - 1));
        const int y = lround_x86(v * (float)(p.sh - 1));
        const float d = sm_sample(p, x, y);
        if (d == FLT_MAX) return 1.0f;
        return (z <= d + bias) ? 1.0f : 0.0f;
    }
    const float fx = u * (float)(p.sw - 1);
    const float fy = v * (float)(p.sh - 1);
    const int x0 = clampi(int_x86(floorf(fx)), 0, p.sw - 1);
    const int y0 = clampi(int_x86(floorf(fy)), 0, p.sh - 1);
    const int x1 = clampi(x0 + 1, 0, p.sw - 1);
    const int y1 = clampi(y0 + 1, 0, p.sh - 1);
    const float d00 = sm_sample(p, x0, y0), d10 = sm_sample(p, x1, y0), d01 = sm_sample(p, x0, y1), d11 = sm_sample(p, x1, y1);
    const float s00 = (d00 == FLT_MAX) ? 1.0f : ((z <= d00 + bias) ? 1.0f : 0.0f);
    const float s10 = (d10 == FLT_MAX) ? 1.0f : ((z <= d10 + bias) ? 1.0f : 0.0f);
    const float s01 = (d01 == FLT_MAX) ? 1.0f : ((z <= d01 + bias) ? 1.0f : 0.0f);
    const float s11 = (d11 == FLT_MAX) ? 1.0f : ((z <= d11 + bias) ? 1.0f : 0.0f);
    return 0.25f * (((s00 + s10) + s01) + s11);
}

// pow(x, 5.0f), pow(x, 256.0f), pow(x, 520.0f): products in double rounded once, as pow64
__device__ __forceinline__ float pow5(float x) {
    const double d = (double)x, d2 = d * d;
    return (float)(d2 * d2 * d);
}
__device__ __forceinline__ float pow256(float x) {
    double d = (double)x;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = d * d;
    return (float)d;
}
__device__ __forceinline__ float pow520(float x) {   // 512 and 8
    double d = (double)x;
    d = d * d; d = d * d; d = d * d;
    double e = d;
#pragma unroll
    for (int i = 0; i < 6; ++i) e = e * e;
    return (float)(e * d);
}

// One channel's way to the screen in hello_water.cpp (:984-992, :1088-1095): the exposure, tonemap_reinhard, gamma_2p2
// (glm::clamp, then pow), the channel * 255.  The byte is a rounding, clampi((int)lround(.), 0, 255), where the other
// shadings truncate: water_byte.
__device__ __forceinline__ float water_encode(float x) {
    x = x / (1.0f + x);
    x = powf(g_clamp01(x), 1.0f / 2.2f);
    return x * 255.0f;
}
__device__ __forceinline__ uint32_t water_byte(float x) { return (uint32_t)clampi(lround_away_x86(x), 0, 255); }

// The shown fragment of hello_water.cpp's camera pass (water :2060-2211, the hard demo's interpolation and velocity)
// through the shader its draw names: fragment_shader_full (:938-994, the atmosphere shader) or fragment_shader_water
// (:1000-1097).  One kernel holds both because one frame mixes them per pixel; the branch is per draw, so a wave
// diverges only where it straddles the water's silhouette.  What the two share is written once: V, the sky along the
// ray, the shadow lookup, the half vector, the fog and the way to the byte.
__device__ void shade_pixel_water(const RtParams &p, int32_t id, float u, float v, float w, uint32_t &rgba, float2 &vel, float4 &pq) {
    const RtRec &r = p.recs[id];
    const RtVary &y = p.vary[id];
    const RtDrawGPU &dr = p.draws[r.draw];
    const float iw0 = r.iw0, iw1 = r.iw1, iw2 = r.iw2;
    const float invw_sum = (u * iw0 + v * iw1) + w * iw2;
    {   // velocity (the hard demo's :1002-1011)
        float pos[4], prev[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pos[k] = (u * y.pos[k] + v * y.pos[4 + k]) + w * y.pos[8 + k];
            prev[k] = (u * y.prev[k] + v * y.prev[4 + k]) + w * y.prev[8 + k];
        }
        float csx, csy, psx, psy;
        to_screen(p, pos[0], pos[1], pos[3], csx, csy);
        to_screen(p, prev[0], prev[1], prev[3], psx, psy);
        float vx = csx - psx, vy = -(csy - psy);
        const float len = sqrtf(vx * vx + vy * vy);
        if (len > p.max_velocity && len > 1e-6f) {
            const float s = p.max_velocity / len;
            vx *= s;
            vy *= s;
        }
        vel = make_float2(vx, vy);
    }
    f3 wp;
    wp.x = ((u * (y.world[0] * iw0) + v * (y.world[3] * iw1)) + w * (y.world[6] * iw2)) / invw_sum;
    wp.y = ((u * (y.world[1] * iw0) + v * (y.world[4] * iw1)) + w * (y.world[7] * iw2)) / invw_sum;
    wp.z = ((u * (y.world[2] * iw0) + v * (y.world[5] * iw1)) + w * (y.world[8] * iw2)) / invw_sum;
    const RtWaterGPU &wf = *p.water;
    const bool is_water = (reinterpret_cast<const uint32_t *>(p.water + 1)[r.draw] & SHS_RT_WATER_SURFACE) != 0u;
    const f3 L = {p.L[0], p.L[1], p.L[2]};
    const f3 toc = sub3(f3{p.cam[0], p.cam[1], p.cam[2]}, wp);
    const f3 V = normalize3(toc);
    // sky_color_simple(normalize(RAY), normalize(-L)) :157-170; its own normalize(sun_dir) is the host's (RtParams::sun)
    f3 sky;
    {
        const f3 ray = normalize3(f3{-V.x, -V.y, -V.z});
        const float t = saturate(ray.y * 0.5f + 0.5f);
        sky = mix3(f3{0.62f, 0.74f, 0.92f}, f3{0.10f, 0.22f, 0.55f}, t);
        const float sd = dot3(f3{wf.sun[0], wf.sun[1], wf.sun[2]}, normalize3(ray));
        const float h = sd * 0.5f + 0.5f;
        const float sun = pow256((h < 0.0f) ? 0.0f : (h > 1.0f ? 1.0f : h));
        sky = add3(sky, f3{(1.0f * sun) * 8.0f, (0.88f * sun) * 8.0f, (0.65f * sun) * 8.0f});
    }
    f3 N;
    float foam = 0.0f;
    if (is_water) {
        water_normal_foam(wf.model, wp, N, foam);
    } else {
        const f3 nsum = {(u * y.nrm[0] + v * y.nrm[3]) + w * y.nrm[6], (u * y.nrm[1] + v * y.nrm[4]) + w * y.nrm[7],
                         (u * y.nrm[2] + v * y.nrm[5]) + w * y.nrm[8]};
        N = normalize3(normalize3(nsum));
    }
    const float ndotl = dot3(N, L);
    float shadow = 1.0f;
    if (p.shadow) shadow = shadow_factor_water(p, wp, ndotl);
    const f3 H = normalize3(add3(L, V));
    const float ndoth = g_max(dot3(N, H), 0.0f);
    f3 hdr;
    float exposure;
    if (is_water) {
        const float NoV = g_clamp01(dot3(N, V));
        const float NoL = g_clamp01(ndotl);
        const float fresnel = 0.02f + (1.0f - 0.02f) * pow5(1.0f - NoV);
        f3 refl_col = sky;
        if (wf.refl) {   // the planar reflection :1021-1044
            float cx, cy, cz, cw;
            m4p(wf.refl_vp, wp.x, wp.y, wp.z, cx, cy, cz, cw);
            if (fabsf(cw) > 1e-6f) {
                const float rx_ndc = cx / cw, ry_ndc = cy / cw;
                if (rx_ndc >= -1.0f && rx_ndc <= 1.0f && ry_ndc >= -1.0f && ry_ndc <= 1.0f) {
                    float sx = (rx_ndc * 0.5f + 0.5f) * (float)(wf.refl_w - 1);
                    float sy = (1.0f - (ry_ndc * 0.5f + 0.5f)) * (float)(wf.refl_h - 1);
                    sx += N.x * 0.75f;
                    sy += N.z * 0.75f;
                    // sx lies in [-0.75, w - 0.25] or is NaN (|N.x| <= 1 or NaN): lround's halves away from zero on
                    // either side; a NaN gives (int)LONG_MIN = 0, so rx = 0 and ry_canvas = h - 1
                    const int rx = lround_away_x86(sx);
                    const int ry_screen = lround_away_x86(sy);
                    const int ry_canvas = (wf.refl_h - 1) - ry_screen;
                    // sample_canvas_nearest :146-151
                    const uint32_t rc = wf.refl[(size_t)clampi(ry_canvas, 0, wf.refl_h - 1) * wf.refl_w + clampi(rx, 0, wf.refl_w - 1)];
                    refl_col = f3{(float)(rc & 0xffu) / 255.0f, (float)((rc >> 8) & 0xffu) / 255.0f, (float)((rc >> 16) & 0xffu) / 255.0f};
                }
            }
        }
        const float spec = pow520(ndoth);
        const float spec_kill = 1.0f - foam * 0.90f;
        const float specular = ((1.0f * spec) * 0.95f) * spec_kill;
        const float diffuse = (1.0f * NoL) * 0.05f;
        f3 surface = mix3(f3{0.03f, 0.12f, 0.16f}, refl_col, fresnel);
        const f3 foam_col = mix3(f3{0.75f, 0.85f, 0.95f}, sky, 0.25f);
        const float foam_gain = foam * (0.35f + 0.65f * (1.0f - NoV));
        surface = mix3(surface, foam_col, foam_gain);
        const float sd = shadow * diffuse, ss = shadow * specular;
        hdr = f3{surface.x * (sky.x * 0.12f + sd) + ss, surface.y * (sky.y * 0.12f + sd) + ss, surface.z * (sky.z * 0.12f + sd) + ss};
        exposure = 0.90f;
    } else {
        f3 base = {dr.colf[0] / 255.0f, dr.colf[1] / 255.0f, dr.colf[2] / 255.0f};
        if (dr.texels) {
            // sample_nearest :121-140
            const float tu = ((u * (y.uv[0] * iw0) + v * (y.uv[2] * iw1)) + w * (y.uv[4] * iw2)) / invw_sum;
            const float tv = ((u * (y.uv[1] * iw0) + v * (y.uv[3] * iw1)) + w * (y.uv[5] * iw2)) / invw_sum;
            const float su = saturate(tu), sv = saturate(tv);
            const int x = clampi(lround_x86(su * (float)(dr.tw - 1)), 0, dr.tw - 1);
            const int yy = clampi(lround_x86(sv * (float)(dr.th - 1)), 0, dr.th - 1);
            const uint32_t tc = dr.texels[(size_t)yy * dr.tw + x];
            base = f3{(float)(tc & 0xffu) / 255.0f, (float)((tc >> 8) & 0xffu) / 255.0f, (float)((tc >> 16) & 0xffu) / 255.0f};
        }
        const float NoL = g_max(ndotl, 0.0f);
        const float diffuse = (1.0f * NoL) * 0.90f;
        const float specular = (1.0f * pow64(ndoth)) * 0.35f;
        const float lit = shadow * (diffuse + specular);
        hdr = f3{base.x * (sky.x * 0.08f + lit), base.y * (sky.y * 0.08f + lit), base.z * (sky.z * 0.08f + lit)};
        exposure = 1.00f;
    }
    // apply_fog_exp2 :172-176 over clampf(length(camera_pos - world_pos), 0, 250), then the exposure
    float dist = sqrtf(dot3(toc, toc));
    dist = (dist < 0.0f) ? 0.0f : (dist > 250.0f ? 250.0f : dist);
    const float tr = exp2f(-0.0065f * dist);
    const float fr = 1.0f - tr;
    const float pr = water_encode((hdr.x * tr + sky.x * fr) * exposure);
    const float pg = water_encode((hdr.y * tr + sky.y * fr) * exposure);
    const float pb = water_encode((hdr.z * tr + sky.z * fr) * exposure);
    rgba = water_byte(pr) | (water_byte(pg) << 8) | (water_byte(pb) << 16) | 0xff000000u;
    pq = make_float4(pr, pg, pb, shadow);
}

// SHADING: shs_rt_frame::shading of the camera pass, a compile-time choice (the shadow pass ignores it); shading 4 is
// three instantiations, RT_SHADING_IBL + the sky model it samples (RT_SKY_*), which takes the values 4 to 6: shading 5
// is RT_SHADING_WATER
constexpr int RT_SHADING_IBL = 4;
constexpr int RT_SHADING_WATER = 7;
template <bool SHADOW, int SHADING = 0>
__global__ __launch_bounds__(256) void k_rt_raster(const RtParams p) {
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
            cand = (__float_as_uint(q3.y) & RT_VALID) && lo16(gbx) <= gx1 && hi16(gbx) >= gx0 && lo16(gby) <= gy1 &&
                   hi16(gby) >= gy0 && axis_meets(q3.z, q3.w, gx0, gx1, j0x, j1x, p.tile_w, p.W) &&
                   axis_meets(q4.x, q4.y, gy0, gy1, j0y, j1y, p.tile_h, p.H);
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
        if (live) {
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
                    const float4 a5 = s_rec[c * 6 + 5];   // (iw0, iw1, iw2, draw)
                    const float invw_sum = (u * a5.x + v * a5.y) + w * a5.z;
                    if (invw_sum <= 1e-8f) continue;
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
    if constexpr (SHADING == 1) {
        if (sid >= 0) shade_pixel_soft(p, sid, su, sv, sw, px, py, rgba, pq);   // the velocity plane stays zero
    } else if constexpr (SHADING == 2) {
        if (sid >= 0) shade_pixel_pbr<false>(p, sid, su, sv, sw, px, py, rgba, vel, pq);
    } else if constexpr (SHADING == 3) {
        if (sid >= 0) shade_pixel_pbr<true>(p, sid, su, sv, sw, px, py, rgba, vel, pq);
    } else if constexpr (SHADING == RT_SHADING_WATER) {
        if (sid >= 0) shade_pixel_water(p, sid, su, sv, sw, rgba, vel, pq);
    } else if constexpr (SHADING >= RT_SHADING_IBL) {
        if (sid >= 0) shade_pixel_ibl<SHADING - RT_SHADING_IBL>(p, sid, su, sv, sw, rgba, vel, pq);
    } else {
        if (sid >= 0) shade_pixel(p, sid, su, sv, sw, rgba, vel, pq);
    }
    const size_t o = (size_t)(p.H - 1 - py) * p.W + px;   // canvas rows
    p.color[o] = rgba;
    p.depth[o] = best;
    p.velocity[o] = vel;
    p.ids[o] = sid;
    if (p.prequant) p.prequant[o] = pq;
}

// shs_rt_pcss_samples: one lane per sample through the device function the raster calls
__global__ __launch_bounds__(256) void k_rt_pcss_samples(const RtPcssSamples q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    const PcssMap m = {q.map, q.w, q.h, q.pcss_light, q.pcss_search, q.pcss_min, q.pcss_max, q.pcss_eps, q.pcss_blockers, q.pcss_taps};
    q.out[i] = pcss_shadow_factor(m, q.uv[2 * i], q.uv[2 * i + 1], q.z[i], q.bias[i], q.rot[i]);
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

// ---- skybox_background_pass (pbr :733-799) over the legacy sky models ("sky :line": hello-shs-renderer/shs_renderer.hpp)

__device__ __forceinline__ f3 ld3(const float *p) { return {p[0], p[1], p[2]}; }

// AnalyticSky::sample (sky :558-608) after the host's part (RtSkyModel).  Its three std::pow(x, 3.0f / 4.0f / 12.0f)
// are products in double rounded once, as pow64; everything else is + - * / sqrt and compares, so cosGamma and with
// it the disc / edge branch are the reference's.
__device__ f3 sky_analytic(const RtSkyModel &m, f3 dir) {
    const f3 d = normalize3(dir);
    const f3 s = ld3(m.s);
    const float cosTheta = g_min(g_max(d.y, -1.0f), 1.0f);
    const float cosGamma = dot3(d, s);
    // glm::smoothstep(-0.15f, 0.15f, cosTheta)
    const float t = g_clamp01((cosTheta - -0.15f) / (0.15f - -0.15f));
    const float sky_ground = t * t * (3.0f - 2.0f * t);
    const double up = (double)(1.0f - g_max(0.0f, cosTheta));
    const f3 upper = mix3(ld3(m.zenith), ld3(m.horizon), (float)(up * up * up));
    const double hz = (double)(1.0f + g_min(0.0f, cosTheta)), hz2 = hz * hz;
    const f3 lower = mix3(ld3(m.ground), ld3(m.half_horizon), (float)(hz2 * hz2));
    f3 c = mix3(lower, upper, sky_ground);
    const double g = (double)g_clamp01(cosGamma), g2 = g * g, g4 = g2 * g2;
    const float glow = (float)((g4 * g4) * g4);
    c = add3(c, sc3(ld3(m.glow), glow));
    if (cosGamma > 0.9998f) {
        c = {4.0f, 3.5f, 3.0f};
    } else if (cosGamma > 0.9992f) {
        const float edge = (cosGamma - 0.9992f) / (0.9998f - 0.9992f);
        c = mix3(c, f3{3.0f, 2.5f, 1.5f}, edge);
    }
    return c;
}

// Texture2D::get (sky :360-363) then to_lin (sky :462-465): {0, 0, 0, 0} out of bounds, which the table takes to 0 as
// pow(0, 2.2f).  An unconditional load at a clamped address plus a select (as pcss_tap).
__device__ __forceinline__ f3 sky_texel(const uint32_t *tex, int w, int h, const float *lut, int x, int y) {
    const bool in = x >= 0 && x < w && y >= 0 && y < h;
    const uint32_t raw = tex[(size_t)clampi(y, 0, h - 1) * w + clampi(x, 0, w - 1)];
    const uint32_t tc = in ? raw : 0u;
    return {lut[tc & 0xffu], lut[(tc >> 8) & 0xffu], lut[(tc >> 16) & 0xffu]};
}

// CubeMapSky::sample over sample_face_bilinear (sky :439-512).  A NaN coordinate passes glm::clamp and converts to
// INT_MIN (x1 = INT_MIN + 1): all four texels are out of bounds.
__device__ f3 sky_cubemap(const RtSkyModel &m, f3 d) {
    const float len = sqrtf(dot3(d, d));
    if (len < 1e-8f) return {0.0f, 0.0f, 0.0f};
    d = {d.x / len, d.y / len, d.z / len};
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    int face;
    float u, v;
    if (ax >= ay && ax >= az) {
        if (d.x > 0.0f) { face = 0; u = -d.z / ax; v = d.y / ax; }
        else            { face = 1; u = d.z / ax; v = d.y / ax; }
    } else if (ay >= ax && ay >= az) {
        if (d.y > 0.0f) { face = 2; u = d.x / ay; v = -d.z / ay; }
        else            { face = 3; u = d.x / ay; v = d.z / ay; }
    } else {
        if (d.z > 0.0f) { face = 4; u = d.x / az; v = d.y / az; }
        else            { face = 5; u = -d.x / az; v = d.y / az; }
    }
    u = 0.5f * (u + 1.0f);
    v = 0.5f * (v + 1.0f);
    // the face's texture out of the kernel arguments: selects over the six, not a per-lane index into them
    const uint32_t *tex = m.face[0];
    int w = m.fw[0], h = m.fh[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) {
        const bool is = face == k;
        tex = is ? m.face[k] : tex;
        w = is ? m.fw[k] : w;
        h = is ? m.fh[k] : h;
    }
    u = g_clamp01(u);   // glm::clamp: min(max(x, 0), 1)
    v = g_clamp01(v);
    const float fx = u * (float)(w - 1);
    const float fy = v * (float)(h - 1);
    const int x0 = int_x86(floorf(fx));
    const int y0 = int_x86(floorf(fy));
    const int x1 = min(x0 + 1, w - 1);
    const int y1 = min(y0 + 1, h - 1);
    const float tx = fx - (float)x0;
    const float ty = fy - (float)y0;
    const f3 v00 = sky_texel(tex, w, h, m.srgb_lut, x0, y0), v10 = sky_texel(tex, w, h, m.srgb_lut, x1, y0);
    const f3 v01 = sky_texel(tex, w, h, m.srgb_lut, x0, y1), v11 = sky_texel(tex, w, h, m.srgb_lut, x1, y1);
    const f3 vx0 = mix3(v00, v10, tx);
    const f3 vx1 = mix3(v01, v11, tx);
    return sc3(mix3(vx0, vx1, ty), m.intensity);
}

template <int MODEL>
__device__ __forceinline__ f3 sky_sample(const RtSkyModel &m, f3 d) {
    if constexpr (MODEL == RT_SKY_CUBEMAP) return sky_cubemap(m, d);
    else return sky_analytic(m, d);
}

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

hipError_t launch_canvas_rt(const shs_dev::RtParams &p, bool shadow_pass, int shading, hipStream_t s, int sky_model) {
    using namespace shs_dev;
    if (p.n_tris > 0) {
        const int grid = (p.n_tris + 255) / 256;
        if (shadow_pass) hipLaunchKernelGGL(k_rt_setup<true>, dim3(grid), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(k_rt_setup<false>, dim3(grid), dim3(256), 0, s, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int tiles = ((p.W + RT_TW - 1) / RT_TW) * ((p.H + RT_TH - 1) / RT_TH);
    if (shadow_pass) hipLaunchKernelGGL(k_rt_raster<true>, dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 1) hipLaunchKernelGGL((k_rt_raster<false, 1>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 2) hipLaunchKernelGGL((k_rt_raster<false, 2>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 3) hipLaunchKernelGGL((k_rt_raster<false, 3>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 5) hipLaunchKernelGGL((k_rt_raster<false, RT_SHADING_WATER>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 4 && sky_model == RT_SKY_CUBEMAP)
        hipLaunchKernelGGL((k_rt_raster<false, RT_SHADING_IBL + RT_SKY_CUBEMAP>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 4 && sky_model == RT_SKY_ANALYTIC)
        hipLaunchKernelGGL((k_rt_raster<false, RT_SHADING_IBL + RT_SKY_ANALYTIC>), dim3(tiles), dim3(256), 0, s, p);
    else if (shading == 4) hipLaunchKernelGGL((k_rt_raster<false, RT_SHADING_IBL + RT_SKY_NONE>), dim3(tiles), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_rt_raster<false>, dim3(tiles), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace shs_internal
