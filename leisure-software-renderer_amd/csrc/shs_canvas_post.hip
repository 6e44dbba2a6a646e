// shs_canvas_post.hip -- the Canvas-API multi-pass extras on gfx950 (paths
// relative to /root/reference/cpp-folders/src/hello-render-target/):
//   k_canvas_motion_blur   combined_motion_blur_pass (hello_pbr.cpp:1128-1252): per pixel the camera
//                          velocity from depth + matrices (:1051-1109), the object / camera mix, the
//                          soft knee (:1111-1122) and the clamp, then `samples` tent-weighted taps;
//   k_canvas_gaussian      gaussian_blur_pass (hello_depth_of_field.cpp:175-251), 5 taps, one axis;
//   k_canvas_autofocus     autofocus_depth_median_center (:257-285): the nth_element median of the
//                          window's finite depths as a rank selection in one workgroup;
//   k_canvas_dof_composite dof_composite_pass (:287-343);
//   k_canvas_light_shafts  light_shafts_pass (hello_pbr_light_shafts.cpp:1390-1707): per pixel a ray march of
//                          up to `steps` samples through noisy height fog, each with the shadow map's
//                          2x2 PCF through light_vp, then the pixel's soft re-tonemap.
// One thread per pixel; every float expression keeps the reference's operation order
// (-ffp-contract=off, correctly rounded '/' and sqrt), so the output bytes are the reference's (the light
// shafts' transcendentals excepted: see sin_r and its neighbours).
#include <float.h>

#include "shs_canvas_post_internal.hpp"

namespace shs_dev {

namespace {

__device__ __forceinline__ void m4v(const float *m, float x, float y, float z, float w, float (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (m[r] * x + m[4 + r] * y) + (m[8 + r] * z + m[12 + r] * w);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return (v < lo) ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return (v < lo) ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float glength(float x, float y) { return sqrtf(x * x + y * y); }
// std::round then (int): half away from zero; NaN -> 0 (x86's INT_MIN clamps to the same 0)
__device__ __forceinline__ int round_i(float v) { return (int)roundf(v); }

// compute_camera_velocity_canvas_fast (hello_pbr.cpp:1077-1109)
__device__ __forceinline__ void camera_velocity(const CanvasMBParams &p, int x, int y, float view_z, float &vx, float &vy) {
    vx = 0.0f;
    vy = 0.0f;
    if (view_z == FLT_MAX) return;
    // canvas_to_ndc_xy (:1058-1068)
    const int py_screen = (p.H - 1) - y;
    const float fx = ((float)x + 0.5f) / (float)p.W;
    const float fy = ((float)py_screen + 0.5f) / (float)p.H;
    const float ndc_x = fx * 2.0f - 1.0f;
    const float ndc_y = 1.0f - fy * 2.0f;
    // viewz_to_ndcz (:1051-1056)
    float c[4];
    m4v(p.curr_proj, 0.0f, 0.0f, view_z, 1.0f, c);
    const float ndc_z = (fabsf(c[3]) < 1e-6f) ? 0.0f : c[2] / c[3];
    float wh[4];
    m4v(p.inv_curr_vp, ndc_x, ndc_y, ndc_z, 1.0f, wh);
    if (fabsf(wh[3]) < 1e-6f) return;
    const float wx = wh[0] / wh[3], wy = wh[1] / wh[3], wz = wh[2] / wh[3];
    float pc[4];
    m4v(p.prev_vp, wx, wy, wz, 1.0f, pc);
    if (fabsf(pc[3]) < 1e-6f) return;
    const float pnx = pc[0] / pc[3], pny = pc[1] / pc[3];
    // ndc_to_screen_xy (:1070-1075)
    const float psx = (pnx * 0.5f + 0.5f) * (float)(p.W - 1);
    const float psy = (1.0f - (pny * 0.5f + 0.5f)) * (float)(p.H - 1);
    vx = (float)x - psx;
    vy = -((float)py_screen - psy);
}

__device__ __forceinline__ uint32_t pack(int r, int g, int b, int a) {
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | ((uint32_t)a << 24);
}

}  // namespace

__global__ __launch_bounds__(256) void k_canvas_motion_blur(CanvasMBParams p) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * p.W + x;
    float cvx, cvy;
    camera_velocity(p, x, y, p.depth[i], cvx, cvy);
    const float2 vf = p.velocity[i];
    const float ox = vf.x - cvx, oy = vf.y - cvy;
    float vx = (p.w_obj * ox + p.w_cam * cvx) * p.strength;
    float vy = (p.w_obj * oy + p.w_cam * cvy) * p.strength;
    if (p.soft_knee) {   // apply_soft_knee (:1111-1122)
        const float len = glength(vx, vy);
        if (!(len <= 1e-6f) && !(len <= p.knee)) {
            const float den = p.max_px - p.knee;
            const float t = (len - p.knee) / ((1e-6f < den) ? den : 1e-6f);
            const float t2 = t / (1.0f + t);
            const float new_len = p.knee + (p.max_px - p.knee) * t2;
            const float s = new_len / len;
            vx *= s;
            vy *= s;
        }
    }
    float len = glength(vx, vy);
    if (len > p.max_px && len > 1e-6f) {
        const float s = p.max_px / len;
        vx *= s;
        vy *= s;
        len = p.max_px;
    }
    if (len < 0.001f || p.samples <= 1) {
        p.dst[i] = p.src[i];
        return;
    }
    const float dx = vx / len, dy = vy / len;
    float r = 0.0f, g = 0.0f, b = 0.0f, wsum = 0.0f;
    for (int k = 0; k < p.samples; ++k) {
        const float t = (float)k / (float)(p.samples - 1);
        const float a = (t - 0.5f) * 2.0f;
        const float al = a * len;
        const int sx = clampi(round_i((float)x + dx * al), 0, p.W - 1);
        const int sy = clampi(round_i((float)y + dy * al), 0, p.H - 1);
        const float wgt = 1.0f - fabsf(a);
        const uint32_t c = p.src[(size_t)sy * p.W + sx];
        r += wgt * (float)(c & 0xffu);
        g += wgt * (float)((c >> 8) & 0xffu);
        b += wgt * (float)((c >> 16) & 0xffu);
        wsum += wgt;
    }
    if (wsum < 0.0001f) wsum = 1.0f;
    p.dst[i] = pack(clampi((int)(r / wsum), 0, 255), clampi((int)(g / wsum), 0, 255), clampi((int)(b / wsum), 0, 255), 255);
}

// gaussian_blur_pass: r = w0 c0 + w1 c1 + w2 c2 + w1 c3 + w0 c4 (left to right), then color_from_rgbaf
__global__ __launch_bounds__(256) void k_canvas_gaussian(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int W,
                                                         int H, int horizontal) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= W || y >= H) return;
    const float w0 = 0.06136f, w1 = 0.24477f, w2 = 0.38774f;
    uint32_t c[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int sx = horizontal ? clampi(x + k - 2, 0, W - 1) : x;
        const int sy = horizontal ? y : clampi(y + k - 2, 0, H - 1);
        c[k] = src[(size_t)sy * W + sx];
    }
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int sh = 8 * ch;
        float v = w0 * (float)((c[0] >> sh) & 0xffu) + w1 * (float)((c[1] >> sh) & 0xffu);
        v = v + w2 * (float)((c[2] >> sh) & 0xffu);
        v = v + w1 * (float)((c[3] >> sh) & 0xffu);
        v = v + w0 * (float)((c[4] >> sh) & 0xffu);
        const float m = (0.0f < v) ? v : 0.0f;        // std::max(0.0f, v)
        const float q = (m < 255.0f) ? m : 255.0f;    // std::min(255.0f, .)
        out |= (uint32_t)(uint8_t)q << sh;
    }
    dst[(size_t)y * W + x] = out;
}

// autofocus_depth_median_center: the window's depths that are not FLT_MAX (out-of-bounds reads are
// FLT_MAX), the element nth_element places at size / 2 == the value of rank size / 2.
constexpr int AF_MAX_RADIUS = 32;
constexpr int AF_MAX = (2 * AF_MAX_RADIUS + 1) * (2 * AF_MAX_RADIUS + 1);

__global__ __launch_bounds__(1024) void k_canvas_autofocus(CanvasDofParams p) {
    __shared__ float s_v[AF_MAX];
    __shared__ int s_n;
    const int tid = (int)threadIdx.x, side = 2 * p.radius + 1, total = side * side;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int k = tid; k < total; k += 1024) {
        const int x = p.cx + (k % side) - p.radius, y = p.cy + (k / side) - p.radius;
        const float d = (x >= 0 && x < p.W && y >= 0 && y < p.H) ? p.depth[(size_t)y * p.W + x] : FLT_MAX;
        if (d != FLT_MAX) s_v[atomicAdd(&s_n, 1)] = d;
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0) {
        if (tid == 0) {
            const bool in = p.cx >= 0 && p.cx < p.W && p.cy >= 0 && p.cy < p.H;
            const float d = in ? p.depth[(size_t)p.cy * p.W + p.cx] : FLT_MAX;
            *p.focus = (d == FLT_MAX) ? 15.0f : d;
        }
        return;
    }
    const int mid = n / 2;
    for (int k = tid; k < n; k += 1024) {
        const float v = s_v[k];
        int less = 0, equal = 0;
        for (int j = 0; j < n; ++j) {
            const float u = s_v[j];
            less += u < v;
            equal += u == v;
        }
        if (less <= mid && mid < less + equal) *p.focus = v;   // every such value compares equal
    }
}

// dof_composite_pass
__global__ __launch_bounds__(256) void k_canvas_dof_composite(CanvasDofParams p) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= p.W || y >= p.H) return;
    const size_t i = (size_t)y * p.W + x;
    const float focus = *p.focus;
    float d = p.depth[i];
    if (d == FLT_MAX) d = focus + p.range;
    const float coc = fabsf(d - focus) / p.range;
    float t = clampf(coc, 0.0f, 1.0f);            // smoothstep01
    t = t * t * (3.0f - 2.0f * t);
    t = clampf(t * p.max_blur, 0.0f, 1.0f);
    t = clampf(t, 0.0f, 1.0f);                    // lerp_color
    const float ia = 1.0f - t;
    const uint32_t a = p.sharp[i], b = p.blur[i];
    uint32_t out = 255u << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
        const float v = ia * (float)((a >> sh) & 0xffu) + t * (float)((b >> sh) & 0xffu);
        out |= (uint32_t)(uint8_t)(int)v << sh;   // x86's float -> uint8_t: cvttss2si, low byte
    }
    p.out[i] = out;
}

// ---- light_shafts_pass (hello_pbr_light_shafts.cpp:1390-1707) ----------------------------------------

namespace {

__device__ __forceinline__ float s_min(float a, float b) { return (b < a) ? b : a; }   // std::min, glm::min
__device__ __forceinline__ float s_max(float a, float b) { return (a < b) ? b : a; }   // std::max, glm::max
// (int)f as the reference's x86-64 build converts it (cvttss2si: NaN and out-of-range give INT_MIN)
__device__ __forceinline__ int int_x86(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
// (int)std::lround(x): halves away from zero; NaN and out-of-range land on a value the caller's clamp brings to 0
// or n - 1 as it does the reference's
__device__ __forceinline__ int lround_x86(float x) {
    if (!(x == x)) return 0;
    const float t = truncf(x);
    return int_x86(t) + ((x - t >= 0.5f) ? 1 : 0);
}
// The reference's sinf / cosf / expf / powf are the host libm's, close to correctly rounded: here the function in
// double, rounded once to float (as pow64 and the analytic sky's powers in shs_canvas_rt.hip).
__device__ __forceinline__ float sin_r(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float cos_r(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float exp_r(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float pow15_r(float x) { const double d = (double)x; return (float)(d * sqrt(d)); }
__device__ __forceinline__ float pow_r(float x, float e) { return (float)pow((double)x, (double)e); }

// volumetric_shadow_visibility (:1494-1507) over shadow_uvz_from_world (:558-576) and shadow_factor_pcf_2x2_raw /
// shadow_compare_raw (:1450-1492).  The four loads are unconditional at clamped texels (without the PCF all four
// are the nearest texel); every early return of the reference is a select on what they gave.
__device__ __forceinline__ float ls_visibility(const CanvasLSParams &p, float wx, float wy, float wz) {
    float c[4];
    m4v(p.light_vp, wx, wy, wz, 1.0f, c);
    const float nx = c[0] / c[3], ny = c[1] / c[3], z = c[2] / c[3];
    bool lit = fabsf(c[3]) < 1e-6f || z < 0.0f || z > 1.0f;
    const float u = nx * 0.5f + 0.5f;
    const float v = 1.0f - (ny * 0.5f + 0.5f);
    const float fx = u * (float)(p.sw - 1);
    const float fy = v * (float)(p.sh - 1);
    int x0, y0, x1, y1;
    if (p.pcf) {
        x0 = clampi(int_x86(floorf(fx)), 0, p.sw - 1);
        y0 = clampi(int_x86(floorf(fy)), 0, p.sh - 1);
        x1 = clampi(x0 + 1, 0, p.sw - 1);
        y1 = clampi(y0 + 1, 0, p.sh - 1);
    } else {
        lit = lit || u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f;
        x0 = x1 = clampi(lround_x86(fx), 0, p.sw - 1);
        y0 = y1 = clampi(lround_x86(fy), 0, p.sh - 1);
    }
    const float d00 = p.map[y0 * p.sw + x0], d10 = p.map[y0 * p.sw + x1];
    const float d01 = p.map[y1 * p.sw + x0], d11 = p.map[y1 * p.sw + x1];
    const float c00 = (d00 == FLT_MAX || z <= d00 + p.bias) ? 1.0f : 0.0f;
    const float c10 = (d10 == FLT_MAX || z <= d10 + p.bias) ? 1.0f : 0.0f;
    const float c01 = (d01 == FLT_MAX || z <= d01 + p.bias) ? 1.0f : 0.0f;
    const float c11 = (d11 == FLT_MAX || z <= d11 + p.bias) ? 1.0f : 0.0f;
    const float vis = p.pcf ? 0.25f * (((c00 + c10) + c01) + c11) : c00;
    return lit ? 1.0f : vis;
}

}  // namespace

// One lane per pixel over 32 x 8 pixel tiles: a wave is two rows of 32, whose rays run side by side through the
// shadow map.  SHADOW: p.use_shadow with a map (otherwise vis is 1 and the kernel has no map load).
template <bool SHADOW>
__global__ __launch_bounds__(256) void k_canvas_light_shafts(const CanvasLSParams p) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u));
    const int y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= p.W || y >= p.H) return;
    const int i = y * p.W + x;
    const uint32_t base = p.src[i];
    const float view_z = p.depth[i];
    float ray_max = p.max_dist;
    if (view_z != FLT_MAX) ray_max = s_min(ray_max, s_max(p.min_dist, view_z - 0.25f));
    if (!p.enable || ray_max <= p.min_dist) {
        p.dst[i] = base;
        if (p.pq) p.pq[i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    // reconstruct_world_dir_from_pixel (:1395-1420)
    float vx = 0.0f, vy = 0.0f, vz = 1.0f;
    {
        const int py_screen = (p.H - 1) - y;
        const float fx = ((float)x + 0.5f) / (float)p.W;
        const float fy = ((float)py_screen + 0.5f) / (float)p.H;
        const float ndc_x = fx * 2.0f - 1.0f;
        const float ndc_y = 1.0f - fy * 2.0f;
        float wf[4];
        m4v(p.inv_vp, ndc_x, ndc_y, 1.0f, 1.0f, wf);
        if (!(fabsf(wf[3]) < 1e-8f)) {
            const float dx = wf[0] / wf[3] - p.cam[0], dy = wf[1] / wf[3] - p.cam[1], dz = wf[2] / wf[3] - p.cam[2];
            const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (!(len < 1e-6f)) {
                vx = dx / len;
                vy = dy / len;
                vz = dz / len;
            }
        }
    }
    const float cos_theta = (vx * p.sun[0] + vy * p.sun[1]) + vz * p.sun[2];
    // phase_hg (:1432-1440); g's clamp and its products are the host's
    const float phase = p.one_m_gg / pow15_r(s_max(1e-4f, p.one_p_gg - p.g2 * clampf(cos_theta, -1.0f, 1.0f)));
    const float gate = clampf((cos_theta - 0.1f) / 0.9f, 0.0f, 1.0f);
    const float ds = ray_max / (float)p.steps;
    const uint32_t seed = ((uint32_t)x * 1973u) ^ ((uint32_t)y * 9277u);
    const float random_val = (float)(seed & 0xffffu) / 65536.0f;
    float t = p.min_dist + (random_val * ds) * p.jitter;
    float Tm = 1.0f, lr = 0.0f, lg = 0.0f, lb = 0.0f;
    int acc = 0;
    for (int k = 0; k < p.steps; ++k) {
        if (t >= ray_max) break;
        const float wx = p.cam[0] + vx * t, wy = p.cam[1] + vy * t, wz = p.cam[2] + vz * t;
        float vis = 1.0f;
        if (SHADOW) vis = ls_visibility(p, wx, wy, wz);   // ahead of the density tests: the gathers fly under the sin / cos / exp
        const float h = s_max(0.0f, wy);
        float dens = p.base_density * exp_r(-h * p.height_falloff);   // fog_density (:1423-1429)
        if (dens > 1e-6f) {   // volumetric_cloud_noise (:1516-1522)
            const float sx = wx * p.noise_scale, sy = wy * p.noise_scale, sz = wz * p.noise_scale;
            const float n = (sin_r(sx) * cos_r(sy)) * sin_r(sz + sx * 0.5f);
            const float dust = n * 0.5f + 0.5f;
            dens *= 1.0f * (1.0f - p.noise_strength) + dust * p.noise_strength;
        }
        if (dens > 1e-6f) {
            const float sigma_s = p.sigma_s * dens;
            const float sigma_t = p.sigma_t * dens;
            const float direct_light = (phase * vis) * gate;
            const float light_term = direct_light * p.intensity + p.ambient;
            float scatter = ((Tm * sigma_s) * light_term) * ds;
            const float dist01 = t / p.dist_den;
            const float dist_fall = 1.0f - dist01 * dist01;
            scatter *= dist_fall;
            const float iv = 1.0f - vis;   // glm::mix(ambient_tint, shafts_tint, vis)
            lr += (0.60f * iv + 0.92f * vis) * scatter;
            lg += (0.65f * iv + 0.96f * vis) * scatter;
            lb += (0.70f * iv + 1.00f * vis) * scatter;
            Tm *= exp_r(-sigma_t * ds);
            ++acc;
            if (Tm < 0.01f) break;
        }
        t += ds;
    }
    const float ls[3] = {lr, lg, lb};
    float out[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float o = p.srgb_lut[(base >> (8 * ch)) & 0xffu] + ls[ch];    // srgb_to_linear(color_to_srgb01(base)) + Ls
        o = o / (1.0f + o * 0.15f);
        o = s_min(s_max(o, 0.0f), 1.0f);                              // glm::clamp
        o = pow_r(s_min(s_max(o, 0.0f), 1.0f), 1.0f / 2.2f);          // linear_to_srgb
        out[ch] = s_min(s_max(o, 0.0f), 1.0f) * 255.0f;               // rgb01_to_color before the truncation
    }
    uint32_t rgba = 0xff000000u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) rgba |= (out[ch] == out[ch] ? (uint32_t)(int32_t)out[ch] & 0xffu : 0u) << (8 * ch);
    p.dst[i] = rgba;
    if (p.pq) p.pq[i] = make_float4(out[0], out[1], out[2], (float)acc);
}

}  // namespace shs_dev

namespace shs_internal {
using namespace shs_dev;

static dim3 px_grid(int W, int H) { return dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)); }

hipError_t launch_canvas_motion_blur(const CanvasMBParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_motion_blur, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_gaussian(const uint32_t *src, uint32_t *dst, int W, int H, bool horizontal, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_gaussian, px_grid(W, H), dim3(256), 0, s, src, dst, W, H, horizontal ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_canvas_autofocus(const CanvasDofParams &p, hipStream_t s) {
    if (p.radius < 0 || p.radius > AF_MAX_RADIUS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_canvas_autofocus, dim3(1), dim3(1024), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_dof_composite(const CanvasDofParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_canvas_dof_composite, px_grid(p.W, p.H), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_canvas_light_shafts(const CanvasLSParams &p, hipStream_t s) {
    const dim3 grid((unsigned)((p.W + 31) / 32), (unsigned)((p.H + 7) / 8));
    if (p.map) hipLaunchKernelGGL(k_canvas_light_shafts<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_canvas_light_shafts<false>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace shs_internal
