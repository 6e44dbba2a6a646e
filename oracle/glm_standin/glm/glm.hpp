// glm/glm.hpp -- a GLM STAND-IN, written for this project.  NOT GLM.
//
// TEST INFRASTRUCTURE ONLY.  It exists so that the reference library's own headers
// (sw_render/rasterizer.hpp, shader/builtin_shaders.hpp, lighting/shadow_sample.hpp,
// passes/pass_tonemap.hpp, passes/pass_motion_blur.hpp, core/context.hpp) compile into
// oracle/_ref/libshs_ref_lib.so (oracle/Makefile, oracle/ref_lib.cpp), against which the oracle and
// the GPU kernels are compared word for word.
//
// GLM ITSELF STAYS UNPINNED: GLM is not available to this project's build, so this header restates
// the operation order of GLM's published sources (detail/type_vec*.inl, type_mat*.inl,
// func_common.inl, func_geometric.inl, func_matrix.inl) exactly as csrc/shs_glm.hpp and the g_*
// helpers of oracle/shs_oracle_lib.c state them:
//   dot(vec3)   = (x + y) + z                 dot(vec4) = (x + y) + (z + w)
//   normalize   = v * (1 / sqrt(dot(v, v)))   length    = sqrt(dot(v, v))
//   mix(x,y,a)  = x * (1 - a) + y * a         reflect   = I - N * dot(N, I) * 2
//   min(x, y)   = (y < x) ? y : x             max(x, y) = (x < y) ? y : x
//   clamp       = min(max(x, lo), hi)
//   mat4 * vec4 = (m0 * x + m1 * y) + (m2 * z + m3 * w)
//   mat3 * vec3 = (m0 * x + m1 * y) + m2 * z  (left to right)
//   mat4 * mat4 : column c = ((a0 * b[c].x + a1 * b[c].y) + a2 * b[c].z) + a3 * b[c].w
//   determinant / inverse: the cofactor forms of func_matrix.inl
// It provides only what those reference headers use: vec2/3/4, mat3/4, the constructors and
// component aliases (.x/.r, .y/.g, .z/.b, .w/.a) they name, component-wise operators, and mix,
// normalize, dot, max, min, clamp, reflect, length, determinant, inverse, transpose, pi.
// The trigonometric matrix builders (lookAt, perspective, translate, rotate, ...) are absent on
// purpose: nothing this project compiles against the stand-in may reach them.
#pragma once
#include <cmath>
#include <cstddef>

namespace glm {

struct vec2;
struct vec3;
struct vec4;

struct vec2 {
    union { float x, r, s; };
    union { float y, g, t; };
    constexpr vec2() : x(0.0f), y(0.0f) {}
    constexpr explicit vec2(float v) : x(v), y(v) {}
    constexpr vec2(float a, float b) : x(a), y(b) {}
    explicit vec2(const vec3 &v);
    explicit vec2(const vec4 &v);
    float &operator[](int i) { return i == 0 ? x : y; }
    const float &operator[](int i) const { return i == 0 ? x : y; }
    vec2 &operator*=(float k) { x *= k; y *= k; return *this; }
};

struct vec3 {
    union { float x, r, s; };
    union { float y, g, t; };
    union { float z, b, p; };
    constexpr vec3() : x(0.0f), y(0.0f), z(0.0f) {}
    constexpr explicit vec3(float v) : x(v), y(v), z(v) {}
    constexpr vec3(float a, float b_, float c) : x(a), y(b_), z(c) {}
    explicit vec3(const vec4 &v);
    float &operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    const float &operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    vec3 &operator*=(float k) { x *= k; y *= k; z *= k; return *this; }
};

struct vec4 {
    union { float x, r, s; };
    union { float y, g, t; };
    union { float z, b, p; };
    union { float w, a, q; };
    constexpr vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    constexpr explicit vec4(float v) : x(v), y(v), z(v), w(v) {}
    constexpr vec4(float a_, float b_, float c, float d) : x(a_), y(b_), z(c), w(d) {}
    constexpr vec4(const vec3 &v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
    constexpr vec4(const vec2 &v, float c, float d) : x(v.x), y(v.y), z(c), w(d) {}
    float &operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    const float &operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    vec4 &operator*=(float k) { x *= k; y *= k; z *= k; w *= k; return *this; }
};

inline vec2::vec2(const vec3 &v) : x(v.x), y(v.y) {}
inline vec2::vec2(const vec4 &v) : x(v.x), y(v.y) {}
inline vec3::vec3(const vec4 &v) : x(v.x), y(v.y), z(v.z) {}

// ---- component-wise operators (type_vec2/3/4.inl) ---------------------------------------------
inline vec2 operator+(const vec2 &a, const vec2 &b) { return vec2(a.x + b.x, a.y + b.y); }
inline vec2 operator-(const vec2 &a, const vec2 &b) { return vec2(a.x - b.x, a.y - b.y); }
inline vec2 operator*(const vec2 &a, const vec2 &b) { return vec2(a.x * b.x, a.y * b.y); }
inline vec2 operator*(const vec2 &a, float k) { return vec2(a.x * k, a.y * k); }
inline vec2 operator*(float k, const vec2 &a) { return vec2(k * a.x, k * a.y); }
inline vec2 operator/(const vec2 &a, float k) { return vec2(a.x / k, a.y / k); }
inline vec2 operator-(const vec2 &a) { return vec2(-a.x, -a.y); }

inline vec3 operator+(const vec3 &a, const vec3 &b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3 &a, const vec3 &b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3 &a, const vec3 &b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator*(const vec3 &a, float k) { return vec3(a.x * k, a.y * k, a.z * k); }
inline vec3 operator*(float k, const vec3 &a) { return vec3(k * a.x, k * a.y, k * a.z); }
inline vec3 operator/(const vec3 &a, float k) { return vec3(a.x / k, a.y / k, a.z / k); }
inline vec3 operator-(const vec3 &a) { return vec3(-a.x, -a.y, -a.z); }

inline vec4 operator+(const vec4 &a, const vec4 &b) { return vec4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline vec4 operator-(const vec4 &a, const vec4 &b) { return vec4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
inline vec4 operator*(const vec4 &a, const vec4 &b) { return vec4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
inline vec4 operator*(const vec4 &a, float k) { return vec4(a.x * k, a.y * k, a.z * k, a.w * k); }
inline vec4 operator*(float k, const vec4 &a) { return vec4(k * a.x, k * a.y, k * a.z, k * a.w); }
inline vec4 operator/(const vec4 &a, float k) { return vec4(a.x / k, a.y / k, a.z / k, a.w / k); }
inline vec4 operator-(const vec4 &a) { return vec4(-a.x, -a.y, -a.z, -a.w); }

// ---- func_common.inl ---------------------------------------------------------------------------
inline float min(float x, float y) { return (y < x) ? y : x; }
inline float max(float x, float y) { return (x < y) ? y : x; }
inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }

inline vec2 max(const vec2 &a, const vec2 &b) { return vec2(max(a.x, b.x), max(a.y, b.y)); }
inline vec3 max(const vec3 &a, const vec3 &b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
inline vec4 max(const vec4 &a, const vec4 &b) { return vec4(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z), max(a.w, b.w)); }
inline vec2 min(const vec2 &a, const vec2 &b) { return vec2(min(a.x, b.x), min(a.y, b.y)); }
inline vec3 min(const vec3 &a, const vec3 &b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec4 min(const vec4 &a, const vec4 &b) { return vec4(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z), min(a.w, b.w)); }
inline vec3 clamp(const vec3 &v, float lo, float hi) { return vec3(clamp(v.x, lo, hi), clamp(v.y, lo, hi), clamp(v.z, lo, hi)); }

inline vec2 mix(const vec2 &x, const vec2 &y, float a) { return x * (1.0f - a) + y * a; }
inline vec3 mix(const vec3 &x, const vec3 &y, float a) { return x * (1.0f - a) + y * a; }
inline vec4 mix(const vec4 &x, const vec4 &y, float a) { return x * (1.0f - a) + y * a; }

// ---- func_geometric.inl -------------------------------------------------------------------------
inline float dot(const vec2 &a, const vec2 &b) { const vec2 t = a * b; return t.x + t.y; }
inline float dot(const vec3 &a, const vec3 &b) { const vec3 t = a * b; return t.x + t.y + t.z; }
inline float dot(const vec4 &a, const vec4 &b) { const vec4 t = a * b; return (t.x + t.y) + (t.z + t.w); }
inline float length(const vec2 &v) { return std::sqrt(dot(v, v)); }
inline float length(const vec3 &v) { return std::sqrt(dot(v, v)); }
inline float length(const vec4 &v) { return std::sqrt(dot(v, v)); }
inline float inversesqrt(float x) { return 1.0f / std::sqrt(x); }
inline vec2 normalize(const vec2 &v) { return v * inversesqrt(dot(v, v)); }
inline vec3 normalize(const vec3 &v) { return v * inversesqrt(dot(v, v)); }
inline vec4 normalize(const vec4 &v) { return v * inversesqrt(dot(v, v)); }
inline vec3 reflect(const vec3 &I, const vec3 &N) { return I - N * dot(N, I) * 2.0f; }

// ---- matrices, column-major: m[c][r] (type_mat3x3.inl, type_mat4x4.inl) ---------------------------
struct mat4;

struct mat3 {
    vec3 value[3];
    constexpr mat3() : value{vec3(), vec3(), vec3()} {}
    constexpr explicit mat3(float d) : value{vec3(d, 0.0f, 0.0f), vec3(0.0f, d, 0.0f), vec3(0.0f, 0.0f, d)} {}
    constexpr mat3(const vec3 &c0, const vec3 &c1, const vec3 &c2) : value{c0, c1, c2} {}
    explicit mat3(const mat4 &m);
    vec3 &operator[](int c) { return value[c]; }
    const vec3 &operator[](int c) const { return value[c]; }
};

struct mat4 {
    vec4 value[4];
    constexpr mat4() : value{vec4(), vec4(), vec4(), vec4()} {}
    constexpr explicit mat4(float d)
        : value{vec4(d, 0.0f, 0.0f, 0.0f), vec4(0.0f, d, 0.0f, 0.0f), vec4(0.0f, 0.0f, d, 0.0f), vec4(0.0f, 0.0f, 0.0f, d)} {}
    constexpr mat4(const vec4 &c0, const vec4 &c1, const vec4 &c2, const vec4 &c3) : value{c0, c1, c2, c3} {}
    vec4 &operator[](int c) { return value[c]; }
    const vec4 &operator[](int c) const { return value[c]; }
};

inline mat3::mat3(const mat4 &m) : value{vec3(m[0]), vec3(m[1]), vec3(m[2])} {}

inline vec3 operator*(const mat3 &m, const vec3 &v) {
    return vec3(m[0][0] * v.x + m[1][0] * v.y + m[2][0] * v.z,
                m[0][1] * v.x + m[1][1] * v.y + m[2][1] * v.z,
                m[0][2] * v.x + m[1][2] * v.y + m[2][2] * v.z);
}

inline vec4 operator*(const mat4 &m, const vec4 &v) {
    const vec4 mul0 = m[0] * vec4(v.x), mul1 = m[1] * vec4(v.y);
    const vec4 add0 = mul0 + mul1;
    const vec4 mul2 = m[2] * vec4(v.z), mul3 = m[3] * vec4(v.w);
    const vec4 add1 = mul2 + mul3;
    return add0 + add1;
}

inline mat4 operator*(const mat4 &a, const mat4 &b) {
    mat4 o;
    for (int c = 0; c < 4; ++c) o[c] = a[0] * b[c][0] + a[1] * b[c][1] + a[2] * b[c][2] + a[3] * b[c][3];
    return o;
}

inline mat4 operator*(const mat4 &m, float k) { return mat4(m[0] * k, m[1] * k, m[2] * k, m[3] * k); }

// ---- func_matrix.inl ------------------------------------------------------------------------------
inline mat3 transpose(const mat3 &m) {
    mat3 o;
    for (int c = 0; c < 3; ++c)
        for (int r_ = 0; r_ < 3; ++r_) o[c][r_] = m[r_][c];
    return o;
}

inline float determinant(const mat3 &m) {
    return +m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2])
           - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2])
           + m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]);
}

inline mat3 inverse(const mat3 &m) {
    const float one_over = 1.0f / determinant(m);
    mat3 o;
    o[0][0] = +(m[1][1] * m[2][2] - m[2][1] * m[1][2]) * one_over;
    o[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * one_over;
    o[2][0] = +(m[1][0] * m[2][1] - m[2][0] * m[1][1]) * one_over;
    o[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * one_over;
    o[1][1] = +(m[0][0] * m[2][2] - m[2][0] * m[0][2]) * one_over;
    o[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * one_over;
    o[0][2] = +(m[0][1] * m[1][2] - m[1][1] * m[0][2]) * one_over;
    o[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * one_over;
    o[2][2] = +(m[0][0] * m[1][1] - m[1][0] * m[0][1]) * one_over;
    return o;
}

inline float determinant(const mat4 &m) {
    const float s00 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
    const float s01 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
    const float s02 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
    const float s03 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
    const float s04 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
    const float s05 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
    const vec4 coef(+(m[1][1] * s00 - m[1][2] * s01 + m[1][3] * s02),
                    -(m[1][0] * s00 - m[1][2] * s03 + m[1][3] * s04),
                    +(m[1][0] * s01 - m[1][1] * s03 + m[1][3] * s05),
                    -(m[1][0] * s02 - m[1][1] * s04 + m[1][2] * s05));
    return m[0][0] * coef[0] + m[0][1] * coef[1] + m[0][2] * coef[2] + m[0][3] * coef[3];
}

inline mat4 inverse(const mat4 &m) {
    const float c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3];
    const float c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3];
    const float c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
    const float c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
    const float c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3];
    const float c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
    const float c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2];
    const float c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2];
    const float c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
    const float c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
    const float c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3];
    const float c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
    const float c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2];
    const float c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2];
    const float c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
    const float c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
    const float c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1];
    const float c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
    const vec4 fac0(c00, c00, c02, c03), fac1(c04, c04, c06, c07), fac2(c08, c08, c10, c11);
    const vec4 fac3(c12, c12, c14, c15), fac4(c16, c16, c18, c19), fac5(c20, c20, c22, c23);
    const vec4 v0(m[1][0], m[0][0], m[0][0], m[0][0]);
    const vec4 v1(m[1][1], m[0][1], m[0][1], m[0][1]);
    const vec4 v2(m[1][2], m[0][2], m[0][2], m[0][2]);
    const vec4 v3(m[1][3], m[0][3], m[0][3], m[0][3]);
    const vec4 inv0(v1 * fac0 - v2 * fac1 + v3 * fac2);
    const vec4 inv1(v0 * fac0 - v2 * fac3 + v3 * fac4);
    const vec4 inv2(v0 * fac1 - v1 * fac3 + v3 * fac5);
    const vec4 inv3(v0 * fac2 - v1 * fac4 + v2 * fac5);
    const vec4 sign_a(+1.0f, -1.0f, +1.0f, -1.0f), sign_b(-1.0f, +1.0f, -1.0f, +1.0f);
    const mat4 inv(inv0 * sign_a, inv1 * sign_b, inv2 * sign_a, inv3 * sign_b);
    const vec4 row0(inv[0][0], inv[1][0], inv[2][0], inv[3][0]);
    const vec4 dot0(m[0] * row0);
    const float dot1 = (dot0.x + dot0.y) + (dot0.z + dot0.w);
    const float one_over = 1.0f / dot1;
    return inv * one_over;
}

}  // namespace glm
