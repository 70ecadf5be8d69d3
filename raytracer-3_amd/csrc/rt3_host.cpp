// rt3_host.cpp — host half of librt3hip.so: the scene API that runs before the render path
// (entities -> GFace[] / vec4[]), camera set-up, PPM serialisation, benchmark scene builders.
//
// Everything here is ordinary CPU code in the reference too (src/lib/entities/*.cpp, src/lib/camera/*.cpp);
// the render path itself (rt3_render*, rt3_render_path*) lives in rt3_device.hip and has no CPU form.
// Compiled with -ffp-contract=off: the reference's flattening is plain IEEE binary32 with libm double trig.
#include "rt3.h"
#include "rt3_sphere_plan.hpp"
#include "rt3_env_sample.hpp"
#include "rt3_light_sample.hpp"
#include "rt3_display_law.hpp"
#include "rt3_display_sequence_law.hpp"
#include "rt3_lens_law.hpp"
#include "rt3_texture_law.hpp"
#include "rt3_aov_chain_law.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace {

struct Vec3 {
    float x, y, z;
    Vec3() : x(0), y(0), z(0) {}
    Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    explicit Vec3(const float* p) : x(p[0]), y(p[1]), z(p[2]) {}
};
inline Vec3 operator+(Vec3 a, Vec3 b) { return Vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Vec3 operator-(Vec3 a, Vec3 b) { return Vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline Vec3 operator*(float s, Vec3 a) { return Vec3(s * a.x, s * a.y, s * a.z); }
inline Vec3 operator*(Vec3 a, float s) { return Vec3(a.x * s, a.y * s, a.z * s); }
inline Vec3 operator/(Vec3 a, Vec3 b) { return Vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
// glm::dot / glm::cross / glm::normalize as the reference's vendored GLM 0.9.9.8 evaluates them
// (glm/detail/func_geometric.inl:48-55, :68-79, :82-90): sums left to right, normalize = v * (1/sqrt(v.v)).
inline float dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline Vec3 cross(Vec3 a, Vec3 b) { return Vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
inline Vec3 normalize(Vec3 v) { return v * (1.0f / std::sqrt(dot(v, v))); }

inline void put_vertex(float* vertices, uint32_t index, Vec3 p) {
    float* v = vertices + 4 * (size_t)index;
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = 0.0f;
}
inline void put_face(rt3_gface& f, uint32_t a, uint32_t b, uint32_t c, Vec3 n, Vec3 col) {
    std::memset(&f, 0, sizeof f);
    f.v1 = a; f.v2 = b; f.v3 = c;
    f.normal[0] = n.x; f.normal[1] = n.y; f.normal[2] = n.z;
    f.color[0] = col.x; f.color[1] = col.y; f.color[2] = col.z;
}
// colour * |n . (0,0,-1)|  — the baked "headlight" shading of Sphere.cpp:155 and Object.cpp:194.
inline Vec3 bake(Vec3 color, Vec3 n) { return color * std::fabs(dot(n, Vec3(0.0f, 0.0f, -1.0f))); }

// One point of the UV sphere, Sphere.cpp:69-79 (double-precision trig, float everything else).
struct UvSphere {
    Vec3 center; float radius; uint32_t meridians, parallels;
    Vec3 at(uint32_t ix, uint32_t iy) const {
        const float fx = (float)ix, fy = (float)iy;
        const double theta = M_PI * (fy / (float)(parallels - 1));
        const double phi = 2 * M_PI * (fx / (float)meridians);
        return center + radius * Vec3((float)(std::sin(theta) * std::cos(phi)), (float)std::cos(theta),
                                      (float)(std::sin(theta) * std::sin(phi)));
    }
    // vertex index of ring iy (1..parallels-2), column ix
    uint32_t ring(uint32_t iy, uint32_t ix) const { return 1 + (iy - 1) * meridians + ix; }
};

}  // namespace

extern "C" {

void rt3_prerender_triangle(const float p1[3], const float p2[3], const float p3[3], const float color[3],
                            rt3_gface* faces, float* vertices) {
    const Vec3 a(p1), b(p2), c(p3);
    put_vertex(vertices, 0, a);
    put_vertex(vertices, 1, b);
    put_vertex(vertices, 2, c);
    put_face(faces[0], 0, 1, 2, normalize(cross(c - a, b - a)), Vec3(color));   // Triangle.cpp:48, colour unshaded
}

uint32_t rt3_sphere_face_count(uint32_t m, uint32_t p) { return m + 2 * ((p - 3) * m) + m; }
uint32_t rt3_sphere_vertex_count(uint32_t m, uint32_t p) { return 2 + (p - 2) * m; }

// Sphere.cpp:120-261.  The reference walks (y, x) and rewrites shared vertices several times with identical
// values; here vertices are written once, then faces ring by ring — same arrays.
void rt3_prerender_sphere(const float center[3], float radius, uint32_t m, uint32_t p, const float color[3],
                          rt3_gface* faces, float* vertices) {
    const UvSphere s{ Vec3(center), radius, m, p };
    const Vec3 col(color);
    const uint32_t south = 1 + (p - 2) * m;

    put_vertex(vertices, 0, s.at(0, 0));
    for (uint32_t iy = 1; iy + 1 < p; iy++)
        for (uint32_t ix = 0; ix < m; ix++) put_vertex(vertices, s.ring(iy, ix), s.at(ix, iy));
    put_vertex(vertices, south, s.at(0, p - 1));

    for (uint32_t ix = 0; ix < m; ix++) {                       // north cap, faces [0, m)
        const uint32_t prev = ix > 0 ? ix - 1 : m - 1;
        const Vec3 v1 = s.at(0, 0), v2 = s.at(prev, 1), v3 = s.at(ix, 1);
        const Vec3 n = normalize(cross(v3 - v1, v2 - v1));
        put_face(faces[ix], 0, 1 + prev, 1 + ix, n, bake(col, n));
    }
    for (uint32_t iy = 2; iy + 1 < p; iy++) {                   // quads between ring iy-1 and ring iy
        const uint32_t base = m + 2 * (iy - 2) * m;
        for (uint32_t ix = 0; ix < m; ix++) {
            const uint32_t prev = ix > 0 ? ix - 1 : m - 1;
            const Vec3 v1 = s.at(prev, iy - 1), v2 = s.at(ix, iy - 1), v3 = s.at(prev, iy), v4 = s.at(ix, iy);
            const Vec3 n1 = normalize(cross(v4 - v1, v3 - v1)), n2 = normalize(cross(v4 - v1, v2 - v1));
            const uint32_t i1 = s.ring(iy - 1, prev), i2 = s.ring(iy - 1, ix), i3 = s.ring(iy, prev), i4 = s.ring(iy, ix);
            put_face(faces[base + 2 * ix], i1, i3, i4, n1, bake(col, n1));
            put_face(faces[base + 2 * ix + 1], i1, i2, i4, n2, bake(col, n2));
        }
    }
    {                                                           // south cap
        const uint32_t iy = p - 1, base = m + 2 * (iy - 2) * m;
        for (uint32_t ix = 0; ix < m; ix++) {
            const uint32_t prev = ix > 0 ? ix - 1 : m - 1;
            const Vec3 v1 = s.at(0, iy), v2 = s.at(prev, iy - 1), v3 = s.at(ix, iy - 1);
            const Vec3 n = normalize(cross(v3 - v1, v2 - v1));
            put_face(faces[base + ix], south, s.ring(iy - 1, prev), s.ring(iy - 1, ix), n, bake(col, n));
        }
    }
}

// Object.cpp:84-119 — every line must read as `char float float float`, otherwise the reference aborts.
int rt3_object_count(const char* path, uint32_t* n_faces, uint32_t* n_vertices) {
    std::ifstream in(path);
    if (!in.is_open()) return RT3_E_IO;
    uint32_t nf = 0, nv = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        char kind; float a, b, c;
        if (!(ss >> kind >> a >> b >> c)) return RT3_E_IO;
        if (kind == 'f') ++nf; else if (kind == 'v') ++nv;
    }
    *n_faces = nf; *n_vertices = nv;
    return 0;
}

// Object.cpp:131-199.
int rt3_prerender_object(const char* path, const float center[3], float scale, const float color[3],
                         rt3_gface* faces, uint32_t n_faces, float* vertices, uint32_t n_vertices) {
    std::ifstream in(path);
    if (!in.is_open()) return RT3_E_IO;
    const Vec3 origin(center), col(color);
    uint32_t nf = 0, nv = 0;
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        char kind; float a, b, c;
        if (!(ss >> kind >> a >> b >> c)) return RT3_E_IO;
        if (kind == 'v') {
            if (nv >= n_vertices) return RT3_E_ARG;
            put_vertex(vertices, nv++, origin + scale * Vec3(a, b, c));
        } else if (kind == 'f') {
            if (nf >= n_faces) return RT3_E_ARG;
            // indices arrive as floats (Object.cpp:157-170); the reference casts blindly, here anything that is not a
            // representable index is a malformed file (the cast of a negative, non-finite or >= 2^32 float is undefined)
            auto index_ok = [](float x) { return x >= 0.0f && x < 4294967296.0f; };     // false for NaN
            if (!index_ok(a) || !index_ok(b) || !index_ok(c)) return RT3_E_IO;
            put_face(faces[nf++], (uint32_t)a, (uint32_t)b, (uint32_t)c, Vec3(), col);
        }
    }
    uint32_t lowest = 0xFFFFFFFFu;                              // indices need not be zero-based (:181-186)
    for (uint32_t i = 0; i < nf; i++) {
        lowest = faces[i].v1 < lowest ? faces[i].v1 : lowest;
        lowest = faces[i].v2 < lowest ? faces[i].v2 : lowest;
        lowest = faces[i].v3 < lowest ? faces[i].v3 : lowest;
    }
    for (uint32_t i = 0; i < nf; i++) {
        rt3_gface& f = faces[i];
        f.v1 -= lowest; f.v2 -= lowest; f.v3 -= lowest;
        if (f.v1 >= nv || f.v2 >= nv || f.v3 >= nv) return RT3_E_IO;         // a face names a vertex the file does not hold
        const Vec3 a(vertices + 4 * (size_t)f.v1), b(vertices + 4 * (size_t)f.v2), c(vertices + 4 * (size_t)f.v3);
        const Vec3 n = normalize(cross(c - a, b - a));
        const Vec3 shaded = bake(Vec3(f.color), n);
        f.normal[0] = n.x; f.normal[1] = n.y; f.normal[2] = n.z;
        f.color[0] = shaded.x; f.color[1] = shaded.y; f.color[2] = shaded.z;
    }
    return 0;
}

// SequentialRenderer.cpp:174-195.
void rt3_transfer_entity(rt3_gface* dst_faces, uint32_t* dst_nf, float* dst_vertices, uint32_t* dst_nv,
                         const rt3_gface* faces, uint32_t nf, const float* vertices, uint32_t nv) {
    const uint32_t rebase = *dst_nv;
    rt3_gface* out = dst_faces + *dst_nf;
    for (uint32_t i = 0; i < nf; i++) {
        out[i] = faces[i];
        out[i].v1 += rebase; out[i].v2 += rebase; out[i].v3 += rebase;
    }
    std::memcpy(dst_vertices + 4 * (size_t)rebase, vertices, sizeof(float) * 4 * (size_t)nv);
    *dst_nf += nf;
    *dst_nv += nv;
}

// Camera.cpp:89-92.
void rt3_camera_update(rt3_camera* cam, float focal_length, float viewport_width, float viewport_height) {
    const Vec3 origin(0.0f, 0.0f, 0.0f), horizontal(viewport_width, 0.0f, 0.0f), vertical(0.0f, viewport_height, 0.0f);
    const Vec3 two(2.0f, 2.0f, 2.0f);
    const Vec3 llc = origin - horizontal / two - vertical / two - Vec3(0.0f, 0.0f, focal_length);
    std::memcpy(cam->origin, &origin, 12);
    std::memcpy(cam->horizontal, &horizontal, 12);
    std::memcpy(cam->vertical, &vertical, 12);
    std::memcpy(cam->lower_left_corner, &llc, 12);
}

// Book camera (look-from / look-at) expressed in the reference's four vectors.  Build-owned extension.
void rt3_camera_look_at(rt3_camera* cam, const float from[3], const float at[3], const float vup[3],
                        float vfov_deg, float aspect, float focus_dist) {
    const double theta = (double)vfov_deg * M_PI / 180.0;
    const float half_h = (float)std::tan(theta / 2.0);
    const float vh = 2.0f * half_h * focus_dist, vw = vh * aspect;
    const Vec3 f(from), a(at), up(vup);
    const Vec3 w = normalize(f - a), u = normalize(cross(up, w)), v = cross(w, u);
    const Vec3 horizontal = vw * u, vertical = vh * v;
    const Vec3 llc = f - 0.5f * horizontal - 0.5f * vertical - focus_dist * w;
    std::memcpy(cam->origin, &f, 12);
    std::memcpy(cam->horizontal, &horizontal, 12);
    std::memcpy(cam->vertical, &vertical, 12);
    std::memcpy(cam->lower_left_corner, &llc, 12);
}

// Frame.cpp:125-143.
uint64_t rt3_frame_ppm_bytes(const uint32_t* pixels, uint32_t width, uint32_t height, uint8_t* out, uint64_t cap) {
    const std::string header = "P6\n# Image rendered by the RayTracer-3\n" + std::to_string(width) + " " +
                               std::to_string(height) + "\n255\n";
    const uint64_t total = header.size() + 3ull * width * height;
    if (out == nullptr) return total;
    if (cap < total) return 0;
    std::memcpy(out, header.data(), header.size());
    uint8_t* p = out + header.size();
    for (uint64_t i = 0, n = (uint64_t)width * height; i < n; i++) {
        const uint32_t px = pixels[i];
        *p++ = (uint8_t)(px >> 24); *p++ = (uint8_t)(px >> 16); *p++ = (uint8_t)(px >> 8);
    }
    return total;
}

int rt3_frame_to_ppm(const uint32_t* pixels, uint32_t width, uint32_t height, const char* path) {
    std::vector<uint8_t> bytes(rt3_frame_ppm_bytes(pixels, width, height, nullptr, 0));
    rt3_frame_ppm_bytes(pixels, width, height, bytes.data(), bytes.size());
    FILE* f = std::fopen(path, "wb");
    if (!f) return RT3_E_IO;
    const size_t n = std::fwrite(bytes.data(), 1, bytes.size(), f);
    std::fclose(f);
    return n == bytes.size() ? 0 : RT3_E_IO;
}

// Portable float map (PF: 3 channels, Pf: 1), scale -1.0 = little-endian floats, rows from the bottom of the image up.  The floats are copied
// bit for bit (inf and NaN included).
uint64_t rt3_frame_pfm_bytes(const float* data, uint32_t width, uint32_t height, uint32_t channels, uint32_t stride_floats, uint8_t* out,
                             uint64_t cap) {
    if ((channels != 1 && channels != 3) || stride_floats < channels || width == 0 || height == 0) return 0;
    const std::string header = std::string(channels == 3 ? "PF" : "Pf") + "\n" + std::to_string(width) + " " + std::to_string(height) + "\n-1.0\n";
    const uint64_t total = header.size() + 4ull * channels * width * height;
    if (out == nullptr) return total;
    if (cap < total || data == nullptr) return 0;
    std::memcpy(out, header.data(), header.size());
    uint8_t* p = out + header.size();
    for (uint32_t r = 0; r < height; r++) {
        const float* row = data + (uint64_t)(height - 1 - r) * width * stride_floats;
        for (uint32_t x = 0; x < width; x++)
            for (uint32_t c = 0; c < channels; c++) {
                const float v = row[(uint64_t)x * stride_floats + c];
                uint32_t bits;
                std::memcpy(&bits, &v, 4);
                *p++ = (uint8_t)bits; *p++ = (uint8_t)(bits >> 8); *p++ = (uint8_t)(bits >> 16); *p++ = (uint8_t)(bits >> 24);
            }
    }
    return total;
}

int rt3_frame_to_pfm(const float* data, uint32_t width, uint32_t height, uint32_t channels, uint32_t stride_floats, const char* path) {
    const uint64_t need = rt3_frame_pfm_bytes(data, width, height, channels, stride_floats, nullptr, 0);
    if (need == 0 || data == nullptr || path == nullptr) return RT3_E_ARG;
    std::vector<uint8_t> bytes(need);
    rt3_frame_pfm_bytes(data, width, height, channels, stride_floats, bytes.data(), bytes.size());
    FILE* f = std::fopen(path, "wb");
    if (!f) return RT3_E_IO;
    const size_t n = std::fwrite(bytes.data(), 1, bytes.size(), f);
    std::fclose(f);
    return n == bytes.size() ? 0 : RT3_E_IO;
}

// random_v1.glsl:22-29 and :37-52.
uint32_t rt3_hash_u32(uint32_t x) {
    x += x << 10; x ^= x >> 6; x += x << 3; x ^= x >> 11; x += x << 15;
    return x;
}
float rt3_random_float(uint32_t m) {
    const uint32_t bits = (m & 0x007FFFFFu) | 0x3F800000u;
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f - 1.0f;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------
// Benchmark scenes.  xi(seed, slot, dim) = random(hash(uvec2(hash(uvec2(slot*8+dim, seed)))).
// ------------------------------------------------------------------------------------------------------
namespace {

inline float xi(uint32_t seed, uint32_t slot, uint32_t dim) {
    const uint32_t key = slot * 8u + dim + 1u;                  // never hash a zero key: hash(0) == 0
    return rt3_random_float(rt3_hash_u32(key ^ rt3_hash_u32(seed)));
}

struct SphereSink {
    float* cr; rt3_material* mats; uint32_t cap; uint32_t n;
    void add(float x, float y, float z, float r, uint32_t kind, float cr_, float cg, float cb, float param) {
        if (cr != nullptr && n < cap) {
            float* s = cr + 4 * (size_t)n;
            s[0] = x; s[1] = y; s[2] = z; s[3] = r;
            rt3_material& m = mats[n];
            m.rgb[0] = cr_; m.rgb[1] = cg; m.rgb[2] = cb; m.param = param; m.kind = kind;
        }
        n++;
    }
};

}  // namespace

extern "C" {

// BASELINE.json config 1: ground + two r=0.5 spheres, all Lambertian.
uint32_t rt3_scene_three_spheres(float* center_radius, rt3_material* materials, uint32_t cap) {
    SphereSink out{ center_radius, materials, cap, 0 };
    out.add(0.0f, -100.5f, -1.0f, 100.0f, RT3_MAT_LAMBERT, 0.8f, 0.8f, 0.0f, 0.0f);
    out.add(0.0f, 0.0f, -1.0f, 0.5f, RT3_MAT_LAMBERT, 0.7f, 0.3f, 0.3f, 0.0f);
    out.add(1.0f, 0.0f, -1.0f, 0.5f, RT3_MAT_LAMBERT, 0.8f, 0.6f, 0.2f, 0.0f);
    return out.n;
}

// BASELINE.json config 2/3: the book's final scene.  22x22 grid of r=0.2 spheres, jittered, minus those within
// 0.9 of (4, 0.2, 0); material by xi: <0.8 Lambertian (albedo xi*xi), <0.95 metal (albedo in [0.5,1), fuzz in
// [0,0.5)), else glass 1.5; plus ground r=1000 and three r=1 spheres.
uint32_t rt3_scene_weekend(uint32_t seed, float* center_radius, rt3_material* materials, uint32_t cap) {
    SphereSink out{ center_radius, materials, cap, 0 };
    out.add(0.0f, -1000.0f, 0.0f, 1000.0f, RT3_MAT_LAMBERT, 0.5f, 0.5f, 0.5f, 0.0f);
    uint32_t slot = 0;
    for (int a = -11; a < 11; a++) {
        for (int b = -11; b < 11; b++, slot++) {
            const float choose = xi(seed, slot, 0);
            const float cx = (float)a + 0.9f * xi(seed, slot, 1), cy = 0.2f, cz = (float)b + 0.9f * xi(seed, slot, 2);
            const float dx = cx - 4.0f, dy = cy - 0.2f, dz = cz - 0.0f;
            if (!(std::sqrt(dx * dx + dy * dy + dz * dz) > 0.9f)) continue;
            if (choose < 0.8f) {
                out.add(cx, cy, cz, 0.2f, RT3_MAT_LAMBERT, xi(seed, slot, 3) * xi(seed, slot, 4),
                        xi(seed, slot, 5) * xi(seed, slot, 6), xi(seed, slot, 7) * xi(seed, slot + 65536u, 0), 0.0f);
            } else if (choose < 0.95f) {
                out.add(cx, cy, cz, 0.2f, RT3_MAT_METAL, 0.5f + 0.5f * xi(seed, slot, 3), 0.5f + 0.5f * xi(seed, slot, 4),
                        0.5f + 0.5f * xi(seed, slot, 5), 0.5f * xi(seed, slot, 6));
            } else {
                out.add(cx, cy, cz, 0.2f, RT3_MAT_DIELECTRIC, 1.0f, 1.0f, 1.0f, 1.5f);
            }
        }
    }
    out.add(0.0f, 1.0f, 0.0f, 1.0f, RT3_MAT_DIELECTRIC, 1.0f, 1.0f, 1.0f, 1.5f);
    out.add(-4.0f, 1.0f, 0.0f, 1.0f, RT3_MAT_LAMBERT, 0.4f, 0.2f, 0.1f, 0.0f);
    out.add(4.0f, 1.0f, 0.0f, 1.0f, RT3_MAT_METAL, 0.7f, 0.6f, 0.5f, 0.0f);
    return out.n;
}

// BASELINE.json config 4: n Lambertian spheres, centres uniform in [-50,50]x[0.2,20]x[-100,0], r in [0.05,0.4].
uint32_t rt3_scene_stress(uint32_t n, uint32_t seed, float* center_radius, rt3_material* materials, uint32_t cap) {
    SphereSink out{ center_radius, materials, cap, 0 };
    for (uint32_t i = 0; i < n; i++) {
        out.add(-50.0f + 100.0f * xi(seed, i, 0), 0.2f + 19.8f * xi(seed, i, 1), -100.0f * xi(seed, i, 2),
                0.05f + 0.35f * xi(seed, i, 3), RT3_MAT_LAMBERT, 0.1f + 0.8f * xi(seed, i, 4), 0.1f + 0.8f * xi(seed, i, 5),
                0.1f + 0.8f * xi(seed, i, 6), 0.0f);
    }
    return out.n;
}

}  // extern "C"

// Cornell-style box (BASELINE.json config 5): five walls and two boxes, each rectangle split into grid x grid
// quads of two triangles, plus a two-triangle emissive quad under the ceiling.  Unindexed (3 vertices per face).
namespace {

struct MeshSink {
    rt3_gface* faces; float* vertices; rt3_material* mats; uint32_t cap; uint32_t n;
    void tri(Vec3 a, Vec3 b, Vec3 c, const rt3_material& m) {
        if (faces != nullptr && n < cap) {
            const float col[3] = { m.rgb[0], m.rgb[1], m.rgb[2] };
            const float pa[3] = { a.x, a.y, a.z }, pb[3] = { b.x, b.y, b.z }, pc[3] = { c.x, c.y, c.z };
            rt3_prerender_triangle(pa, pb, pc, col, faces + n, vertices + 12 * (size_t)n);
            faces[n].v1 = 3 * n; faces[n].v2 = 3 * n + 1; faces[n].v3 = 3 * n + 2;
            if (mats != nullptr) mats[n] = m;
        }
        n++;
    }
    // rectangle o + s*eu + t*ev, s,t in [0,1], tessellated g x g
    void rect(Vec3 o, Vec3 eu, Vec3 ev, uint32_t g, const rt3_material& m) {
        for (uint32_t j = 0; j < g; j++)
            for (uint32_t i = 0; i < g; i++) {
                const float s0 = (float)i / (float)g, s1 = (float)(i + 1) / (float)g;
                const float t0 = (float)j / (float)g, t1 = (float)(j + 1) / (float)g;
                const Vec3 p00 = o + s0 * eu + t0 * ev, p10 = o + s1 * eu + t0 * ev;
                const Vec3 p01 = o + s0 * eu + t1 * ev, p11 = o + s1 * eu + t1 * ev;
                tri(p00, p10, p11, m);
                tri(p00, p11, p01, m);
            }
    }
    void box(Vec3 lo, Vec3 hi, uint32_t g, const rt3_material& m) {
        const Vec3 dx(hi.x - lo.x, 0, 0), dy(0, hi.y - lo.y, 0), dz(0, 0, hi.z - lo.z);
        rect(lo, dx, dy, g, m); rect(lo + dz, dx, dy, g, m);
        rect(lo, dz, dy, g, m); rect(lo + dx, dz, dy, g, m);
        rect(lo, dx, dz, g, m); rect(lo + dy, dx, dz, g, m);
    }
};

inline rt3_material mat(uint32_t kind, float r, float g, float b, float param = 0.0f) {
    rt3_material m; m.rgb[0] = r; m.rgb[1] = g; m.rgb[2] = b; m.param = param; m.kind = kind; return m;
}

}  // namespace

extern "C" uint32_t rt3_scene_cornell(uint32_t grid, rt3_gface* faces, float* vertices, rt3_material* face_materials,
                                      uint32_t cap_faces) {
    MeshSink out{ faces, vertices, face_materials, cap_faces, 0 };
    const rt3_material white = mat(RT3_MAT_LAMBERT, 0.73f, 0.73f, 0.73f), red = mat(RT3_MAT_LAMBERT, 0.65f, 0.05f, 0.05f);
    const rt3_material green = mat(RT3_MAT_LAMBERT, 0.12f, 0.45f, 0.15f), light = mat(RT3_MAT_FLAT, 15.0f, 15.0f, 15.0f);
    // box spans x,y in [-1,1], z in [-4,-2]; the camera of Camera::update sits at the origin looking down -z
    out.rect(Vec3(-1, -1, -2), Vec3(0, 0, -2), Vec3(0, 2, 0), grid, red);       // left
    out.rect(Vec3(1, -1, -2), Vec3(0, 0, -2), Vec3(0, 2, 0), grid, green);      // right
    out.rect(Vec3(-1, -1, -2), Vec3(2, 0, 0), Vec3(0, 0, -2), grid, white);     // floor
    out.rect(Vec3(-1, 1, -2), Vec3(2, 0, 0), Vec3(0, 0, -2), grid, white);      // ceiling
    out.rect(Vec3(-1, -1, -4), Vec3(2, 0, 0), Vec3(0, 2, 0), grid, white);      // back
    const uint32_t gb = grid / 4 > 0 ? grid / 4 : 1;
    out.box(Vec3(-0.65f, -1.0f, -3.6f), Vec3(-0.05f, 0.2f, -3.0f), gb, white);  // tall box
    out.box(Vec3(0.1f, -1.0f, -3.0f), Vec3(0.7f, -0.4f, -2.4f), gb, white);     // short box
    out.rect(Vec3(-0.25f, 0.998f, -3.25f), Vec3(0.5f, 0, 0), Vec3(0, 0, 0.5f), 1, light);
    return out.n;
}

// Tests only: what rt3_set_spheres decides before it builds anything (rt3_sphere_plan.hpp, unchanged) — no device, no context.
// The environment map's lookup law (rt3.h) on the host: the device's env_lookup operation for operation — IEEE f32, each rounded on its
// own (this file is compiled with -ffp-contract=off), no fused multiply-add.
namespace {
inline void env_axis(float c, float m, uint32_t n, uint32_t& i0, uint32_t& i1, float& w) {
    const float q = c / m;
    const float u = q * 0.5f + 0.5f;
    const float f = u * (float)n - 0.5f;
    const float f0 = std::floor(f);
    w = f - f0;
    const int k = (int)std::fmin(std::fmax(f0, -1.0f), (float)n - 1.0f);
    i0 = (uint32_t)(k > 0 ? k : 0);
    i1 = (uint32_t)(k + 1 < (int)n - 1 ? k + 1 : (int)n - 1);
}
}  // namespace
extern "C" int rt3_debug_environment_lookup(const float* rgba, uint32_t n, const float d[3], float out_rgb[3]) {
    if (!rgba || !d || !out_rgb || n == 0 || n > RT3_ENV_MAX_FACE) return RT3_E_ARG;
    const float x = d[0], y = d[1], z = d[2];
    const float ax = std::fabs(x), ay = std::fabs(y), az = std::fabs(z);
    uint32_t f; float m, sc, tc;
    if (ax >= ay && ax >= az) { f = x < 0.0f ? 1u : 0u; m = ax; sc = x < 0.0f ? z : -z; tc = -y; }
    else if (ay >= az)        { f = y < 0.0f ? 3u : 2u; m = ay; sc = x; tc = y < 0.0f ? -z : z; }
    else                      { f = z < 0.0f ? 5u : 4u; m = az; sc = z < 0.0f ? -x : x; tc = -y; }
    uint32_t i0, i1, j0, j1; float wx, wy;
    env_axis(sc, m, n, i0, i1, wx);
    env_axis(tc, m, n, j0, j1, wy);
    const float* row0 = rgba + 4 * (((size_t)f * n + j0) * n);
    const float* row1 = rgba + 4 * (((size_t)f * n + j1) * n);
    for (int c = 0; c < 3; c++) {
        const float c00 = row0[4 * (size_t)i0 + c], c10 = row0[4 * (size_t)i1 + c], c01 = row1[4 * (size_t)i0 + c], c11 = row1[4 * (size_t)i1 + c];
        const float top = c00 + wx * (c10 - c00);
        const float bot = c01 + wx * (c11 - c01);
        out_rgb[c] = top + wy * (bot - top);
    }
    return 0;
}

// The sampling table and the sampling law (rt3.h) on the host: the table built cell after cell — the device builds it in any order and
// gets the same integers — then rt3env::sample, the very function shade_lane calls.  The entry point takes one (base, depth) per call and the tests make
// thousands on one map, so the last map's table is kept, with a copy of the map that every call compares (a table is never reused for other texels).
namespace {
struct HostEnvTable {
    std::vector<float> rgba; uint32_t n = 0;
    std::vector<uint32_t> q; std::vector<uint64_t> cdf; uint64_t total = 0;
    void build(const float* map, uint32_t n_face) {
        const uint32_t m = rt3env::cells_per_edge(n_face), cells = 6u * m * m;
        rgba.assign(map, map + (size_t)24 * n_face * n_face);
        n = n_face;
        std::vector<float> w(cells);
        float w_max = 0.0f;
        for (uint32_t k = 0; k < cells; k++) {
            const uint32_t face = k / (m * m), in = k - face * (m * m), row = in / m, col = in - row * m;
            w[k] = rt3env::cell_weight(map, n_face, m, face, row, col);
            if (w[k] > w_max) w_max = w[k];
        }
        q.resize(cells); cdf.resize(cells);
        total = 0;
        for (uint32_t k = 0; k < cells; k++) { q[k] = rt3env::quantise(w[k], w_max); total += q[k]; cdf[k] = total; }
    }
};
}  // namespace
extern "C" int rt3_debug_environment_sample(const float* rgba, uint32_t n, uint32_t base, uint32_t depth, uint32_t* cell, float dir[3], float* pdf) {
    if (!rgba || !cell || !dir || !pdf || n == 0 || n > RT3_ENV_MAX_FACE) return RT3_E_ARG;
    static thread_local HostEnvTable T;
    if (T.n != n || std::memcmp(T.rgba.data(), rgba, T.rgba.size() * sizeof(float)) != 0) T.build(rgba, n);
    if (T.total == 0) { *cell = 0xFFFFFFFFu; dir[0] = dir[1] = dir[2] = 0.0f; *pdf = 0.0f; return 0; }
    rt3env::Sample S;
    rt3env::sample(T.q.data(), T.cdf.data(), rt3env::cells_per_edge(n), T.total, base, depth, S);
    *cell = S.cell; dir[0] = S.dx; dir[1] = S.dy; dir[2] = S.dz; *pdf = S.pdf;
    return 0;
}

// The emitters' sampling table and sampling law (rt3.h "Emitters: sampling") on the host: the table built entry after entry — the device
// builds it in any order and gets the same integers — then rt3light::pick and the point functions, the very ones shade_lane calls.  One (base, depth)
// per call and thousands of calls per scene in the tests, so the last scene's table is kept with a copy of the arrays that every call compares.
namespace {
struct HostLightTable {
    std::vector<uint8_t> key;                                       // the caller's arrays, byte for byte
    std::vector<rt3light::Face> face; std::vector<float> cr;
    std::vector<uint32_t> q; std::vector<uint64_t> cdf; uint64_t total = 0;
    bool valid = false;
    static void append(std::vector<uint8_t>& k, const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; k.insert(k.end(), b, b + n); }
    static std::vector<uint8_t> key_of(const rt3_gface* faces, uint32_t nf, const float* verts, uint32_t nv, const rt3_material* fm, const float* sph,
                                       const rt3_material* sm, uint32_t ns) {
        std::vector<uint8_t> k;
        append(k, &nf, 4); append(k, &nv, 4); append(k, &ns, 4);
        if (nf) { append(k, faces, (size_t)nf * sizeof(rt3_gface)); append(k, fm, (size_t)nf * sizeof(rt3_material)); }
        if (nv) append(k, verts, (size_t)nv * 16u);
        if (ns) { append(k, sph, (size_t)ns * 16u); append(k, sm, (size_t)ns * sizeof(rt3_material)); }
        return k;
    }
    void build(const rt3_gface* faces, uint32_t nf, const float* verts, const rt3_material* fm, const float* sph, const rt3_material* sm, uint32_t ns) {
        const uint32_t n = nf + ns;
        face.resize(nf); cr.assign(sph, sph + (size_t)4 * ns);
        std::vector<float> w(n);
        float w_max = 0.0f;
        for (uint32_t i = 0; i < nf; i++) {
            rt3light::face_of(verts + 4 * (size_t)faces[i].v1, verts + 4 * (size_t)faces[i].v2, verts + 4 * (size_t)faces[i].v3, face[i]);
            w[i] = rt3light::weight(rt3light::brightness(fm[i].kind, fm[i].rgb[0], fm[i].rgb[1], fm[i].rgb[2]), rt3light::face_area(face[i]));
        }
        for (uint32_t i = 0; i < ns; i++)
            w[nf + i] = rt3light::weight(rt3light::brightness(sm[i].kind, sm[i].rgb[0], sm[i].rgb[1], sm[i].rgb[2]), rt3light::sphere_area(sph[4 * (size_t)i + 3]));
        for (uint32_t k = 0; k < n; k++) if (w[k] > w_max) w_max = w[k];
        q.resize(n); cdf.resize(n);
        total = 0;
        for (uint32_t k = 0; k < n; k++) { q[k] = rt3light::quantise(w[k], w_max); total += q[k]; cdf[k] = total; }
        valid = true;
    }
};
}  // namespace
extern "C" int rt3_debug_light_sample(const rt3_gface* faces, uint32_t n_faces, const float* vertices, uint32_t n_vertices, const rt3_material* face_materials,
                                      const float* center_radius, const rt3_material* sphere_materials, uint32_t n_spheres, uint32_t base, uint32_t depth,
                                      uint32_t* light, float point[3], float light_normal[3], float* area, float* pl) {
    if (!light || !point || !light_normal || !area || !pl) return RT3_E_ARG;
    if ((n_faces && (!faces || !face_materials)) || (n_vertices && !vertices) || (n_spheres && (!center_radius || !sphere_materials))) return RT3_E_ARG;
    if ((uint64_t)n_faces + n_spheres > 0x7FFFFFFFull) return RT3_E_ARG;
    for (uint32_t i = 0; i < n_faces; i++)
        if (faces[i].v1 >= n_vertices || faces[i].v2 >= n_vertices || faces[i].v3 >= n_vertices) return RT3_E_ARG;
    static thread_local HostLightTable T;
    std::vector<uint8_t> key = HostLightTable::key_of(faces, n_faces, vertices, n_vertices, face_materials, center_radius, sphere_materials, n_spheres);
    if (!T.valid || T.key != key) {
        T.build(faces, n_faces, vertices, face_materials, center_radius, sphere_materials, n_spheres);
        T.key = std::move(key);
    }
    *light = rt3light::kNoLight; *area = 0.0f; *pl = 0.0f;
    for (int a = 0; a < 3; a++) point[a] = light_normal[a] = 0.0f;
    if (T.total == 0) return 0;
    float ua, ub;
    const uint32_t li = rt3light::pick(T.cdf.data(), n_faces + n_spheres, T.total, base, depth, ua, ub);
    rt3light::Point Y;
    if (li < n_faces) rt3light::point_on_face(T.face[li], ua, ub, Y);
    else { const float* s = T.cr.data() + 4 * (size_t)(li - n_faces); rt3light::point_on_sphere(s[0], s[1], s[2], s[3], ua, ub, Y); }
    *light = li; point[0] = Y.x; point[1] = Y.y; point[2] = Y.z; light_normal[0] = Y.nx; light_normal[1] = Y.ny; light_normal[2] = Y.nz;
    *area = Y.area; *pl = (float)T.q[li] / (float)T.total;
    return 0;
}

// The display transform's law (rt3.h "Display transform") on the host: the functions of rt3_display_law.hpp the kernels call, one pixel or
// one histogram per call.  A refused call writes nothing.
extern "C" int rt3_debug_display_bin(const float rgb[3], uint32_t* bin) {
    if (!rgb || !bin) return RT3_E_ARG;
    *bin = rt3disp::bin(rgb[0], rgb[1], rgb[2]);
    return 0;
}
extern "C" int rt3_debug_display_gain(const uint32_t hist[512], const rt3_display_params* p, float* gain) {
    if (!hist || !p || !gain || rt3disp::refusal(*p)) return RT3_E_ARG;
    *gain = rt3disp::gain_of(hist, p->trim_low, p->trim_high, p->exposure, p->key);
    return 0;
}
extern "C" int rt3_debug_display_pixel(const float rgb[3], float gain, const rt3_display_params* p, uint32_t* word) {
    if (!rgb || !p || !word || rt3disp::refusal(*p)) return RT3_E_ARG;
    *word = rt3disp::pixel(rgb[0], rgb[1], rgb[2], gain, p->curve, p->transfer, p->white, rt3disp::kSrgbTable);
    return 0;
}
extern "C" int rt3_debug_display_srgb_table(uint8_t out[4096]) {
    if (!out) return RT3_E_ARG;
    std::memcpy(out, rt3disp::kSrgbTable, sizeof rt3disp::kSrgbTable);
    return 0;
}

// The law of display sequences (rt3.h "Display sequences") on the host: the functions of rt3_display_sequence_law.hpp the kernels call,
// one histogram or one frame per call, serially.  A refused call writes nothing.
extern "C" int rt3_debug_exposure_step(const rt3_exposure* prev, const uint32_t hist[512], const rt3_display_sequence_params* p, rt3_exposure* out) {
    if (!hist || !p || !out || rt3dseq::refusal(*p)) return RT3_E_ARG;
    const rt3_display_params& d = p->display;
    if (!(d.flags & RT3_DISPLAY_AUTO_EXPOSURE)) {
        if (prev) return RT3_E_ARG;
        *out = rt3_exposure{ 0u, 0u, d.exposure, 0u };
        return 0;
    }
    if (prev && prev->level > rt3dseq::kMaxLevel) return RT3_E_ARG;
    uint64_t n = 0;
    const uint32_t target = rt3dseq::target_of(hist, d.trim_low, d.trim_high, &n);
    *out = rt3dseq::exposure_next(prev ? prev->level : 0u, prev ? prev->frames : 0u, n, target, p->adapt_brighter, p->adapt_darker, d.exposure, d.key);
    return 0;
}
extern "C" int rt3_debug_bloom(uint32_t w, uint32_t h, const float* rgba, float gain, float threshold, uint32_t levels, float* out_u1, float* out_bloom) {
    using namespace rt3dseq;
    if (!rgba || w == 0 || h == 0 || (uint64_t)w * h > (1ull << 26) || levels < 1 || levels > kMaxBloomLevels) return RT3_E_ARG;
    if (!(threshold >= 0.0f) || !(threshold <= kFltMax)) return RT3_E_ARG;
    const auto store = [](std::vector<float>& plane, size_t t, const Rgb& c) { plane[4 * t] = c.r; plane[4 * t + 1] = c.g; plane[4 * t + 2] = c.b; plane[4 * t + 3] = 0.0f; };
    std::vector<std::vector<float>> d(levels + 1);                  // d[l]: D_l, then U_l; d[0]: b0
    std::vector<uint32_t> pw(levels + 1), ph(levels + 1);
    pw[0] = w; ph[0] = h;
    d[0].resize(4 * (size_t)w * h);
    for (size_t t = 0; t < (size_t)w * h; t++) store(d[0], t, bright(exposed(rgba[4 * t], rgba[4 * t + 1], rgba[4 * t + 2], gain), threshold));
    for (uint32_t l = 1; l <= levels; l++) {
        pw[l] = half_of(pw[l - 1]); ph[l] = half_of(ph[l - 1]);
        d[l].resize(4 * (size_t)pw[l] * ph[l]);
        const Plane s{ d[l - 1].data(), pw[l - 1], ph[l - 1] };
        for (uint32_t j = 0; j < ph[l]; j++)
            for (uint32_t i = 0; i < pw[l]; i++) store(d[l], (size_t)j * pw[l] + i, down_texel(s, i, j));
    }
    for (uint32_t l = levels - 1; l >= 1; l--) {
        const Plane u{ d[l + 1].data(), pw[l + 1], ph[l + 1] }, own{ d[l].data(), pw[l], ph[l] };
        for (uint32_t j = 0; j < ph[l]; j++)
            for (uint32_t i = 0; i < pw[l]; i++) store(d[l], (size_t)j * pw[l] + i, sum(texel(own, i, j), up_texel(u, i, j)));
    }
    if (out_u1) std::memcpy(out_u1, d[1].data(), d[1].size() * sizeof(float));
    if (out_bloom) {
        const Plane u1{ d[1].data(), pw[1], ph[1] };
        const float weight = level_weight(levels);
        for (uint32_t j = 0; j < h; j++)
            for (uint32_t i = 0; i < w; i++) {
                const Rgb b = bloom_texel(u1, i, j, weight);
                float* o = out_bloom + 4 * ((size_t)j * w + i);
                o[0] = b.r; o[1] = b.g; o[2] = b.b; o[3] = 0.0f;
            }
    }
    return 0;
}

extern "C" uint32_t rt3_debug_sphere_plan(const float* center_radius, uint32_t n, float centre[3], uint32_t direct[4]) {
    if (!centre || !direct || (n != 0 && !center_radius)) return 0;
    for (int k = 0; k < 4; k++) direct[k] = 0xFFFFFFFFu;
    sphere_filter_centre(center_radius, n, centre);
    return sphere_direct_list(center_radius, n, centre, direct);
}

// The lens models' law (rt3.h "Lens models") on the host: the statement of rt3_lens_law.hpp k_lens_rays evaluates, one ray per call,
// and the frame a lens looks through.  A refused call writes nothing.
extern "C" int rt3_debug_lens_ray(const rt3_lens* lens, const rt3_params* p, uint32_t x, uint32_t y, uint32_t s, rt3_ray* out) {
    if (!lens || !p || !out || p->width == 0 || p->height == 0 || p->spp == 0 || x >= p->width || y >= p->height || s >= p->spp) return RT3_E_ARG;
    if (rt3lens::refusal(lens, p->width, p->height)) return RT3_E_ARG;
    const rt3lens::Frame f{ p->width, p->height, p->spp, p->seed, rt3lens::edge_of(p->spp) };
    rt3lens::ray_of(*lens, f, x, y, s, out->origin, out->direction);
    out->t_max = __builtin_inff();
    out->_pad = 0u;
    return 0;
}
// One hit of the specular-chain law (rt3.h "Specular-chain AOVs") on the host: the statement of rt3_aov_chain_law.hpp k_aov_bounce evaluates.
extern "C" int rt3_debug_aov_bounce(const float d[3], const float p[3], const float n[3], uint32_t mat_kind, const float mat[4], const float T[3],
                                    uint32_t bounces_used, const rt3_aov_chain_params* chain, float out_rgb[3], float out_normal[3],
                                    float out_direction[3], uint32_t* follow) {
    if (!d || !p || !n || !mat || !T || !out_rgb || !out_normal || !out_direction || !follow || rt3chain::refusal(chain)) return RT3_E_ARG;
    const rt3chain::Step S = rt3chain::step(d[0], d[1], d[2], p[0], p[1], p[2], n[0], n[1], n[2], mat_kind, mat[0], mat[1], mat[2], mat[3],
                                            T[0], T[1], T[2], bounces_used, chain->max_bounces, chain->max_fuzz);
    out_rgb[0] = S.ax; out_rgb[1] = S.ay; out_rgb[2] = S.az;
    out_normal[0] = S.nx; out_normal[1] = S.ny; out_normal[2] = S.nz;
    out_direction[0] = S.dx; out_direction[1] = S.dy; out_direction[2] = S.dz;
    *follow = S.follow;
    return 0;
}
// The inverse law (rt3.h "Lens sequences") on the host: the statements of rt3_lens_law.hpp k_temporal_reproject evaluates.
extern "C" float rt3_debug_turns(float c, float s) { return rt3lens::turns(c, s); }

// The image texture law in C (rt3.h "Image textures"; rt3_texture_law.hpp is the one statement, the device's too).
extern "C" int rt3_debug_texture_lookup(const float* rgba, uint32_t w, uint32_t h, uint32_t wrap, const float uv[2], float out_rgb[3]) {
    if (!rgba || !uv || !out_rgb || w == 0 || h == 0 || w > RT3_TEX_MAX_SIDE || h > RT3_TEX_MAX_SIDE || (uint64_t)w * h > (1ull << 26)) return RT3_E_ARG;
    if (wrap != RT3_TEX_REPEAT && wrap != RT3_TEX_CLAMP) return RT3_E_ARG;
    struct Texel { float x, y, z, w; };
    rt3tex::lookup(reinterpret_cast<const Texel*>(rgba), w, h, wrap, uv[0], uv[1], out_rgb[0], out_rgb[1], out_rgb[2]);
    return 0;
}
extern "C" int rt3_debug_texture_sphere_uv(const float n[3], float uv[2]) {
    if (!n || !uv) return RT3_E_ARG;
    rt3tex::sphere_uv(n[0], n[1], n[2], uv[0], uv[1]);
    return 0;
}
extern "C" int rt3_debug_texture_face_uv(const float p1[3], const float p2[3], const float p3[3], const float uv6[6], const float p[3], float uv[2]) {
    if (!p1 || !p2 || !p3 || !uv6 || !p || !uv) return RT3_E_ARG;
    rt3tex::face_uv(p1, p2, p3, uv6, p, uv[0], uv[1]);
    return 0;
}
extern "C" int rt3_debug_optic_pixel(const rt3_lens* prev_lens, uint32_t width, uint32_t height, const float r[3], uint32_t is_hit,
                                     float out_xy_depth[3], uint32_t* face, uint32_t* valid) {
    if (!prev_lens || !r || !out_xy_depth || !face || !valid || width < 2 || height < 2) return RT3_E_ARG;
    if (rt3lens::refusal(prev_lens, width, height)) return RT3_E_ARG;
    float xp = __builtin_nanf(""), yp = __builtin_nanf(""), zhat = 0.0f;      // (the pole behind a fisheye leaves x', y' as they are)
    uint32_t f = 0;
    const bool ok = rt3lens::project_of(*prev_lens, width, height, r, xp, yp, zhat, f);
    if (prev_lens->model == RT3_LENS_ORTHO && !is_hit) {            // not projected: the pixel keeps its own position
        out_xy_depth[0] = out_xy_depth[1] = __builtin_nanf("");
        out_xy_depth[2] = zhat;
        *face = 0;
        *valid = 1;
        return 0;
    }
    out_xy_depth[0] = xp; out_xy_depth[1] = yp; out_xy_depth[2] = zhat;
    *face = f;
    *valid = ok ? 1u : 0u;
    return 0;
}
// Worked out in double and rounded once per component: each axis is then a unit vector to a few 2^-25, far inside the 2^-20 the entry points ask for.
extern "C" void rt3_lens_look_at(rt3_lens* lens, uint32_t model, const float from[3], const float at[3], const float vup[3]) {
    if (!lens || !from || !at || !vup) return;
    double f[3], r[3], u[3];
    for (int c = 0; c < 3; c++) f[c] = (double)at[c] - (double)from[c];
    const double lf = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (int c = 0; c < 3; c++) f[c] /= lf;
    r[0] = f[1] * vup[2] - f[2] * vup[1]; r[1] = f[2] * vup[0] - f[0] * vup[2]; r[2] = f[0] * vup[1] - f[1] * vup[0];
    const double lr = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int c = 0; c < 3; c++) r[c] /= lr;
    u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
    lens->model = model;
    for (int c = 0; c < 3; c++) { lens->origin[c] = from[c]; lens->right[c] = (float)r[c]; lens->up[c] = (float)u[c]; lens->forward[c] = (float)f[c]; }
    lens->_pad0 = lens->_pad1 = lens->_pad2 = lens->_pad3 = 0.0f;
}
