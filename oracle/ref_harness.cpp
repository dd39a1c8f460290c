// ref_harness -- runs the reference's own functions, for tests/test_reference_parity.py.
//
// TEST INFRASTRUCTURE ONLY, our own text.  It includes the reference's headers from the
// directory given with -I (never copied into this tree) in the order of the reference's
// Renderer.hpp:3-8, behind the stand-ins of oracle/ref_standins/, and calls the
// reference's functions by name.  Built by `make -C oracle ref` into oracle/_ref/.
//
//     ref_harness REQUEST RESPONSE
//
// REQUEST and RESPONSE are files of flat little-endian records (u32, i32, f32, u8); the
// first u32 of a request is the operation.  A scene is: u32 n, n x 4 f32 centres, n f32
// radii, n x 4 f32 colours, n u8 materials, n f32 g_diffuses; the w lanes of centres and
// colours are written as 0, as the reference's Vec4{x, y, z} initialisers leave them.
//
//   1 draws     u32 seed, f32 a, f32 b, u32 count           -> count f32
//   2 generate  u32 which (0 GenerateSpheres, 1 InitSpheres), u32 seed -> a scene
//   3 camera    3 f32 eye, look-at, up each                 -> 16 f32: Transpose(CreateCameraBasisMatrix)
//   4 geometry  scene, u32 rays, rays x 4 f32 o, rays x 4 f32 d, rays i32 aim
//               -> rays u32 FindClosestIntersectionSphere; rays x 10 f32: ClosestContactPoint
//                  (4), its factor t, ContactNormal (4), LengthSquared(o - P) of the sphere
//                  found (zeros on a miss); rays u8 RaySphereIntersection of sphere aim (0 if aim < 0)
//   5 trace     scene, u32 paths, per path 4 f32 d, 4 f32 o, u32 bounces, u32 seed
//               -> paths x 4 f32 TraceAndSampleColor
//   6 segment   scene, 16 f32 viewMatrix, 4 f32 eyePos, u32 mode (0 RenderSegment,
//               1 RenderSegmentTask), u32 seed, u32 yBegin, yEnd, xBegin, xEnd
//               -> u32 count, count x (u32 index, 4 f32 colour) as handed to WritePixel,
//                  in call order; g_size u8 g_data (zeroed before the call)
//
// Every operation that draws runs on a fresh std::thread after the clock of the stand-in
// <intrin.h> is set to the seed: the reference's thread_local splitmix is then
// constructed from static_cast<unsigned int>(seed), i.e. starts at seed << 31 | seed.
//
// Exit status 0, or 2 with a message: a malformed request, or n > 255 (the uint8_t index
// of FindClosestIntersectionSphere, Collision.hpp:92, never reaches such an n: the
// reference does not terminate there).
#include <Math.hpp>
#include <IOHelpers.hpp>
#include <Globals.hpp>

// io::WritePixel's arguments, recorded at the tracers' call sites: the calls are rewritten
// to pass the index through ref_tap(), which notes it with the colour.  WritePixel itself
// (IOHelpers.hpp, already included) is untouched and still writes g_data.
struct RefTap { uint32_t index; float color[4]; };
static std::vector<RefTap> g_taps;
static inline uint32_t ref_tap(uint32_t index, math::Vec4 color)
{
    g_taps.push_back({index, {color.xyzw[0], color.xyzw[1], color.xyzw[2], color.xyzw[3]}});
    return index;
}
#define WritePixel(index, color) WritePixel(ref_tap((index), (color)), (color))
#include <SingleThreadPathTracer.hpp>
#include <TaskBasedPathTracer.hpp>
#undef WritePixel
#include <SceneGenerators.hpp>

namespace {

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    void need(size_t n)
    {
        if (buf.size() - at < n) {
            std::fprintf(stderr, "ref_harness: request too short\n");
            std::exit(2);
        }
    }
    void raw(void *dst, size_t n) { need(n); std::memcpy(dst, buf.data() + at, n); at += n; }
    uint32_t u32() { uint32_t v; raw(&v, 4); return v; }
    int32_t i32() { int32_t v; raw(&v, 4); return v; }
    float f32() { float v; raw(&v, 4); return v; }
    math::Vec4 vec3w0() { float v[4]; raw(v, 16); return math::Vec4{v[0], v[1], v[2], 0.f}; }
    math::Vec4 vec4() { float v[4]; raw(v, 16); return math::Vec4{v[0], v[1], v[2], v[3]}; }
};

struct Writer {
    std::vector<uint8_t> buf;
    void raw(const void *src, size_t n) { const uint8_t *p = (const uint8_t *)src; buf.insert(buf.end(), p, p + n); }
    void u32(uint32_t v) { raw(&v, 4); }
    void f32(float v) { raw(&v, 4); }
    void vec4(math::Vec4 v) { raw(v.xyzw, 16); }
};

void read_scene(Reader &in)
{
    uint32_t n = in.u32();
    if (n > 255) {
        std::fprintf(stderr, "ref_harness: n = %u > 255: FindClosestIntersectionSphere's uint8_t index never ends\n", n);
        std::exit(2);
    }
    g_spheres.clear(); g_radii.clear(); g_colors.clear(); g_materials.clear(); g_diffuses.clear();
    for (uint32_t i = 0; i < n; ++i) g_spheres.push_back(in.vec3w0());
    for (uint32_t i = 0; i < n; ++i) g_radii.push_back(in.f32());
    for (uint32_t i = 0; i < n; ++i) g_colors.push_back(in.vec3w0());
    for (uint32_t i = 0; i < n; ++i) { uint8_t m; in.raw(&m, 1); g_materials.push_back(static_cast<Material>(m)); }
    for (uint32_t i = 0; i < n; ++i) g_diffuses.push_back(in.f32());
    g_sphereNumber = n;
}

void write_scene(Writer &out)
{
    uint32_t n = g_sphereNumber;
    out.u32(n);
    // a generator that left the arrays at different lengths would be a finding: say so
    if (g_spheres.size() != n || g_radii.size() != n || g_colors.size() != n || g_materials.size() != n ||
        g_diffuses.size() != n) {
        std::fprintf(stderr, "ref_harness: scene arrays of different lengths\n");
        std::exit(2);
    }
    for (uint32_t i = 0; i < n; ++i) out.vec4(g_spheres[i]);
    for (uint32_t i = 0; i < n; ++i) out.f32(g_radii[i]);
    for (uint32_t i = 0; i < n; ++i) out.vec4(g_colors[i]);
    for (uint32_t i = 0; i < n; ++i) { uint8_t m = static_cast<uint8_t>(g_materials[i]); out.raw(&m, 1); }
    for (uint32_t i = 0; i < n; ++i) out.f32(g_diffuses[i]);
}

// fn() on a fresh thread whose generator the reference will seed with `seed`
template <class F> void on_fresh_thread(uint32_t seed, F fn)
{
    spt_ref_clock_reading = static_cast<long long>(seed);
    std::thread t(fn);
    t.join();
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: ref_harness REQUEST RESPONSE\n");
        return 2;
    }
    Reader in;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) { std::perror(argv[1]); return 2; }
        uint8_t chunk[1 << 16];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) in.buf.insert(in.buf.end(), chunk, chunk + got);
        std::fclose(f);
    }
    Writer out;
    const uint32_t op = in.u32();
    switch (op) {
    case 1: {
        uint32_t seed = in.u32();
        float a = in.f32(), b = in.f32();
        uint32_t count = in.u32();
        on_fresh_thread(seed, [&] {
            for (uint32_t i = 0; i < count; ++i) out.f32(random::GenerateUniformRealDist(a, b));
        });
        break;
    }
    case 2: {
        uint32_t which = in.u32(), seed = in.u32();
        on_fresh_thread(seed, [&] {
            if (which == 0)
                GenerateSpheres();
            else
                InitSpheres();
        });
        write_scene(out);
        break;
    }
    case 3: {
        float v[9];
        in.raw(v, sizeof v);
        math::Vec4 eye{v[0], v[1], v[2]}, look{v[3], v[4], v[5]}, up{v[6], v[7], v[8]};
        math::Mat4 m = math::Transpose(math::CreateCameraBasisMatrix(eye, look, up));
        out.raw(m.array, sizeof m.array);
        break;
    }
    case 4: {
        read_scene(in);
        uint32_t rays = in.u32();
        std::vector<math::Vec4> o(rays), d(rays);
        std::vector<int32_t> aim(rays);
        for (auto &v : o) v = in.vec4();
        for (auto &v : d) v = in.vec4();
        for (auto &v : aim) v = in.i32();
        std::vector<uint32_t> idx(rays);
        for (uint32_t i = 0; i < rays; ++i) idx[i] = cd::FindClosestIntersectionSphere(d[i], o[i]);
        out.raw(idx.data(), 4 * idx.size());
        for (uint32_t i = 0; i < rays; ++i) {
            float rec[10] = {0};
            if (idx[i] < g_sphereNumber) {
                math::Vec4 c = g_spheres[idx[i]];
                float r = g_radii[idx[i]];
                math::Vec4 p = cd::CalculateRaySphereClosestContactPoint(c, r, o[i], d[i]);
                float t = cd::CalculateRaySphereMinIntersectionFactor(c - o[i], r, d[i]);
                math::Vec4 nrm = cd::CalculateRaySphereContactNormal(p, c);
                float ds = math::LengthSquared(o[i] - p);
                std::memcpy(rec, p.xyzw, 16);
                rec[4] = t;
                std::memcpy(rec + 5, nrm.xyzw, 16);
                rec[9] = ds;
            }
            out.raw(rec, sizeof rec);
        }
        for (uint32_t i = 0; i < rays; ++i) {
            uint8_t pass = 0;
            if (aim[i] >= 0) {
                if ((uint32_t)aim[i] >= g_sphereNumber) { std::fprintf(stderr, "ref_harness: aim out of range\n"); return 2; }
                pass = cd::RaySphereIntersection(g_spheres[aim[i]], g_radii[aim[i]], d[i], o[i]) ? 1 : 0;
            }
            out.raw(&pass, 1);
        }
        break;
    }
    case 5: {
        read_scene(in);
        uint32_t paths = in.u32();
        for (uint32_t i = 0; i < paths; ++i) {
            math::Vec4 d = in.vec4(), o = in.vec4();
            uint32_t bounces = in.u32(), seed = in.u32();
            on_fresh_thread(seed, [&] { out.vec4(TraceAndSampleColor(d, o, bounces)); });
        }
        break;
    }
    case 6: {
        read_scene(in);
        float view[16];
        in.raw(view, sizeof view);
        std::memcpy(viewMatrix.array, view, sizeof view);
        eyePos = in.vec4();
        uint32_t mode = in.u32(), seed = in.u32();
        RenderSegmentData seg;
        seg.yBegin = in.u32();
        seg.yEnd = in.u32();
        seg.xBegin = in.u32();
        seg.xEnd = in.u32();
        if (seg.yBegin > seg.yEnd || seg.xBegin > seg.xEnd || seg.yEnd > g_height || seg.xEnd > g_width) {
            std::fprintf(stderr, "ref_harness: segment outside the %u x %u frame\n", g_width, g_height);
            return 2;
        }
        // RenderSegmentTask's colorIndex strides rows by the segment's height
        // (TaskBasedPathTracer.hpp:103, 186): on a tile taller than wide it writes past the
        // end of its std::vector, which is undefined
        const uint64_t w = seg.xEnd - seg.xBegin, h = seg.yEnd - seg.yBegin;
        if (mode != 0 && w && h && (w - 1) + (h - 1) * h >= w * h) {
            std::fprintf(stderr, "ref_harness: RenderSegmentTask indexes past its colour array on a %llu x %llu tile\n",
                         (unsigned long long)w, (unsigned long long)h);
            return 2;
        }
        std::memset(g_data, 0, g_size);
        on_fresh_thread(seed, [&] {
            if (mode == 0)
                RenderSegment(seg);
            else
                RenderSegmentTask(seg);
        });
        out.u32(static_cast<uint32_t>(g_taps.size()));
        for (const RefTap &t : g_taps) { out.u32(t.index); out.raw(t.color, 16); }
        out.raw(g_data, g_size);
        break;
    }
    default:
        std::fprintf(stderr, "ref_harness: unknown operation %u\n", op);
        return 2;
    }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    size_t put = std::fwrite(out.buf.data(), 1, out.buf.size(), f);
    if (std::fclose(f) != 0 || put != out.buf.size()) { std::fprintf(stderr, "ref_harness: short write\n"); return 2; }
    return 0;
}
