// ref_dropin_driver -- the reference's Renderer.hpp against the drop-in shim, for what the
// reference's Main.cpp never reaches (tests/test_gpu_dropin_reference.py).
//
// TEST INFRASTRUCTURE ONLY, our own text.  It includes the reference's <Renderer.hpp> from
// the directory given with -I (never copied into this tree), behind the stand-ins of
// oracle/ref_app_standins/ and oracle/ref_standins/ and with include/dropin in front of the
// reference's include directory, exactly as _ref/ref_dropin_main (the reference's Main.cpp
// itself) is built, and calls the reference's functions by name.  Main.cpp's constexpr
// choices (Globals.hpp:8-9: TASK_MULTI_THREAD, REFERENCE) reach one scene and one calling
// pattern; the modes here reach the others.  Every frame is the reference's: 1440 x 1440,
// 100 spp, 10 bounces (constexpr too).  Built by `make -C oracle ref` into oracle/_ref/.
//
//     ref_dropin_driver image  <init|random>   RenderImage(): RenderSegmentTask over the
//                                              whole frame, then SaveImage
//     ref_dropin_driver frames <init|random>   RenderImageParallelMain() on this thread,
//                                              three times; before the third, eyePos moves
//                                              to {0.6, 1.3, -3} and viewMatrix is
//                                              recomputed with CreateCameraBasisMatrix
//     ref_dropin_driver pick REQUEST RESPONSE  GenerateSpheres(), one such frame, then
//                                              spt_shim::PickSphere per pixel and
//                                              spt_shim::FindClosestIntersectionSpheres
//                                              over the rays of the request
//
// Set-up as MainLoop's (Renderer.hpp:321-333): viewMatrix from eyePos, lookAt and upDir,
// then InitSpheres() or GenerateSpheres() on this thread, whose generator starts from
// SPT_REF_CLOCK_SEED.  g_data is filled with 0xAB before every frame: a byte no tile wrote
// keeps it.  Every SaveImage leaves a dump (SPT_REF_DUMP.<k>, see the stb stand-in).
//
// REQUEST is flat little-endian: u32 pixels, pixels x (u32 x, u32 y), u32 rays, rays x 4 f32
// origins, rays x 4 f32 directions.  RESPONSE: pixels u32, then rays u32.
//
// Exit status 0, or 2 with a message.
#include <Renderer.hpp>

namespace {

int usage()
{
    std::fprintf(stderr, "usage: ref_dropin_driver image|frames <init|random> | pick REQUEST RESPONSE\n");
    return 2;
}

bool set_up(const char *scene)
{
    spt_ref_app_seed_clock();
    viewMatrix = Transpose(math::CreateCameraBasisMatrix(eyePos, lookAt, upDir));
    if (std::strcmp(scene, "init") == 0)
        InitSpheres();
    else if (std::strcmp(scene, "random") == 0)
        GenerateSpheres();
    else
        return false;
    return true;
}

void frame()
{
    std::memset(g_data, 0xAB, g_size);
    RenderImageParallelMain();
}

bool read_all(const char *path, std::vector<uint8_t> &buf)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) return usage();
    const std::string mode = argv[1];
    if (mode == "image") {
        if (!set_up(argv[2])) return usage();
        std::memset(g_data, 0xAB, g_size);
        RenderImage();
        return 0;
    }
    if (mode == "frames") {
        if (!set_up(argv[2])) return usage();
        frame();
        frame();
        eyePos = {0.6f, 1.3f, -3.f};
        viewMatrix = Transpose(math::CreateCameraBasisMatrix(eyePos, lookAt, upDir));
        frame();
        return 0;
    }
    if (mode == "pick") {
        if (argc != 4) return usage();
        std::vector<uint8_t> req;
        if (!read_all(argv[2], req)) { std::perror(argv[2]); return 2; }
        size_t at = 0;
        auto u32 = [&](uint32_t &v) {
            if (req.size() - at < 4) return false;
            std::memcpy(&v, req.data() + at, 4);
            at += 4;
            return true;
        };
        uint32_t pixels = 0, rays = 0;
        if (!u32(pixels) || (req.size() - at) / 8 < pixels) { std::fprintf(stderr, "ref_dropin_driver: request too short\n"); return 2; }
        std::vector<uint32_t> xy(2 * (size_t)pixels);
        std::memcpy(xy.data(), req.data() + at, 8 * (size_t)pixels);
        at += 8 * (size_t)pixels;
        if (!u32(rays) || (req.size() - at) / 32 < rays) { std::fprintf(stderr, "ref_dropin_driver: request too short\n"); return 2; }
        std::vector<float> o(4 * (size_t)rays), d(4 * (size_t)rays);
        std::memcpy(o.data(), req.data() + at, 16 * (size_t)rays);
        std::memcpy(d.data(), req.data() + at + 16 * (size_t)rays, 16 * (size_t)rays);
        for (uint32_t i = 0; i < pixels; ++i)
            if (xy[2 * i] >= g_width || xy[2 * i + 1] >= g_height) {
                std::fprintf(stderr, "ref_dropin_driver: pixel outside the %u x %u frame\n", g_width, g_height);
                return 2;
            }
        set_up("random");
        frame();
        std::vector<uint32_t> out(pixels + (size_t)rays);
        for (uint32_t i = 0; i < pixels; ++i) out[i] = spt_shim::PickSphere(xy[2 * i], xy[2 * i + 1]);
        if (rays) spt_shim::FindClosestIntersectionSpheres(o.data(), d.data(), rays, out.data() + pixels);
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) { std::perror(argv[3]); return 2; }
        const size_t put = std::fwrite(out.data(), 4, out.size(), f);
        if (std::fclose(f) != 0 || put != out.size()) { std::fprintf(stderr, "ref_dropin_driver: short write\n"); return 2; }
        return 0;
    }
    return usage();
}
