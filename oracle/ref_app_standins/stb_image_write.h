/* Stand-in for stb_image_write.h (application build, see intrin.h beside this file).  Our
 * own text.  <stdlib.h> and <math.h> exactly as ref_standins/stb_image_write.h keeps them:
 * overload resolution in the reference depends on them.  stbi_write_bmp, the one function
 * io::SaveImage names, encodes no BMP: where SPT_REF_DUMP is set it writes the w*h*comp
 * bytes it was handed, raw, to $SPT_REF_DUMP.<k> (k = 1, 2, ...: the call's ordinal, so a
 * process that saves several frames leaves several files), and its own arguments to
 * $SPT_REF_DUMP.<k>.args as four lines (file name, w, h, comp); then it counts the call,
 * which is what the glfwWindowShouldClose stand-in waits for.  It only reads the frame. */
#pragma once
#include <stdlib.h>
#include <math.h>

inline int stbi_write_bmp(char const *filename, int w, int h, int comp, const void *data)
{
    static std::mutex mu;
    static int calls = 0;
    std::lock_guard<std::mutex> lock(mu);
    const int k = ++calls;
    int ok = 1;
    if (const char *base = getenv("SPT_REF_DUMP")) {
        const std::string path = std::string(base) + "." + std::to_string(k);
        const size_t bytes = (size_t)w * (size_t)h * (size_t)comp;
        FILE *f = fopen(path.c_str(), "wb");
        ok = f && fwrite(data, 1, bytes, f) == bytes;
        if (f && fclose(f) != 0) ok = 0;
        FILE *a = fopen((path + ".args").c_str(), "w");
        ok = a && fprintf(a, "%s\n%d\n%d\n%d\n", filename, w, h, comp) > 0 && ok;
        if (a && fclose(a) != 0) ok = 0;
        if (!ok) fprintf(stderr, "spt_ref_app: could not write %s\n", path.c_str());
    }
    spt_ref_app::saved.fetch_add(1);
    return ok;
}
