/*
 * spt_oracle.h -- CPU restatement of SimplePathTracer's per-pixel render loop.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path (simplepathtracer_amd/,
 * include/spt_hip.h) includes, links or calls this code.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it, as the
 * checker / CPU timing baseline.
 *
 * PARITY STATUS: the reference (header-only MSVC C++) is built headless behind
 * stand-ins of our own for the headers it lacks (oracle/ref_standins/: <intrin.h>,
 * glbinding/GLFW via Gl.hpp, stb via IOHelpers.hpp) by `make ref`, into oracle/_ref/.
 * tests/test_reference_parity.py compares this file with the reference's own functions
 * bit for bit: uniform draws from a seeded thread, both scene generators, the camera
 * basis, FindClosestIntersectionSphere and the contact functions, TraceAndSampleColor
 * paths (spo_trace_ray) on the golden and the degenerate scenes, RenderSegment and
 * RenderSegmentTask tiles with g_data (the spo_render_segment*_stream functions, which
 * share every line with the keyed ones).  NOT pinned: the keyed-stream design below (the
 * reference can only start a stream at seed << 31 | seed), Renderer.hpp's tiling (needs
 * GL), MSVC's own code generation and C runtime, more than 255 spheres (the reference
 * does not terminate), sky colours other than the reference's constant.
 * Pinned piecewise besides (tests/test_oracle_kat.py, oracle/kat_*.c*):
 *   - uniform draws vs the real libstdc++ std::uniform_real_distribution<float>
 *     driven by the reference's splitmix mixer (Random.hpp:30-36, 86-93);
 *   - Vec4 arithmetic (Dot/LengthSquared/Normalize/Reflect/Mat4*Vec4) vs the real
 *     SSE4.1 intrinsics the reference uses (Math.hpp:107-187);
 *   - glibc pow/sqrt in double precision as used by SampleColorRefractive.
 * Semantics follow SURVEY.md §8(a): fp32 everywhere, no FMA contraction, IEEE
 * division and sqrt, libstdc++/glibc double promotion of pow()/sqrt() in the
 * refraction branch.  Build with -ffp-contract=off and without -ffast-math.
 *
 * RNG seam (SURVEY.md §8c seam (b)): the reference draws from a time-seeded
 * thread_local splitmix (Random.hpp:86-93).  Here every (pixel, sample) owns a
 * keyed splitmix stream: state0 = fmix64(fmix64(seed) ^ (pixel << 32 | sample)),
 * pixel = y * width + x.  Draw n mixes state0 + (n+1)*0x9E3779B97F4A7C15 with the
 * reference mixer, so results are independent of tiling and thread scheduling.
 */
#ifndef SPT_ORACLE_H
#define SPT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Material enum, Definitions.hpp:7-13 */
enum { SPO_SKYBOX = 0, SPO_REFLECTIVE = 1, SPO_REFRACTIVE = 2, SPO_DIFFUSE = 3 };

/* Paths with more specular events than this are cut (color 0).  The reference
 * recurses without bound (SingleThreadPathTracer.hpp:45,63-91) and would overflow
 * its stack long before; the GPU path uses the same cap. */
#define SPO_SPECULAR_CAP 1024u
/* RenderSegmentTask's pass cap, TaskBasedPathTracer.hpp:81 (pass < 10). */
#define SPO_TASK_PASSES 10u

/* What a path went through, counted by spo_trace_ray: sphere hits by material (a glass hit
 * counts once per Schlick reflection, once if it refracts in and out, once per total
 * internal reflection), how the path ended (the diffuse walk ran out of bounces; a ray
 * left for the sky and took its colour) and whether SPO_SPECULAR_CAP cut it. */
enum {
    SPO_EV_DIFFUSE = 0, SPO_EV_MIRROR, SPO_EV_GLASS_REFLECT, SPO_EV_REFRACT_TWICE, SPO_EV_TIR,
    SPO_EV_END_BOUNCES, SPO_EV_END_SKY, SPO_EV_CUT, SPO_EV_COUNT
};
#define SPO_TRACE_INFO (2u + SPO_EV_COUNT)

/* Scene SoA, Globals.hpp:31-37 (g_spheres, g_radii, g_colors, g_materials,
 * g_diffuses, g_sphereNumber).  centers/colors are float4 per sphere; the w lane
 * is treated as 0 as in the reference's Vec4{x,y,z} initialisers. */
typedef struct spo_scene {
    uint32_t n;
    const float *centers;
    const float *radii;
    const float *colors;
    const uint8_t *materials;
    const float *fuzz;
} spo_scene;

/* Camera + compile-time config, Globals.hpp:8-29. view is viewMatrix (row-major,
 * already transposed as in Renderer.hpp:321). */
typedef struct spo_frame {
    float view[16];
    float eye[4];
    float sky[4];
    uint32_t width, height, spp, bounces;
    uint64_t seed;
} spo_frame;

/* ---- RNG (Random.hpp) ---- */
uint32_t spo_next_u32(uint64_t *state);
float spo_uniform(uint64_t *state, float a, float b);
float spo_uniform_u32(uint32_t bits, float a, float b);
uint64_t spo_sample_key(uint64_t seed, uint32_t pixel, uint32_t sample);
uint64_t spo_scene_state(uint32_t seed);
void spo_ball_vector(uint64_t *state, float out[4]);
void spo_unit_vector(uint64_t *state, float out[4]);

/* ---- math / geometry (Math.hpp, Collision.hpp) ---- */
float spo_dot(const float a[4], const float b[4]);
float spo_length_squared(const float a[4]);
void spo_normalize(const float a[4], float out[4]);
void spo_reflect(const float v[4], const float n[4], float out[4]);
void spo_matvec(const float m[16], const float v[4], float out[4]);
void spo_camera_basis(const float eye[4], const float look_at[4], const float up[4], float view_out[16]);
uint32_t spo_find_closest(const spo_scene *sc, const float d[4], const float o[4]);
void spo_write_pixel(const float c[4], uint8_t out[3]);
/* Sphere i alone on the ray (o, d), as find_closest sees it: returns whether
 * RaySphereIntersection passes; out[0] = the squared distance compared with min_d,
 * out[1] = 1 if the contact lies ahead of the origin (Collision.hpp:98). */
int spo_probe_sphere(const spo_scene *sc, uint32_t i, const float d[4], const float o[4], float out[2]);

/* ---- render loop (SingleThreadPathTracer.hpp, TaskBasedPathTracer.hpp) ---- */
/* One (pixel, sample) path of RenderSegment: out[0..3] = color, returns number
 * of FindClosest calls.  task_mode: apply RenderSegmentTask's pass cap; out[3]
 * becomes 1.0 if the sample is counted, 0.0 if dropped. */
/* Direction of a primary ray of pixel (x, y) (SingleThreadPathTracer.hpp:125-128); the two
 * jitter draws come from *state. */
void spo_primary_ray(const spo_frame *fr, uint32_t x, uint32_t y, uint64_t *state, float d[4]);
void spo_primary_winners(const spo_scene *sc, const spo_frame *fr, const uint32_t *xys, uint32_t n, uint32_t *winner);
uint32_t spo_trace_sample(const spo_scene *sc, const spo_frame *fr, uint32_t x, uint32_t y,
                          uint32_t s, int task_mode, float out[4]);
/* spo_trace_sample, and info[0] = the path's specular events (the one that meets
 * SPO_SPECULAR_CAP or the pass cap included), info[1] = 1 if task mode dropped it. */
uint32_t spo_trace_sample_info(const spo_scene *sc, const spo_frame *fr, uint32_t x, uint32_t y,
                               uint32_t s, int task_mode, float out[4], uint32_t info[2]);
/* TraceAndSampleColor(d, o, bounces) drawing from the caller's raw stream *state (advanced
 * past the path's draws); the code of every keyed path above.  fr supplies the sky colour
 * only.  out = the colour's four lanes; info[0] = specular events, info[1] = 1 if the path
 * was cut at SPO_SPECULAR_CAP (the reference would recurse on), info[2 + e] = count of
 * SPO_EV_e.  Returns the number of FindClosest calls. */
uint32_t spo_trace_ray(const spo_scene *sc, const spo_frame *fr, const float d[4], const float o[4],
                       uint32_t bounces, uint64_t *state, float out[4], uint32_t info[SPO_TRACE_INFO]);
/* Record the base 1 - c of every Schlick powf(1 - c, 5) traced by the calling thread
 * into buf (NULL stops); returns the count since the previous call (may exceed cap). */
uint32_t spo_schlick_log(float *buf, uint32_t cap);
/* RenderSegment over [yB,yE)x[xB,xE).  rgba: region-local float4 per pixel
 * (row-major), rgb8: full-frame g_data in the reference index layout.  Either may
 * be NULL. Returns total FindClosest calls. */
uint64_t spo_render_segment(const spo_scene *sc, const spo_frame *fr, uint32_t yB, uint32_t yE,
                            uint32_t xB, uint32_t xE, float *rgba, uint8_t *rgb8);
/* RenderSegmentTask, faithful breadth-first restatement including its material
 * queues, its 10-pass cap and its colorIndex stride (correct for square tiles). */
uint64_t spo_render_segment_task(const spo_scene *sc, const spo_frame *fr, uint32_t yB, uint32_t yE,
                                 uint32_t xB, uint32_t xE, float *rgba, uint8_t *rgb8);
/* spo_render_segment / spo_render_segment_task with one sequential stream *state running
 * through every pixel, sample and path in the reference's order, where the keyed
 * functions give each (pixel, sample) its own: the same code, only the uint64_t * differs.
 * This is what the reference computes on one thread whose generator starts at *state
 * (tests/test_reference_parity.py).  dropped (may be NULL) is increased by the number of
 * samples the 10-pass cap leaves unresolved. */
uint64_t spo_render_segment_stream(const spo_scene *sc, const spo_frame *fr, uint32_t yB, uint32_t yE,
                                   uint32_t xB, uint32_t xE, uint64_t *state, float *rgba, uint8_t *rgb8);
uint64_t spo_render_segment_task_stream(const spo_scene *sc, const spo_frame *fr, uint32_t yB, uint32_t yE,
                                        uint32_t xB, uint32_t xE, uint64_t *state, float *rgba, uint8_t *rgb8,
                                        uint64_t *dropped);
/* RenderImageParallelMain tiling (Renderer.hpp:257-302) with thread_count tiles
 * per side and at most thread_count tiles in flight.  mode 0 = RenderSegment,
 * 1 = RenderSegmentTask.  rgba is a full-frame float4 buffer (may be NULL). */
int spo_render_image_parallel(const spo_scene *sc, const spo_frame *fr, uint32_t thread_count,
                              int mode, float *rgba, uint8_t *rgb8);

/* ---- scene generators (SceneGenerators.hpp), sequential splitmix(seed) ---- */
uint32_t spo_generate_spheres(uint32_t seed, uint32_t cap, float *centers, float *radii,
                              float *colors, uint8_t *materials, float *fuzz);
uint32_t spo_init_spheres(uint32_t seed, float *centers, float *radii, float *colors,
                          uint8_t *materials, float *fuzz);

/* The scalar primitives over consecutive uint32 input patterns [first, first + count),
 * count <= 2^32, by their literal definitions: sqrtf, glibc's powf(x, 5.f),
 * spo_uniform_u32 on the three ranges in use, the refraction scalar of
 * sample_refractive for air->glass and glass->air (-1e30f where no_tir fails),
 * spo_write_pixel's byte and the x86 float -> uint8_t conversion.  The op codes are those
 * of tests/cpp/spt_mathsweep.hip (SQRT_POS and SQRT_RAW are device forms only).
 * spo_math_block writes the result bits (any NaN as 0x7FC00000, a byte zero-extended);
 * spo_math_digest one wrapping 64-bit sum of fmix64(u << 32 | bits) per block of 2^20
 * patterns.  Threaded with OpenMP (OMP_NUM_THREADS).  Return 0, or 1 on a bad argument. */
enum {
    SPO_MATH_SQRT = 0,
    SPO_MATH_SQRT_POS = 1,
    SPO_MATH_SQRT_RAW = 2,
    SPO_MATH_POW5 = 3,
    SPO_MATH_UNI_M1_1 = 4,
    SPO_MATH_UNI_H = 5,
    SPO_MATH_UNI_0_1 = 6,
    SPO_MATH_REFR_AG = 7,
    SPO_MATH_REFR_GA = 8,
    SPO_MATH_GAMMA = 9,
    SPO_MATH_F2U8 = 10
};
#define SPO_MATH_BLOCK ((uint64_t)1 << 20)
int spo_math_block(int op, uint32_t first, uint64_t count, uint32_t *out);
int spo_math_digest(int op, uint32_t first, uint64_t count, uint64_t *digest);

#ifdef __cplusplus
}
#endif
#endif
