/* Null stand-in for GLFW (application build, see ../intrin.h).  Our own text.  There is no
 * window: glfwCreateWindow hands out a static object, and glfwWindowShouldClose turns true
 * once io::SaveImage has run (the stb stand-in counts its calls), when the application asks
 * for it, or never returns once the deadline has passed.  glfwPollEvents sleeps a
 * millisecond, so that MainLoop does not spin a CPU while the frame renders.  glfwInit also
 * sets the reference's clock from the environment: it runs before MainLoop's first draw. */
#pragma once

struct GLFWwindow {
    int should_close;
};
typedef void (*GLFWkeyfun)(GLFWwindow *, int, int, int, int);
typedef void (*GLFWglproc)(void);

#define GLFW_RELEASE 0
#define GLFW_PRESS 1
#define GLFW_KEY_ESCAPE 256
#define GLFW_RESIZABLE 0x00020003
#define GLFW_CONTEXT_VERSION_MAJOR 0x00022002
#define GLFW_CONTEXT_VERSION_MINOR 0x00022003
#define GLFW_OPENGL_PROFILE 0x00022008
#define GLFW_OPENGL_CORE_PROFILE 0x00032001

inline int glfwInit()
{
    spt_ref_app_seed_clock();
    return 1;
}
inline void glfwTerminate() {}
inline void glfwWindowHint(int, int) {}
inline GLFWwindow *glfwCreateWindow(int, int, const char *, void *, void *)
{
    static GLFWwindow window = {0};
    return &window;
}
inline void glfwMakeContextCurrent(GLFWwindow *) {}
inline GLFWglproc glfwGetProcAddress(const char *) { return nullptr; }
inline GLFWkeyfun glfwSetKeyCallback(GLFWwindow *, GLFWkeyfun) { return nullptr; }
inline void glfwGetFramebufferSize(GLFWwindow *, int *width, int *height) { *width = *height = 0; }
inline void glfwSetWindowShouldClose(GLFWwindow *window, int value) { window->should_close = value; }
inline int glfwGetKey(GLFWwindow *, int) { return GLFW_RELEASE; }
inline int glfwWindowShouldClose(GLFWwindow *window)
{
    if (window->should_close || spt_ref_app::saved.load() > 0) return 1;
    spt_ref_app::check_deadline("MainLoop");
    return 0;
}
inline void glfwSwapBuffers(GLFWwindow *) {}
inline void glfwPollEvents() { spt_ref_app::sleep_ms(); }
