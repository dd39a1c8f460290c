/* Null stand-in for glbinding's gl.h (application build, see ../../intrin.h): the scalar
 * types, GLenum, the enumerators that Renderer.hpp names, and functions that do nothing.
 * Our own text.  No function reads or writes through a pointer it is given, except the
 * out-parameters below: shader and program queries report success, object names are
 * non-zero, and a uniform's location is >= 0, so that the reference's Startup() takes
 * the path it takes with a working GL.  g_data reaches glTexImage2D only, which ignores it.
 * (`class`, not `typename`, in the templates: ref_standins/intrin.h defines `typename`
 * away.) */
#pragma once
namespace gl {

typedef unsigned int GLuint;
typedef int GLint;
typedef int GLsizei;
typedef char GLchar;
typedef float GLfloat;
typedef unsigned int GLenum;

#define SPT_REF_GL_ENUM(name, value) constexpr GLenum name = value;
SPT_REF_GL_ENUM(GL_FALSE, 0)
SPT_REF_GL_ENUM(GL_TRIANGLES, 0x0004)
SPT_REF_GL_ENUM(GL_FRONT_AND_BACK, 0x0408)
SPT_REF_GL_ENUM(GL_TEXTURE_2D, 0x0DE1)
SPT_REF_GL_ENUM(GL_UNSIGNED_BYTE, 0x1401)
SPT_REF_GL_ENUM(GL_UNSIGNED_INT, 0x1405)
SPT_REF_GL_ENUM(GL_FLOAT, 0x1406)
SPT_REF_GL_ENUM(GL_RGB, 0x1907)
SPT_REF_GL_ENUM(GL_FILL, 0x1B02)
SPT_REF_GL_ENUM(GL_NEAREST, 0x2600)
SPT_REF_GL_ENUM(GL_LINEAR, 0x2601)
SPT_REF_GL_ENUM(GL_TEXTURE_MAG_FILTER, 0x2800)
SPT_REF_GL_ENUM(GL_TEXTURE_MIN_FILTER, 0x2801)
SPT_REF_GL_ENUM(GL_TEXTURE_WRAP_S, 0x2802)
SPT_REF_GL_ENUM(GL_TEXTURE_WRAP_T, 0x2803)
SPT_REF_GL_ENUM(GL_COLOR_BUFFER_BIT, 0x4000)
SPT_REF_GL_ENUM(GL_CLAMP_TO_BORDER, 0x812D)
SPT_REF_GL_ENUM(GL_CLAMP_TO_EDGE, 0x812F)
SPT_REF_GL_ENUM(GL_TEXTURE0, 0x84C0)
SPT_REF_GL_ENUM(GL_ARRAY_BUFFER, 0x8892)
SPT_REF_GL_ENUM(GL_ELEMENT_ARRAY_BUFFER, 0x8893)
SPT_REF_GL_ENUM(GL_STATIC_DRAW, 0x88E4)
SPT_REF_GL_ENUM(GL_FRAGMENT_SHADER, 0x8B30)
SPT_REF_GL_ENUM(GL_VERTEX_SHADER, 0x8B31)
SPT_REF_GL_ENUM(GL_COMPILE_STATUS, 0x8B81)
SPT_REF_GL_ENUM(GL_LINK_STATUS, 0x8B82)
#undef SPT_REF_GL_ENUM

/* calls whose arguments are ignored and that return nothing */
#define SPT_REF_GL_NOOP(name) \
    template <class... Args> inline void name(Args...) {}
SPT_REF_GL_NOOP(glShaderSource)
SPT_REF_GL_NOOP(glCompileShader)
SPT_REF_GL_NOOP(glGetShaderInfoLog)
SPT_REF_GL_NOOP(glAttachShader)
SPT_REF_GL_NOOP(glLinkProgram)
SPT_REF_GL_NOOP(glGetProgramInfoLog)
SPT_REF_GL_NOOP(glDeleteShader)
SPT_REF_GL_NOOP(glBindVertexArray)
SPT_REF_GL_NOOP(glBindBuffer)
SPT_REF_GL_NOOP(glBufferData)
SPT_REF_GL_NOOP(glEnableVertexAttribArray)
SPT_REF_GL_NOOP(glVertexAttribPointer)
SPT_REF_GL_NOOP(glUseProgram)
SPT_REF_GL_NOOP(glUniform1i)
SPT_REF_GL_NOOP(glBindTexture)
SPT_REF_GL_NOOP(glTexParameteri)
SPT_REF_GL_NOOP(glTexImage2D)
SPT_REF_GL_NOOP(glGenerateMipmap)
SPT_REF_GL_NOOP(glDeleteVertexArrays)
SPT_REF_GL_NOOP(glDeleteBuffers)
SPT_REF_GL_NOOP(glViewport)
SPT_REF_GL_NOOP(glClearColor)
SPT_REF_GL_NOOP(glClear)
SPT_REF_GL_NOOP(glActiveTexture)
SPT_REF_GL_NOOP(glUniform4f)
SPT_REF_GL_NOOP(glUniformMatrix4fv)
SPT_REF_GL_NOOP(glPolygonMode)
SPT_REF_GL_NOOP(glDrawElements)
#undef SPT_REF_GL_NOOP

/* object names: non-zero, as a working GL hands them out */
inline GLuint spt_ref_gl_name()
{
    static GLuint next = 0;
    return ++next;
}
inline GLuint glCreateShader(GLenum) { return spt_ref_gl_name(); }
inline GLuint glCreateProgram() { return spt_ref_gl_name(); }
inline void glGenVertexArrays(GLsizei n, GLuint *names) { for (GLsizei i = 0; i < n; ++i) names[i] = spt_ref_gl_name(); }
inline void glGenBuffers(GLsizei n, GLuint *names) { for (GLsizei i = 0; i < n; ++i) names[i] = spt_ref_gl_name(); }
inline void glGenTextures(GLsizei n, GLuint *names) { for (GLsizei i = 0; i < n; ++i) names[i] = spt_ref_gl_name(); }

/* queries: success */
inline void glGetShaderiv(GLuint, GLenum, GLint *status) { *status = 1; }
inline void glGetProgramiv(GLuint, GLenum, GLint *status) { *status = 1; }
inline GLint glGetUniformLocation(GLuint, const GLchar *) { return 0; }

}  // namespace gl
