/* Stand-in for glbinding's gl.h: the GL scalar types that the reference's Globals.hpp names.
 * The harness never calls GL. */
#pragma once
namespace gl { typedef unsigned int GLuint; typedef int GLint; typedef char GLchar; typedef float GLfloat; }
