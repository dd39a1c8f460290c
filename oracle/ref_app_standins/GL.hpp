/* Renderer.hpp:9 includes <GL.hpp>; the reference's file is Gl.hpp (the same file where
 * file names ignore case).  Our own text: it only forwards. */
#pragma once
#include <Gl.hpp>
