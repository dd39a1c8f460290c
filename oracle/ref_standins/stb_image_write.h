/* Stand-in for stb_image_write.h: <stdlib.h> and <math.h> as its implementation section
 * includes them (see stb_image.h beside this file), and the one function the reference's
 * SaveImage names; the harness never saves an image. */
#pragma once
#include <stdlib.h>
#include <math.h>
inline int stbi_write_bmp(char const *, int, int, int, const void *) { return 0; }
