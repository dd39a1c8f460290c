/* Stand-in for stb_image.h.  Its implementation section includes <stdlib.h> and <math.h>,
 * which decide that pow/sqrt/abs on floats bind to the float overloads in the reference's
 * tracers (tests/test_oracle_kat.py::test_overload_probe): keep both. */
#pragma once
#include <stdlib.h>
#include <math.h>
