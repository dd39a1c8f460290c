/* Null stand-in for glbinding/Binding.h (application build, see ../intrin.h): there is no
 * GL to bind, so initialize() takes the loader and does nothing. */
#pragma once
namespace glbinding {
struct Binding {
    template <class Loader> static void initialize(Loader) {}
};
}  // namespace glbinding
