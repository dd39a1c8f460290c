/* Stand-in for GLFW: the window type that the reference's Globals.hpp points to. */
#pragma once
struct GLFWwindow;
