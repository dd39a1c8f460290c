/* Stand-in for glbinding/Binding.h: the harness never binds GL. */
#pragma once
