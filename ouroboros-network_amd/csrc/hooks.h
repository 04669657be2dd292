// hooks.h -- the test hooks of the host runtime, included by the host units
// that are compiled a second time for the test build (runtime.cpp, plan.cpp).
#pragma once
#include "knobs.h"

// TEST HOOKS, compiled only into the test build (lib/libouro_verify_test.so,
// -DOURO_TEST_HOOKS=1; tests/test_gpu_hooks.py runs the hook tests in a child
// process on it): with OURO_TEST_DEVICE_ERROR set in the environment every
// launch reports a device error, so the tests reach the host recompute path
// on a healthy GPU; OURO_TEST_PLAN_POISON (plan.cpp plan_poison).  The product
// library reads neither variable.  The other decisions the macro switches:
// runtime.cpp split_launch (OURO_SPLIT) and lat_skip_mask (OURO_LAT_SKIP),
// plan.cpp's sentinel (OURO_TEST_PLAN_SENTINEL), ouro_debug_test_hooks.
#ifndef OURO_TEST_HOOKS
#define OURO_TEST_HOOKS 0
#endif

#pragma GCC visibility push(hidden)
namespace ouro_rt {
#if OURO_TEST_HOOKS
inline bool injected_device_error() { return ouro_knobs::get().test_device_error.load(std::memory_order_relaxed); }
#else
constexpr bool injected_device_error() { return false; }
#endif
}  // namespace ouro_rt
#pragma GCC visibility pop
