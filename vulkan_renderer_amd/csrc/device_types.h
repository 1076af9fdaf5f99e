// The arithmetic mode of a translation unit (device_math.h describes the three) and the vector types of the device
// code: what a header needs that declares device data or a VKR_DEV function and computes nothing.  The arithmetic itself
// is device_math.h, which brings glibc_math.h with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VKR_MATH_MODE
#define VKR_MATH_MODE 0
#endif
#define VKR_FAST_MATH (VKR_MATH_MODE == 1)
// glibc's functions in both IEEE modes (mode 0 keeps the polynomial arctangent: VKR_MATH_MODE == 2 in device_math.h)
#define VKR_LIBM_MATH (VKR_MATH_MODE != 1)

#define VKR_DEV __device__ __forceinline__

namespace vkr {

struct f2 { float x, y; };
struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

}  // namespace vkr
