"""Shared helpers of the test-suite (not collected by pytest)."""
import numpy as np

import oracle
from vulkan_renderer_amd import renderer, synthetic


def oracle_render(host_scene, visibility=None, math_mode=1, bvh=None, width=None, height=None):
    """Shades the host scene with the CPU oracle.  Returns (image, inputs, bvh)."""
    inputs = host_scene.host_inputs()
    e = host_scene.app.swapchain.extent
    if bvh is None:
        bvh = oracle.Bvh(inputs["quantized_positions"], inputs["dequantization_factor"], inputs["dequantization_summand"])
    if visibility is None:
        cam = host_scene.app.scene_specification.camera
        visibility = oracle.primary_visibility(inputs["constants"], bvh, e.width, e.height, cam.near, cam.far)
    inputs["visibility"] = visibility
    frame = oracle.make_frame(inputs, host_scene.oracle_settings(), bvh)
    oracle.set_math_mode(math_mode)
    try:
        image = oracle.shade(frame)
    finally:
        oracle.set_math_mode(0)
    return image, inputs, bvh


def compare(gpu, cpu):
    """Error statistics over RGB of exposure-scaled radiance."""
    a, b = gpu[..., :3].astype(np.float64), cpu[..., :3].astype(np.float64)
    diff = np.abs(a - b)
    per_pixel = diff.max(axis=-1)
    return {
        "rmse": float(np.sqrt(((a - b) ** 2).mean())),
        "max_abs": float(diff.max()),
        "mismatched_pixels": int((per_pixel > 0).sum()),
        "pixels_over_1e-3": int((per_pixel > 1e-3).sum()),
        "nan": int(np.isnan(gpu).sum()),
        "bit_exact": bool(np.array_equal(gpu.view(np.uint32), cpu.view(np.uint32))),
    }


class DeviceBuffer:
    """Plain HIP device memory through ctypes on the HIP runtime that
    libvkr_shading.so already loaded (keeps torch out of the GPU tests)."""
    import ctypes as _C
    _hip = None

    def __init__(self, nbytes):
        C = self._C
        if DeviceBuffer._hip is None:
            DeviceBuffer._hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.ptr = C.c_void_p()
        assert DeviceBuffer._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0
        assert DeviceBuffer._hip.hipMemset(self.ptr, 0, C.c_size_t(nbytes)) == 0

    def upload(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        assert DeviceBuffer._hip.hipMemcpy(self.ptr, self._C.c_void_p(a.ctypes.data), self._C.c_size_t(a.nbytes), 1) == 0

    def download(self, shape, dtype):
        out = np.zeros(shape, dtype)
        assert out.nbytes <= self.nbytes
        assert DeviceBuffer._hip.hipDeviceSynchronize() == 0
        assert DeviceBuffer._hip.hipMemcpy(self._C.c_void_p(out.ctypes.data), self.ptr, self._C.c_size_t(out.nbytes), 2) == 0
        return out

    def zero(self):
        assert DeviceBuffer._hip.hipMemset(self.ptr, 0, self._C.c_size_t(self.nbytes)) == 0
        assert DeviceBuffer._hip.hipDeviceSynchronize() == 0

    def free(self):
        if self.ptr:
            DeviceBuffer._hip.hipFree(self.ptr)
            self.ptr = None


# ---- what the GPU tests of the frame filter and of the frame history share ---------------------------------------------

GUARD_BYTE, GUARD_BYTES = 0xA5, 256


class Arena:
    """[guard][out_colour][guard][out_variance][guard] in one allocation"""

    def __init__(self, width, height):
        self.shape = (height, width, 4)
        self.image_bytes = width * height * 16
        self.stride = GUARD_BYTES + self.image_bytes
        self.outputs = DeviceBuffer(2 * self.stride + GUARD_BYTES)
        self.reset()

    def reset(self):
        self.outputs.upload(np.full(self.outputs.nbytes, GUARD_BYTE, np.uint8))

    def address(self, index):
        return self.outputs.ptr.value + GUARD_BYTES + index * self.stride

    def read(self):
        """-> (out_colour, out_variance, whether every guard byte is intact)"""
        after = self.outputs.download((self.outputs.nbytes,), np.uint8)
        parts = [after[GUARD_BYTES + i * self.stride:GUARD_BYTES + i * self.stride + self.image_bytes] for i in range(2)]
        guards = [after[i * self.stride:i * self.stride + GUARD_BYTES] for i in range(3)]
        return (parts[0].view(np.float32).reshape(self.shape), parts[1].view(np.float32).reshape(self.shape),
                all((guard == GUARD_BYTE).all() for guard in guards))

    def untouched(self):
        return (self.outputs.download((self.outputs.nbytes,), np.uint8) == GUARD_BYTE).all()

    def free(self):
        self.outputs.free()


def differing(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


def assert_same_bits(got, want, what):
    different = differing(got, want)
    assert not different.any(), (what, int(different.sum()), np.argwhere(different)[:4].tolist(), got[different][:2], want[different][:2])


def flush_c_output():
    import ctypes
    ctypes.CDLL(None).fflush(None)


def open_renderer(dataset, arithmetic="libm", extent=(83, 45), **arguments):
    """A renderer behind whose pass the filter and the history run: the frame of tests/feature_buffer_cases.py with
    animated noise, its visibility rendered"""
    import feature_buffer_cases
    r = renderer.Renderer(arithmetic=arithmetic, **arguments)
    feature_buffer_cases.apply_frame(r, dataset, extent[0], extent[1], sample_count=1)
    r.app.render_settings.animate_noise = 1
    r.app.noise_table.random_seed = 4711
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


# ---- pixels on a discontinuity of the shader ---------------------------------------------------
#
# Two arithmetics that agree to a few ulp per operation (libm vs polynomial transcendentals, IEEE vs
# approximate reciprocals) produce frames that agree to ~1e-5 everywhere except at pixels where a
# last-bit difference is pushed through a discontinuity of the shader itself:
#   guard        the NaN guard of the reference (src/shaders/shading_pass.frag.glsl:861-864): a sliver
#                sector makes normalize_approx_and_flip(0) = NaN ("undefined if rhs is zero",
#                polygon_sampling.glsl:597-611) and the pixel is painted (1, 0, 0.8); whether a sample
#                lands in such a sector is decided by the last bits of the sector areas
#   silhouette   a shadow ray whose direction differs in the last bits passes a triangle edge on the
#                other side: one whole estimator term appears or disappears (ray query, :120-138).
#                Recognised mechanically: the two frames agree at that pixel when rendered WITHOUT
#                shadow rays
#   other        anything else - must not exist
GUARD_COLOR = np.array([1.0, 0.0, 0.8])


def is_guard_pixel(image):
    return np.abs(image[..., :3].astype(np.float64) - GUARD_COLOR).max(axis=-1) < 1.0e-5


def classify_outliers(a, b, a_without_rays=None, b_without_rays=None, threshold=1.0e-2):
    """Statistics of frame `a` against frame `b` (same scene and settings, two arithmetics) with
    every pixel that differs by more than `threshold` put into one of the classes above.
    The frames without shadow rays are only needed if such pixels exist outside the guard class."""
    da = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    per_pixel = np.abs(np.nan_to_num(da, nan=1.0e3)).max(axis=-1)
    outlier = per_pixel > threshold
    guard = outlier & (is_guard_pixel(a) | is_guard_pixel(b))
    rest = outlier & ~guard
    silhouette = np.zeros_like(rest)
    if rest.any() and a_without_rays is not None and b_without_rays is not None:
        dn = np.abs(a_without_rays[..., :3].astype(np.float64) - b_without_rays[..., :3].astype(np.float64)).max(axis=-1)
        silhouette = rest & (dn <= threshold)
    other = rest & ~silhouette
    inlier = ~outlier
    return {
        "rmse": float(np.sqrt((np.nan_to_num(da, nan=1.0e3) ** 2).mean())),
        "rmse_without_outliers": float(np.sqrt((da[inlier] ** 2).sum() / da.size)),
        "pixels_over_threshold": int(outlier.sum()), "threshold": threshold,
        "guard_pixels": int(guard.sum()), "silhouette_pixels": int(silhouette.sum()), "other_pixels": int(other.sum()),
        "guard_pixels_in_a": int(is_guard_pixel(a).sum()), "guard_pixels_in_b": int(is_guard_pixel(b).sum()),
        "other_coordinates": [tuple(int(v) for v in yx) for yx in np.argwhere(other)[:8]],
    }


# ---- inputs and expectations of the output encoders (tests/test_output_encoding.py, test_gpu_output_encoding.py) ----

# quiet and signalling NaNs, several payloads; the same with the sign bit
NAN_BITS = [0x7FC00000, 0x7FC00001, 0x7FFFFFFF, 0x7F800001, 0x7FBFFFFF, 0x7FA5A5A5, 0x7FD00000, 0x7F802000]
NAN_BITS = NAN_BITS + [b | 0x80000000 for b in NAN_BITS]
FLOAT_MAX_BITS = 0x7F7FFFFF


def from_bits(bits):
    return np.asarray(bits, np.uint64).astype(np.uint32).view(np.float32)


def unorm8(x):
    """The UNORM8 store of the reference in float32: clamp to [0, 1], x * 255 + 0.5, truncated; NaN gives 0."""
    x = np.asarray(x, np.float32)
    x = np.where(np.isnan(x), np.float32(0), np.minimum(np.maximum(x, np.float32(0)), np.float32(1))).astype(np.float32)
    return (x * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def srgb8_by_starts(x, starts):
    """sRGB8 code of every float of x by the oracle's code table (oracle.srgb8_code_starts()): the last code whose
    start x has reached in [0, 1]; NaN and everything <= 0 give 0, everything >= 1 gives 255."""
    x = np.asarray(x, np.float32).ravel()
    inside = np.where((x > 0) & (x < 1), x, np.float32(0)).view(np.uint32)
    code = np.searchsorted(starts, inside, side="right") - 1
    return np.where(x >= 1, 255, np.where((x > 0) & (x < 1), code, 0)).astype(np.uint8)


def codes_of_range(starts, first, count):
    """sRGB8 codes of the floats with the consecutive bit patterns first ... first + count - 1 (from [0, 1];
    whatever lies beyond 1.0 is taken as 1.0): code c for every position from its start on."""
    edges = np.append(np.clip(starts.astype(np.int64) - first, 0, count), count)
    return np.repeat(np.arange(256, dtype=np.uint8), np.diff(edges))


def encoder_specials():
    """Floats where an sRGB8 / UNORM8 encoder goes wrong: signed zeros, denormals, negatives, values above 1, the
    extremes, +-inf and NaNs, 1 - ulp and 1 + ulp."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x00000002, 0x003FFFFF, 0x00400000, 0x007FFFFF, 0x00800000, 0x00800001,
            0x80000001, 0x807FFFFF, 0x80800000, 0xBF800000, 0xBF000000, 0xB3800000, 0xFF7FFFFF, 0xFF800000,
            0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x3FC00000, 0x40000000, 0x4B000000, 0x7149F2CA, FLOAT_MAX_BITS, 0x7F800000,
            0x3B4D2E1C, 0x3B4D2E1B, 0x3B4D2E1D]  # (0.0031308f and its neighbours: the two branches of linear_to_srgb)
    return from_bits(bits + NAN_BITS)


def half_test_values():
    """Inputs of the half-float split (frame_bits 1 and 2) without the sweeps: every finite half and +-inf; for every
    two adjacent halves (65504 and the 65536 it would round up to included) the float midpoint and its two float
    neighbours, so that ties to even are exercised in every binade; NaNs of both signs with several payloads."""
    halves = np.arange(0, 0x7C01, dtype=np.uint16).view(np.float16).astype(np.float32)  # +0 ... 65504, +inf
    ladder = np.append(halves[:-1], np.float32(65536)).astype(np.float64)
    middle = ((ladder[:-1] + ladder[1:]) / 2).astype(np.float32)  # (12 significant bits: exact in float32)
    around = np.concatenate([middle, np.nextafter(middle, np.float32(-np.inf)), np.nextafter(middle, np.float32(np.inf))])
    positive = np.concatenate([halves, around])
    return np.concatenate([positive, -positive, from_bits(NAN_BITS)]).astype(np.float32)


# the exhaustive ranges of the half split, as first and last bit pattern: every float of the binades 2^-26 ... 2^-15
# (rounding into and inside the half subnormal range, 2^-14 is the smallest normal half), every float from 65504 to
# 2^17 (rounding to 65504 and overflow to infinity)
HALF_SWEEPS = [(0x32800000, 0x38800000), (0x477FE000, 0x48000000)]


def half_sweep_chunks(chunk=1 << 24):
    for first, last in HALF_SWEEPS:
        for start in range(first, last + 1, chunk):
            yield np.arange(start, min(start + chunk, last + 1), dtype=np.uint32).view(np.float32)
