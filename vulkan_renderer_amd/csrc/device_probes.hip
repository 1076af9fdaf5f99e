// Probes for the test-suite: the device's arithmetic primitives (device_math.h, glibc_math.h) and the texture sampler
// on inputs of the caller's choice, the division window, a copy with a chosen number of workgroups.
// This unit is compiled in exact mode with -ffp-contract=off, as the libm- and exact-mode shading kernels are: what
// the tests of device_math.h see here is the arithmetic those kernels use.
#include "shade_launchers.h"
#include "pass_internal.h"
#include "device_math.h"

using namespace vkr;

static const sampler_launch_function_t g_sampler_launchers[3] = VKR_MODE_LAUNCHERS(vkr_launch_texture_sampler);

// evaluate_device_arithmetic(): the primitives as the shading kernels use them
__global__ void __launch_bounds__(256) k_evaluate_arithmetic(uint32_t operation, const float* a, const float* b, float* out, uint32_t count) {
	uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= count) return;
	float x = a[i], y = b ? b[i] : 0.0f;
	switch (operation) {
	case 0: out[i] = divide(x, y); break;
	case 1: out[i] = square_root(x); break;
	case 2: out[i] = rsqrt(x); break;
	case 3: out[i] = x / y; break;
	case 4: out[i] = sqrtf(x); break;
	// the functions of the libm arithmetic mode (glibc_math.h with this file's divide / square_root)
	case 5: out[i] = gm_atanf(x); break;
	case 6: out[i] = gm_acosf(x); break;
	case 7: out[i] = gm_sinf(x); break;
	case 8: out[i] = gm_cosf(x); break;
	case 9: out[i] = gm_log2f(x); break;
	case 10: out[i] = gm_powf(x, y); break;
	case 11: out[i] = gm_atan2f(x, y); break;
	case 12: out[i] = inverse_square_root_ieee(x); break;
	default: out[i] = rsqrt(x); break;  // (what the kernels of this unit's arithmetic mode use)
	}
}

// compare_device_arithmetic(): two one-argument operations of k_evaluate_arithmetic over a range of bit
// patterns, without moving the arguments through the host
__device__ __forceinline__ float evaluate_unary(uint32_t operation, float x, const gm_atan_row_t* atan_rows) {
	switch (operation) {
	case 17: return gm_atanf_rows(x, atan_rows);
	case 1: return square_root(x);
	case 4: return sqrtf(x);
	case 5: return gm_atanf(x);
	case 12: return inverse_square_root_ieee(x);
	case 16: return 1.0f / sqrtf(x);
	default: return rsqrt(x);
	}
}
__global__ void __launch_bounds__(256) k_compare_arithmetic(uint32_t operation_a, uint32_t operation_b, uint32_t first_bits, uint64_t count, unsigned long long* out) {
	// (the table of the arctangent's argument ranges, in LDS as in the shading kernels)
	__shared__ gm_atan_row_t atan_rows[GM_ATAN_ROW_COUNT];
	for (uint32_t i = threadIdx.x; i < GM_ATAN_ROW_COUNT; i += 256u) atan_rows[i] = gm_atan_row(i);
	__syncthreads();
	unsigned long long mismatches = 0;
	for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t) gridDim.x * 256u) {
		uint32_t bits = first_bits + (uint32_t) i;
		float x = __uint_as_float(bits), a = evaluate_unary(operation_a, x, atan_rows), b = evaluate_unary(operation_b, x, atan_rows);
		bool same = __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
		if (!same) { ++mismatches; atomicMin(out + 1, (unsigned long long) bits); }
	}
	if (mismatches) atomicAdd(out, mismatches);
}

// {mismatches, first mismatch}: two counters on the device that start as {0, ~0}; `launch` queues the kernel that counts
// into them on the device's stream, then they are read back
template <typename LAUNCH>
static int count_mismatches(const device_t* device, uint64_t out_mismatches_and_first[2], LAUNCH launch) {
	unsigned long long* counters = NULL;
	if (hip_failed(hipMalloc(&counters, 2 * sizeof(unsigned long long)), "allocating counters")) return 1;
	hipStream_t stream = (hipStream_t) device->stream;
	unsigned long long initial[2] = {0ull, ~0ull};
	int failed = hip_failed(hipMemcpyAsync(counters, initial, sizeof(initial), hipMemcpyHostToDevice, stream), "clearing counters");
	if (!failed) {
		launch(counters, stream);
		failed = vkr_copy_to_host(out_mismatches_and_first, counters, 2 * sizeof(unsigned long long), device);
	}
	(void) hipFree(counters);
	return failed;
}

extern "C" int compare_device_arithmetic(const device_t* device, uint32_t operation_a, uint32_t operation_b, uint32_t first_bits, uint64_t count, uint64_t out_mismatches_and_first[2]) {
	if (!device || !out_mismatches_and_first || count > (1ull << 32)) {
		printf("compare_device_arithmetic() needs a device, an output and at most 2^32 arguments.\n");
		return 1;
	}
	return count_mismatches(device, out_mismatches_and_first, [=](unsigned long long* counters, hipStream_t stream) {
		k_compare_arithmetic<<<8192, 256, 0, stream>>>(operation_a, operation_b, first_bits, count, counters);
	});
}

// compare_device_division(): divide() against the compiler's IEEE a / b for a block of divisor
// significands and EVERY dividend significand (blockIdx.y = divisor, the threads of its blocks share the dividends)
__global__ void __launch_bounds__(256) k_compare_division(uint32_t first_significand, uint32_t stride, uint32_t dividend_exponent, uint32_t divisor_exponent, unsigned long long* out) {
	const uint32_t b_bits = (divisor_exponent << 23) | ((first_significand + blockIdx.y * stride) & 0x7FFFFFu);
	const float b = __uint_as_float(b_bits);
	unsigned long long mismatches = 0;
	for (uint32_t m = blockIdx.x * 256u + threadIdx.x; m < (1u << 23); m += gridDim.x * 256u) {
		const uint32_t a_bits = (dividend_exponent << 23) | m;
		const float a = __uint_as_float(a_bits);
		float mine = divide(a, b), theirs = __fdiv_rn(a, b);
		bool same = __float_as_uint(mine) == __float_as_uint(theirs) || (mine != mine && theirs != theirs);
		if (!same) { ++mismatches; atomicMin(out + 1, ((unsigned long long) b_bits << 32) | a_bits); }
	}
	if (mismatches) atomicAdd(out, mismatches);
}

extern "C" int compare_device_division(const device_t* device, uint32_t first_significand, uint32_t divisor_count, uint32_t stride, uint32_t dividend_exponent, uint32_t divisor_exponent, uint64_t out_mismatches_and_first[2]) {
	if (!device || !out_mismatches_and_first || divisor_count == 0 || divisor_count > 65535u || dividend_exponent > 254u || divisor_exponent > 254u) {
		printf("compare_device_division() needs a device, an output, 1 ... 65535 divisors and biased exponents below 255.\n");
		return 1;
	}
	return count_mismatches(device, out_mismatches_and_first, [=](unsigned long long* counters, hipStream_t stream) {
		k_compare_division<<<dim3(32, divisor_count), 256, 0, stream>>>(first_significand, stride, dividend_exponent, divisor_exponent, counters);
	});
}

__global__ void __launch_bounds__(256) k_copy_with_workgroups(uint4* destination, const uint4* source, uint64_t count) {
	for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < count; i += (uint64_t) gridDim.x * 256u) destination[i] = source[i];
}

extern "C" int copy_with_workgroups(void* destination, const void* source, uint64_t bytes, uint32_t workgroups, void* stream) {
	if (!destination || !source || bytes % 16 != 0 || workgroups == 0) {
		printf("copy_with_workgroups() needs two device buffers, a multiple of 16 bytes and at least one workgroup.\n");
		return 1;
	}
	if (bytes == 0) return 0;
	k_copy_with_workgroups<<<workgroups, 256, 0, (hipStream_t) stream>>>((uint4*) destination, (const uint4*) source, bytes / 16);
	return hip_failed(hipGetLastError(), "launching the copy");
}

extern "C" int evaluate_device_arithmetic(const device_t* device, uint32_t operation, const float* a, const float* b, float* out, uint32_t count) {
	if (!device || !a || !out || operation > 12 || ((operation == 0 || operation == 3 || operation == 10 || operation == 11) && !b)) {
		printf("evaluate_device_arithmetic() needs a device, operands and an operation in 0 ... 12.\n");
		return 1;
	}
	if (!count) return 0;
	hipStream_t stream = (hipStream_t) device->stream;
	float* buffers = NULL;
	size_t bytes = sizeof(float) * (size_t) count;
	if (hip_failed(hipMalloc(&buffers, 3 * bytes), "allocating the operands")) return 1;
	int failed = hip_failed(hipMemcpyAsync(buffers, a, bytes, hipMemcpyHostToDevice, stream), "uploading the operands")
		|| (b && hip_failed(hipMemcpyAsync(buffers + count, b, bytes, hipMemcpyHostToDevice, stream), "uploading the operands"));
	if (!failed) {
		k_evaluate_arithmetic<<<(count + 255u) / 256u, 256, 0, stream>>>(operation, buffers, b ? buffers + count : NULL, buffers + 2 * (size_t) count, count);
		failed = hip_failed(hipMemcpyAsync(out, buffers + 2 * (size_t) count, bytes, hipMemcpyDeviceToHost, stream), "reading the results back")
			|| hip_failed(hipStreamSynchronize(stream), "evaluating the arithmetic");
	}
	(void) hipFree(buffers);
	return failed;
}

// evaluate_device_texture_sampler(): the chain, the sRGB table of the pass (vkr_fill_srgb_table, what create_scene uploads)
// and the inputs go up, k_sample_texture of the chosen arithmetic mode runs, the samples come back
extern "C" int evaluate_device_texture_sampler(const device_t* device, int32_t arithmetic_mode, const uint8_t* texels_rgba8, uint32_t width, uint32_t height, uint32_t mip_count, VkBool32 srgb, const float* inputs, float* out_rgba, uint32_t count) {
	if (!device || !texels_rgba8 || !inputs || !out_rgba || arithmetic_mode < 0 || arithmetic_mode >= arithmetic_mode_count || width == 0 || height == 0 || width > 32768u || height > 32768u || mip_count == 0 || mip_count > 16u) {
		printf("evaluate_device_texture_sampler() needs a device, an arithmetic mode, a texture of 1 ... 32768 texels a side with 1 ... 16 levels, inputs and an output.\n");
		return 1;
	}
	if (!count) return 0;
	size_t texel_count = 0;
	for (uint32_t l = 0, w = width, h = height; l != mip_count; ++l) {
		texel_count += (size_t) w * h;
		w = w > 1 ? w / 2 : 1;
		h = h > 1 ? h / 2 : 1;
	}
	hipStream_t stream = (hipStream_t) device->stream;
	float table[256];
	vkr_fill_srgb_table(table);
	// one allocation: texels, table, inputs, outputs (each a multiple of 16 bytes long but the texels, which are padded)
	size_t texel_bytes = (4 * texel_count + 15) & ~(size_t) 15, input_bytes = 6 * sizeof(float) * (size_t) count, output_bytes = 4 * sizeof(float) * (size_t) count;
	size_t input_offset = texel_bytes + sizeof(table), output_offset = (input_offset + input_bytes + 15) & ~(size_t) 15;
	uint8_t* buffer = NULL;
	if (hip_failed(hipMalloc(&buffer, output_offset + output_bytes), "allocating the texture and the samples")) return 1;
	int failed = hip_failed(hipMemcpyAsync(buffer, texels_rgba8, 4 * texel_count, hipMemcpyHostToDevice, stream), "uploading the texture")
		|| hip_failed(hipMemcpyAsync(buffer + texel_bytes, table, sizeof(table), hipMemcpyHostToDevice, stream), "uploading the sRGB table")
		|| hip_failed(hipMemcpyAsync(buffer + input_offset, inputs, input_bytes, hipMemcpyHostToDevice, stream), "uploading the sampler inputs");
	if (!failed) {
		shade_params p = {};  // (the sampler reads the texels and the table, nothing else)
		p.texels = (const uint32_t*) buffer;
		p.srgb_table = (const float*) (buffer + texel_bytes);
		const uint32_t descriptor[4] = {0u, width, height, mip_count | (srgb ? 1u << 16 : 0u)};
		failed = g_sampler_launchers[arithmetic_mode](&p, descriptor, (const float*) (buffer + input_offset), (float*) (buffer + output_offset), count, stream)
			|| hip_failed(hipMemcpyAsync(out_rgba, buffer + output_offset, output_bytes, hipMemcpyDeviceToHost, stream), "reading the samples back")
			|| hip_failed(hipStreamSynchronize(stream), "sampling the texture");
	}
	(void) hipFree(buffer);
	return failed;
}
