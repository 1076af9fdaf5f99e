// Frame statistics on the device (include/vkr_frame_statistics.h): per-pixel sums of frames in binary64, mean and
// variance from them, and error sums of whole frames with a fixed order of additions.  Compiled without contraction
// like shading_pass.hip; every result is restated in numpy bit for bit (vulkan_renderer_amd/frame_statistics.py).
#include "vkr_frame_statistics.h"
#include "frame_images.h"

constexpr uint32_t kEventRing = VKR_MAX_ACCUMULATED_FRAMES * 2;
constexpr uint32_t kBlock = 256;
// (the grid's x extent)
constexpr uint64_t kMaxPixelCount = 0x7FFFFFFFull * kBlock;

// ---- kernels -----------------------------------------------------------------------------------------------------

template <int K> struct frame_sources {
	const float4* frame[K];
};

// One lane per pixel: K float4 loads, then each of the pixel's three accumulator pairs {S, Q} is read and written
// once ([channel][pixel]: 16-byte accesses, consecutive lanes consecutive addresses).  pixel_count * (16 K + 96) bytes.
template <int K> __global__ void __launch_bounds__(kBlock) k_accumulate_frames(frame_sources<K> sources, double2* sums, uint64_t pixel_count) {
	uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
	if (i >= pixel_count) return;
	float4 x[K];
#pragma unroll
	for (int k = 0; k != K; ++k) x[k] = sources.frame[k][i];
	double2 r = sums[i], g = sums[pixel_count + i], b = sums[2 * pixel_count + i];
	// (frame after frame: the order of the additions is the order of the frames)
#pragma unroll
	for (int k = 0; k != K; ++k) {
		double xr = (double) x[k].x, xg = (double) x[k].y, xb = (double) x[k].z;
		r.x += xr; r.y += xr * xr;
		g.x += xg; g.y += xg * xg;
		b.x += xb; b.y += xb * xb;
	}
	sums[i] = r;
	sums[pixel_count + i] = g;
	sums[2 * pixel_count + i] = b;
}

__device__ static inline double sample_variance(double2 sq, double n) {
	double v = (sq.y - (sq.x * sq.x) / n) / (n - 1.0);
	// (cancellation only: NaN and -0 fail the comparison and pass through)
	return v < 0.0 ? 0.0 : v;
}

__global__ void __launch_bounds__(kBlock) k_resolve_statistics(const double2* sums, uint64_t pixel_count, uint64_t frame_count, float4* out_mean, float4* out_variance) {
	uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x;
	if (i >= pixel_count) return;
	double n = (double) frame_count;
	double2 r = sums[i], g = sums[pixel_count + i], b = sums[2 * pixel_count + i];
	if (out_mean) out_mean[i] = make_float4((float) (r.x / n), (float) (g.x / n), (float) (b.x / n), 1.0f);
	if (out_variance) out_variance[i] = make_float4((float) sample_variance(r, n), (float) sample_variance(g, n), (float) sample_variance(b, n), 1.0f);
}

// Block B reduces the terms of pixels 256 B ... 256 B + 255 with the tree of the header and writes its three partials
// to partials[channel * gridDim.x + B].  squared_differences: e = ((double) a - (double) b)^2, else e = (double) a.
template <bool squared_differences> __global__ void __launch_bounds__(kBlock) k_reduce_frames(const float4* a, const float4* b, uint64_t pixel_count, double* partials) {
	__shared__ double slots[3][kBlock];
	uint32_t j = threadIdx.x;
	uint64_t i = (uint64_t) blockIdx.x * kBlock + j;
	double e[3] = {0.0, 0.0, 0.0};
	if (i < pixel_count) {
		float4 pa = a[i];
		e[0] = (double) pa.x; e[1] = (double) pa.y; e[2] = (double) pa.z;
		if (squared_differences) {
			float4 pb = b[i];
			double d0 = e[0] - (double) pb.x, d1 = e[1] - (double) pb.y, d2 = e[2] - (double) pb.z;
			e[0] = d0 * d0; e[1] = d1 * d1; e[2] = d2 * d2;
		}
	}
	for (int c = 0; c != 3; ++c) slots[c][j] = e[c];
	__syncthreads();
	for (uint32_t s = kBlock / 2; s != 0; s >>= 1) {
		if (j < s)
			for (int c = 0; c != 3; ++c) slots[c][j] += slots[c][j + s];
		__syncthreads();
	}
	if (j < 3) partials[(uint64_t) j * gridDim.x + blockIdx.x] = slots[j][0];
}

// ---- host side ---------------------------------------------------------------------------------------------------

static hipStream_t device_stream(const application_t* app) { return (hipStream_t) app->device.stream; }

static uint64_t frame_pixel_count(const application_t* app) { return (uint64_t) app->swapchain.extent.width * app->swapchain.extent.height; }

// Makes `stream` wait for the accumulations queued so far
static int wait_for_accumulations(const frame_statistics_t* stats, hipStream_t stream) {
	if (!stats->pending) return 0;
	hipEvent_t last = (hipEvent_t) stats->accumulated[(stats->next_event + kEventRing - 1) % kEventRing];
	return hip_failed(hipStreamWaitEvent(stream, last, 0), "waiting for the accumulations");
}

// Makes the object's stream wait for what device->stream has queued (sources produced there, a resolve that still reads the sums)
static int order_behind_device_stream(frame_statistics_t* stats, application_t* app) {
	return hip_failed(hipEventRecord((hipEvent_t) stats->source_ready, device_stream(app)), "marking the device stream")
		|| hip_failed(hipStreamWaitEvent((hipStream_t) stats->stream, (hipEvent_t) stats->source_ready, 0), "ordering the statistics behind the device stream");
}

extern "C" void destroy_frame_statistics(frame_statistics_t* stats, application_t* app) {
	if (stats->stream) (void) hipStreamSynchronize((hipStream_t) stats->stream);
	// (a resolve on device->stream may still read the sums)
	if (stats->resolved && app) (void) hipStreamSynchronize(device_stream(app));
	for (uint32_t i = 0; i != kEventRing + 2; ++i) {
		void* event = i < kEventRing ? stats->accumulated[i] : (i == kEventRing ? stats->resolved : stats->source_ready);
		if (!event) continue;
		// (the pass may still hold the event as the reader of a target)
		if (app) vkr_forget_target_reader(app, event);
		(void) hipEventDestroy((hipEvent_t) event);
	}
	if (stats->stream) (void) hipStreamDestroy((hipStream_t) stats->stream);
	if (stats->sums) (void) hipFree(stats->sums);
	memset(stats, 0, sizeof(*stats));
}

extern "C" int create_frame_statistics(frame_statistics_t* stats, application_t* app, uint64_t pixel_count) {
	memset(stats, 0, sizeof(*stats));
	if (!pixel_count) pixel_count = frame_pixel_count(app);
	if (!pixel_count || pixel_count > kMaxPixelCount) {
		printf("Frame statistics need between 1 and %llu pixels (a pixel count, or a swapchain extent).\n", (unsigned long long) kMaxPixelCount);
		return 1;
	}
	stats->pixel_count = pixel_count;
	size_t bytes = sizeof(double2) * 3 * (size_t) pixel_count;
	hipStream_t stream = NULL;
	if (hipMalloc(&stats->sums, bytes) != hipSuccess) {
		printf("Failed to allocate %.1f MiB for the sums of %llu pixels.\n", bytes / 1048576.0, (unsigned long long) pixel_count);
		stats->sums = NULL;
		return 1;
	}
	int failed = hip_failed(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "creating the statistics stream");
	stats->stream = stream;
	failed = failed || hip_failed(hipEventCreateWithFlags((hipEvent_t*) &stats->source_ready, kSyncEventFlags), "creating statistics events")
		|| hip_failed(hipEventCreateWithFlags((hipEvent_t*) &stats->resolved, kSyncEventFlags), "creating statistics events");
	for (uint32_t i = 0; i != kEventRing && !failed; ++i)
		failed = hip_failed(hipEventCreateWithFlags((hipEvent_t*) &stats->accumulated[i], kSyncEventFlags), "creating statistics events");
	// (the stream's first kernel pays for its hardware queue: see host/device.c)
	failed = failed || (!getenv("VKR_NO_WARM_UP") && vkr_launch_empty_kernel(stream))
		|| hip_failed(hipMemsetAsync(stats->sums, 0, bytes, stream), "clearing the sums")
		|| hip_failed(hipStreamSynchronize(stream), "clearing the sums");
	if (failed) {
		destroy_frame_statistics(stats, app);
		return 1;
	}
	return 0;
}

extern "C" int reset_frame_statistics(frame_statistics_t* stats, application_t* app) {
	if (!stats->sums) return 1;
	stats->frame_count = 0;
	return order_behind_device_stream(stats, app)
		|| hip_failed(hipMemsetAsync(stats->sums, 0, sizeof(double2) * 3 * (size_t) stats->pixel_count, (hipStream_t) stats->stream), "clearing the sums");
}

template <int K> static void launch_accumulate(const void* const* frames, frame_statistics_t* stats) {
	frame_sources<K> sources;
	for (int k = 0; k != K; ++k) sources.frame[k] = (const float4*) frames[k];
	k_accumulate_frames<K><<<block_count(stats->pixel_count, kBlock), kBlock, 0, (hipStream_t) stats->stream>>>(sources, (double2*) stats->sums, stats->pixel_count);
}

extern "C" int accumulate_frames(frame_statistics_t* stats, application_t* app, const void* const* device_frames, uint32_t count) {
	const void* target = app->render_targets.radiance;
	if (!device_frames) {
		device_frames = &target;
		count = 1;
		if (stats->pixel_count > frame_pixel_count(app)) {
			printf("accumulate_frames(): the statistics cover %llu pixels, the radiance target holds %llu.\n", (unsigned long long) stats->pixel_count, (unsigned long long) frame_pixel_count(app));
			return 1;
		}
	}
	if (!stats->sums || count < 1 || count > VKR_MAX_ACCUMULATED_FRAMES) {
		printf("accumulate_frames() takes 1 to %d frames per call and a statistics object that was created.\n", VKR_MAX_ACCUMULATED_FRAMES);
		return 1;
	}
	for (uint32_t k = 0; k != count; ++k)
		if (!device_frames[k]) {
			printf("accumulate_frames(): frame %u is NULL (no render targets?).\n", k);
			return 1;
		}
	hipStream_t stream = (hipStream_t) stats->stream;
	// behind the frames in flight (the sources may be the targets of several of them) and behind what device->stream
	// has queued, like begin_read_back()
	if (vkr_order_behind_frames_in_flight(app, stream) || order_behind_device_stream(stats, app)) return 1;
	switch (count) {
		case 1: launch_accumulate<1>(device_frames, stats); break;
		case 2: launch_accumulate<2>(device_frames, stats); break;
		case 3: launch_accumulate<3>(device_frames, stats); break;
		case 4: launch_accumulate<4>(device_frames, stats); break;
		case 5: launch_accumulate<5>(device_frames, stats); break;
		case 6: launch_accumulate<6>(device_frames, stats); break;
		case 7: launch_accumulate<7>(device_frames, stats); break;
		default: launch_accumulate<8>(device_frames, stats); break;
	}
	if (hip_failed(hipGetLastError(), "accumulating frames")) return 1;
	stats->frame_count += count;
	// later frames that write one of the sources wait for this event in front of the kernel that writes
	void* done = stats->accumulated[stats->next_event];
	if (hip_failed(hipEventRecord((hipEvent_t) done, stream), "marking the accumulation")) return 1;
	stats->next_event = (stats->next_event + 1) % kEventRing;
	stats->pending = 1;
	// (only a pass writes frames, and it is the pass that keeps the readers)
	if (app->shading_pass.constants_device)
		for (uint32_t k = 0; k != count; ++k) vkr_note_target_reader(app, done, device_frames[k], sizeof(float4) * (size_t) stats->pixel_count);
	return 0;
}

extern "C" int resolve_frame_statistics(frame_statistics_t* stats, application_t* app, void* out_mean, void* out_variance) {
	if (!stats->sums || !stats->frame_count) {
		printf("resolve_frame_statistics() needs at least one accumulated frame.\n");
		return 1;
	}
	if (out_variance && stats->frame_count < 2) {
		printf("A variance needs at least two accumulated frames (%llu so far).\n", (unsigned long long) stats->frame_count);
		return 1;
	}
	if (!out_mean && !out_variance) return 0;
	hipStream_t stream = device_stream(app);
	size_t bytes = sizeof(float4) * (size_t) stats->pixel_count;
	// frames in flight may still write (or read) an output such as the radiance target; so may read-backs
	if (finish_frames(app) || wait_for_accumulations(stats, stream)) return 1;
	if (out_mean) vkr_order_target_write(app, out_mean, bytes, stream);
	if (out_variance) vkr_order_target_write(app, out_variance, bytes, stream);
	k_resolve_statistics<<<block_count(stats->pixel_count, kBlock), kBlock, 0, stream>>>((const double2*) stats->sums, stats->pixel_count, stats->frame_count, (float4*) out_mean, (float4*) out_variance);
	if (hip_failed(hipGetLastError(), "resolving the statistics")) return 1;
	const frame_call call = {"resolve_frame_statistics", {}, {out_mean, out_variance}};
	return finish_frame_call(call, app, bytes, stats->resolved, "marking the resolve");
}

extern "C" int read_back_frame_statistics(frame_statistics_t* stats, application_t* app, double* sums, double* squares) {
	if (!stats->sums) return 1;
	hipStream_t stream = device_stream(app);
	size_t pixel_count = (size_t) stats->pixel_count;
	double* channel = (double*) malloc(sizeof(double) * 2 * pixel_count);
	if (!channel) {
		printf("Out of memory reading the statistics back.\n");
		return 1;
	}
	int failed = wait_for_accumulations(stats, stream);
	for (uint32_t c = 0; c != 3 && !failed; ++c) {
		failed = vkr_copy_to_host(channel, (const double2*) stats->sums + c * pixel_count, sizeof(double) * 2 * pixel_count, &app->device);
		for (size_t i = 0; i != pixel_count && !failed; ++i) {
			if (sums) sums[3 * i + c] = channel[2 * i];
			if (squares) squares[3 * i + c] = channel[2 * i + 1];
		}
	}
	free(channel);
	return failed;
}

static int reduce_frames(application_t* app, const void* a, const void* b, uint64_t pixel_count, double out[3], bool squared_differences) {
	if (!a || (squared_differences && !b) || !pixel_count || pixel_count > kMaxPixelCount) {
		printf("The error sums need device buffers and between 1 and %llu pixels.\n", (unsigned long long) kMaxPixelCount);
		return 1;
	}
	hipStream_t stream = device_stream(app);
	uint32_t blocks = block_count(pixel_count, kBlock);
	size_t bytes = sizeof(double) * 3 * (size_t) blocks;
	double* partials = NULL;
	double* host = (double*) malloc(bytes);
	if (!host || hipMalloc(&partials, bytes) != hipSuccess) {
		printf("Failed to allocate %llu bytes for the partial sums.\n", (unsigned long long) bytes);
		free(host);
		return 1;
	}
	// (the buffers may be outputs of frames in flight)
	int failed = finish_frames(app);
	if (!failed) {
		if (squared_differences) k_reduce_frames<true><<<blocks, kBlock, 0, stream>>>((const float4*) a, (const float4*) b, pixel_count, partials);
		else k_reduce_frames<false><<<blocks, kBlock, 0, stream>>>((const float4*) a, NULL, pixel_count, partials);
		failed = hip_failed(hipGetLastError(), "reducing a frame") || vkr_copy_to_host(host, partials, bytes, &app->device);
	}
	// the partials in block order, starting from +0.0
	for (uint32_t c = 0; c != 3 && !failed; ++c) {
		double total = 0.0;
		for (uint32_t block = 0; block != blocks; ++block) total += host[(size_t) c * blocks + block];
		out[c] = total;
	}
	(void) hipFree(partials);
	free(host);
	return failed;
}

extern "C" int sum_squared_differences(application_t* app, const void* a, const void* b, uint64_t pixel_count, double out[3]) {
	return reduce_frames(app, a, b, pixel_count, out, true);
}

extern "C" int sum_frame(application_t* app, const void* a, uint64_t pixel_count, double out[3]) {
	return reduce_frames(app, a, NULL, pixel_count, out, false);
}
