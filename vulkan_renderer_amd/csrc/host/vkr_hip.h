/* What the HIP host code of the library shares, the C99 files and the .hip units alike. */
#ifndef VKR_HIP_H
#define VKR_HIP_H
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

/*! 0 for hipSuccess; otherwise prints the error behind what was being done and returns 1 */
static inline int hip_failed(hipError_t error, const char* what) {
	if (error == hipSuccess) return 0;
	printf("HIP error while %s: %s\n", what, hipGetErrorString(error));
	return 1;
}

#ifdef __cplusplus
/*! Events that order streams of one device: a device-scope release is all they need.  The default (system-scope fence:
	L2 write-back and invalidation at every record) is paid by whatever runs next on the device, and a frame records
	several. */
constexpr unsigned kSyncEventFlags = hipEventDisableTiming | hipEventReleaseToDevice;
#endif

/*! workgroups of `block` lanes that cover `lanes` lanes */
static inline uint32_t block_count(uint64_t lanes, uint32_t block) { return (uint32_t) ((lanes + block - 1) / block); }

/*! Several temporaries in one allocation.  *total is a running offset that starts at 0: every call reserves `bytes`
	bytes, rounded up to a multiple of 256, and returns where they begin; what *total ends up as is the size to allocate. */
static inline size_t vkr_carve(size_t* total, size_t bytes) {
	size_t at = *total;
	*total = at + ((bytes + 255) & ~(size_t) 255);
	return at;
}

#endif
