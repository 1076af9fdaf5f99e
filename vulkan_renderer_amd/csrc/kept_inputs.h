// Results that are kept from launch to launch while their inputs stand still (the light shafts' verdicts, the prepared
// polygons): a launch puts a byte image of everything the result is derived from together, compares it with the image
// kept from the launch before - by memcmp, not through a hash: a collision would keep a wrong result - and keeps the new
// one.  Host code only, nothing of HIP: tests/test_kept_inputs.py compiles it on its own.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// host memory that grows on demand and keeps its content
inline int grow_bytes(uint8_t** buffer, size_t* capacity, size_t size) {
	if (*capacity >= size) return 0;
	uint8_t* grown = (uint8_t*) realloc(*buffer, size);
	if (!grown) return 1;
	*buffer = grown;
	*capacity = size;
	return 0;
}

// where the images are put together; one serves every kept result whose comparisons do not overlap
struct inputs_scratch {
	uint8_t* bytes;
	size_t capacity;
};

// the image of the most recent launch; size 0: none, the result holds nothing to lean on
struct kept_inputs {
	uint8_t* bytes;
	size_t size, capacity;
};

// Starts an image of `size` bytes in the scratch, for the caller to fill.  NULL: no memory, and the kept image is forgotten.
inline uint8_t* begin_inputs(kept_inputs* kept, inputs_scratch* scratch, size_t size) {
	if (grow_bytes(&scratch->bytes, &scratch->capacity, size) || grow_bytes(&kept->bytes, &kept->capacity, size)) {
		kept->size = 0;
		return NULL;
	}
	return scratch->bytes;
}

// whether bytes [from, from + count) of the new image of `size` bytes are those of the kept one; never across sizes
inline bool same_inputs(const kept_inputs* kept, const uint8_t* now, size_t size, size_t from, size_t count) {
	return kept->size == size && memcmp(now + from, kept->bytes + from, count) == 0;
}

// (begin_inputs() has made room)
inline void keep_inputs(kept_inputs* kept, const uint8_t* now, size_t size) {
	memcpy(kept->bytes, now, size);
	kept->size = size;
}

inline void forget_inputs(kept_inputs* kept) { kept->size = 0; }

inline void free_inputs(kept_inputs* kept) {
	free(kept->bytes);
	memset(kept, 0, sizeof(*kept));
}
