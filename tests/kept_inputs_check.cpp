// Stand-alone check of csrc/kept_inputs.h (tests/test_kept_inputs.py compiles and runs it): an image of a prefix and a
// number of records, compared the way the light shaft step compares its own - the prefix first, then every record.
#include "kept_inputs.h"
#include <stdio.h>

static int failures = 0;
#define CHECK(condition) do { if (!(condition)) { printf("line %d: %s\n", __LINE__, #condition); ++failures; } } while (0)

constexpr size_t kPrefix = 40, kRecord = 24;

struct verdict {
	bool started, prefix_same;
	uint32_t same_records;
};

// one launch: an image of `records` records whose bytes derive from `seed`, record `changed` (if any) from another seed
static verdict launch(kept_inputs* kept, inputs_scratch* scratch, uint32_t records, uint8_t seed, int changed = -1, bool keep = true) {
	verdict v = {false, false, 0u};
	const size_t size = kPrefix + kRecord * records;
	uint8_t* now = begin_inputs(kept, scratch, size);
	if (!now) return v;
	v.started = true;
	for (size_t i = 0; i != size; ++i) now[i] = (uint8_t) (seed + 7u * i);
	if (changed >= 0) now[kPrefix + kRecord * (size_t) changed + 5] ^= 0x40u;
	v.prefix_same = same_inputs(kept, now, size, 0, kPrefix);
	for (uint32_t i = 0; i != records; ++i)
		if (same_inputs(kept, now, size, kPrefix + kRecord * i, kRecord)) v.same_records |= 1u << i;
	if (keep) keep_inputs(kept, now, size);
	return v;
}

int main() {
	kept_inputs kept = {NULL, 0, 0};
	inputs_scratch scratch = {NULL, 0};
	// first image: nothing is the same
	verdict v = launch(&kept, &scratch, 4, 1);
	CHECK(v.started && !v.prefix_same && v.same_records == 0u);
	CHECK(kept.size == kPrefix + 4 * kRecord);
	// identical second image: prefix and every record the same
	v = launch(&kept, &scratch, 4, 1);
	CHECK(v.started && v.prefix_same && v.same_records == 0xFu);
	// one changed record: prefix the same, exactly that record differs - and the changed image is the kept one afterwards
	v = launch(&kept, &scratch, 4, 1, 2);
	CHECK(v.started && v.prefix_same && v.same_records == 0xBu);
	v = launch(&kept, &scratch, 4, 1, 2);
	CHECK(v.prefix_same && v.same_records == 0xFu);
	// an image that is compared and not kept leaves the kept one alone
	v = launch(&kept, &scratch, 4, 9, -1, false);
	CHECK(!v.prefix_same && v.same_records == 0u);
	v = launch(&kept, &scratch, 4, 1, 2);
	CHECK(v.prefix_same && v.same_records == 0xFu);
	// another size: nothing the same, although every byte that both images have agrees
	v = launch(&kept, &scratch, 3, 1, 2);
	CHECK(v.started && !v.prefix_same && v.same_records == 0u);
	v = launch(&kept, &scratch, 3, 1, 2);
	CHECK(v.prefix_same && v.same_records == 0x7u);
	// after forget: nothing the same
	forget_inputs(&kept);
	CHECK(kept.size == 0);
	v = launch(&kept, &scratch, 3, 1, 2);
	CHECK(v.started && !v.prefix_same && v.same_records == 0u);
	// growth keeps the kept bytes: a larger image is started, the kept one still compares equal with its own bytes
	const size_t old_size = kept.size, old_capacity = kept.capacity;
	uint8_t copy[kPrefix + 3 * kRecord];
	memcpy(copy, kept.bytes, old_size);
	uint8_t* now = begin_inputs(&kept, &scratch, 64 * old_size);
	CHECK(now != NULL && kept.capacity >= 64 * old_size && kept.capacity > old_capacity && scratch.capacity >= 64 * old_size);
	CHECK(kept.size == old_size && memcmp(kept.bytes, copy, old_size) == 0);
	CHECK(same_inputs(&kept, copy, old_size, 0, old_size));
	CHECK(!same_inputs(&kept, now, 64 * old_size, 0, kPrefix));
	// grow_bytes() on its own: content kept, no shrinking
	uint8_t* bytes = NULL;
	size_t capacity = 0;
	CHECK(grow_bytes(&bytes, &capacity, 16) == 0 && capacity == 16);
	memcpy(bytes, "0123456789abcdef", 16);
	CHECK(grow_bytes(&bytes, &capacity, 1 << 20) == 0 && capacity == (1 << 20) && memcmp(bytes, "0123456789abcdef", 16) == 0);
	CHECK(grow_bytes(&bytes, &capacity, 8) == 0 && capacity == (1 << 20));
	free(bytes);
	// an image of zero light records works
	kept_inputs none = {NULL, 0, 0};
	v = launch(&none, &scratch, 0, 3);
	CHECK(v.started && !v.prefix_same && v.same_records == 0u && none.size == kPrefix);
	v = launch(&none, &scratch, 0, 3);
	CHECK(v.started && v.prefix_same && v.same_records == 0u);
	v = launch(&none, &scratch, 0, 4);
	CHECK(!v.prefix_same);
	// an allocation that fails is reported, and the kept image counts as forgotten
	CHECK(begin_inputs(&none, &scratch, ~(size_t) 0 / 2) == NULL && none.size == 0);
	v = launch(&none, &scratch, 0, 4);
	CHECK(v.started && !v.prefix_same);
	free_inputs(&none);
	CHECK(none.bytes == NULL && none.size == 0 && none.capacity == 0);
	free_inputs(&kept);
	free(scratch.bytes);
	printf(failures ? "kept_inputs: %d checks failed\n" : "kept_inputs ok\n", failures);
	return failures != 0;
}
