/* Frames as Radiance RGBE *.hdr files, encoded on the device: the screenshot format of the reference that keeps the float
   values of a frame (stbi_write_hdr at src/main.c:1757), byte for byte the file that writer makes.  A file is at most
   4.04 bytes per pixel, so that it crosses the bus instead of 16 bytes of RGBA32F per pixel.  The kernels and the host
   side are csrc/hdr_encoder.hip, the numpy restatement of every byte vulkan_renderer_amd/hdr.py.  There is no host
   build: device == NULL is an error. */
#ifndef VKR_HDR_H
#define VKR_HDR_H
#include "vkr_device.h"

/*! No header is longer (two extents of five digits) */
#define VKR_HDR_MAX_HEADER_SIZE 128
/*! Elements of a component plane that one wave codes per step (get_hdr_chunk_size()) */
#define VKR_HDR_CHUNK 64
/*! Pixels of a row that a workgroup stages in LDS at a time, a multiple of VKR_HDR_CHUNK (get_hdr_segment_size()) */
#define VKR_HDR_SEGMENT 1024

/*! An encoder for frames of one extent.  It owns the header, all device scratch and the pinned staging memory of its
	slots: encoding a frame allocates nothing.  Per slot it holds, in device memory, 4 bytes per pixel of RGBE, 32 bytes
	per row of sizes and offsets and get_hdr_capacity() + 16 bytes of file, and get_hdr_capacity() + 16 bytes of pinned
	host memory. */
typedef struct hdr_encoder_s {
	uint32_t width, height;
	uint32_t slot_count;
	/*! the bytes of the header (get_hdr_header()) */
	uint32_t header_size;
	/*! whether rows are run-length coded: 8 <= width < 32768 */
	VkBool32 run_length_coded;
	/*! get_hdr_capacity(width, height) */
	uint64_t capacity;
	/*! header, scratch, staging and events (csrc/hdr_encoder.hip) */
	void* state;
} hdr_encoder_t;

/* ---- the calls -----------------------------------------------------------------------------------------------------

   All return 0 on success and 1 after printing one line.

   create_hdr_encoder(): slot_count is 1 ... VKR_MAX_FRAMES_IN_FLIGHT + 1.  It fails, with *encoder zeroed, for
   device == NULL, a zero extent, an extent above 65535 and a slot count outside that range.

   begin_hdr_encode(): device_pixels is row-major binary32, channel_count 3 (RGB) or 4 (RGBA: render_targets.radiance,
   the images of resolve_frame_statistics(); the fourth channel is ignored), rows row_stride_bytes apart (0: width *
   channel_count * 4; a multiple of 4).  Nothing outside the first height * row_stride_bytes bytes is read.  through_half:
   see SANITISE.  Everything is enqueued on `stream`, a hipStream_t (NULL: device->stream), and the call returns without
   waiting for the device.  Ordering the pixels against their producer on that stream is the caller's business.  The
   slot's previous encode is waited for on the device, not on the host.

   How the file reaches the host without a host wait for its size: the last kernel of the chain reads the size word,
   which the kernel before it left in device memory, and copies the 16-byte size record and that many bytes, sixteen per
   lane, into the slot's pinned staging memory, which is mapped into the device's address space.  Then the slot's
   event is recorded.  So only the bytes of the file cross the bus, in one kernel of a fixed, small grid; the price is
   that these are stores of a kernel to host memory instead of a DMA transfer (DESIGN.md 4.13 has the times).

   end_hdr_encode() waits for the slot's event and hands out the file image in the staging memory, valid until the
   slot's next begin_hdr_encode().  encode_hdr() is begin then end on slot 0 and device->stream.

   encode_hdr_on_device() leaves the file in the caller's device memory: at most `capacity` bytes are written to
   device_out, none at or beyond device_out + capacity, and *device_size_word (8 bytes, device memory) gets the size
   of the complete file, whether it fitted or not.  A file that did not fit is cut off at `capacity`.  It works in the
   scratch memory of slot 0 and is ordered on the device behind that slot's previous encode, as that slot's next is
   behind it.

   get_hdr_capacity(): the size no file of that extent exceeds (CAPACITY below); 0 for an extent that
   create_hdr_encoder() rejects.

   ---- the rule ------------------------------------------------------------------------------------------------------

   The rule below, the order of operations included, is the interface.  All arithmetic is binary32.

   SANITISE.  A channel value c becomes c >= 0 ? min(c, FLT_MAX) : 0: NaN and negative values become 0, +inf becomes
   FLT_MAX.  This is the identity for every value on which the writer's behaviour is defined (it casts out-of-range
   floats to unsigned char and calls frexp on inf).  With through_half set, c is first rounded to binary16, to nearest
   even - the half whose bytes encode_output() writes with frame_bits 1 and 2 -, widened exactly as half_to_float()
   does, and then sanitised: the float that take_screenshot() hands to its writer.

   RGBE.  m = max(r, max(g, b)) with max(a, b) = a > b ? a : b.  If m < 1e-32f the four bytes are 0.  Otherwise
   m = f * 2^e with f in [0.5, 1); m is not subnormal here, so e is its biased exponent minus 126.  normalize =
   f * 256.0f / m is exactly 2^(8 - e): f * 256 is exact and the quotient of the two is a power of two.  The device
   builds normalize from the exponent bits, the restatement divides; both give the same float.  The colour bytes are
   (uint8) (c * normalize), truncated; the fourth byte is the low eight bits of e + 128 (FLT_MAX has e = 128: byte 0,
   as in the writer).

   FILE.  The header is the writer's: "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\n"
   "EXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n" with height and width.  It is made on the host and uploaded
   once per encoder.  Rows go top to bottom.  For width < 8 or width >= 32768 a row is its RGBE quadruples.  Otherwise
   a row is {2, 2, width >> 8, width & 255} followed by the four component planes R, G, B, E, each run-length coded.

   RUN-LENGTH CODING of a plane, stated without a cursor.  Cut the plane into maximal stretches of equal bytes.  A
   stretch of length >= 3 is a run.  Consecutive shorter stretches between two runs, before the first run or after the
   last run merge into one dump.  A dump of length L is written from its start in packets of at most 128 bytes:
   {n, n bytes}.  A run of length R is written from its start in packets of at most 127: {128 + n, value}; a run of 128
   is therefore {255, v} {129, v}.  This equals the writer's cursor loop: its search always starts at a stretch border,
   so the first triple of equal bytes it finds is the start of a maximal stretch.
   Per element, with k the element's offset in its dump or run: a dump element costs 1 byte, plus 1 where k % 128 == 0;
   a run element costs 2 bytes where k % 127 == 0 and 0 otherwise.  The exclusive sum of these costs is every element's
   position in the coded plane.  The kernels compute exactly this: equality with the left neighbour per element, runs
   from three such bits, the start of the stretch and of the dump as the last set bit at or before the element, the
   positions as a sum over lanes and a carry over the chunks of the row.  The count byte of a packet is written by the
   lane of the packet's last element, which alone knows it; every byte of the file is written by exactly one lane.

   CAPACITY.  A coded plane never exceeds width + (width + 127) / 128 bytes, and reaches that only without runs: a run
   of R >= 3 costs at most R - 1, and every dump but the first follows a run.  get_hdr_capacity(width, height) = header
   size + height * (4 + 4 * (width + (width + 127) / 128)) for run-length coded widths and header size + 4 * width *
   height for the others, in 64 bits. */
VKR_API int create_hdr_encoder(hdr_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count);
VKR_API void destroy_hdr_encoder(hdr_encoder_t* encoder);
VKR_API int begin_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, void* stream);
VKR_API int end_hdr_encode(hdr_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_hdr(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_hdr_on_device(hdr_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, VkBool32 through_half,
                                 void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream);
VKR_API uint64_t get_hdr_capacity(uint32_t width, uint32_t height);
/*! VKR_HDR_CHUNK, for tests that place runs and dumps on the borders between the chunks of a row */
VKR_API uint32_t get_hdr_chunk_size(void);
/*! VKR_HDR_SEGMENT, the other border inside a row */
VKR_API uint32_t get_hdr_segment_size(void);
/*! The header for an extent; returns its size in bytes, 0 for an extent that create_hdr_encoder() rejects */
VKR_API uint32_t get_hdr_header(char header[VKR_HDR_MAX_HEADER_SIZE], uint32_t width, uint32_t height);
/*! Writes the file.  Returns 0 on success. */
VKR_API int write_hdr_file(const char* path, const uint8_t* bytes, uint64_t size);

#endif
