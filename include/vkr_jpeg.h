/* Frames as baseline JPEG files, encoded on the device: the third screenshot format of the reference
   (stbi_write_jpg(path, w, h, 3, ldr_copy, 70) at src/main.c:1745-1752), and the cheapest way to get a frame off a GPU
   without display.  The kernels are csrc/jpeg_encoder.hip, the tables and the file header csrc/host/jpeg_tables.c, the
   numpy restatement of every byte vulkan_renderer_amd/jpeg.py.  There is no host build: device == NULL is an error. */
#ifndef VKR_JPEG_H
#define VKR_JPEG_H
#include "vkr_device.h"

/*! The header of every file: SOI, APP0, DQT, SOF0, DHT, SOS */
#define VKR_JPEG_HEADER_SIZE 607
/*! Bytes of the entropy-coded segment that one lane of the stuffing kernels handles (get_jpeg_stuffing_chunk_size()) */
#define VKR_JPEG_STUFFING_CHUNK 64

/*! An encoder for frames of one extent and quality.  It owns the tables, all device scratch and the pinned staging
	memory of its slots: encoding a frame allocates nothing.  Per slot it holds, in device memory, 128 bytes per data
	unit of coefficients, 1.5 times get_jpeg_capacity() of packed and stuffed stream and 16 bytes per data unit of
	lengths and offsets, and get_jpeg_capacity() + 16 bytes of pinned host memory. */
typedef struct jpeg_encoder_s {
	uint32_t width, height;
	/*! the effective quality, 1 ... 100 */
	uint32_t quality;
	/*! 4:2:0: 16 x 16 MCUs of six data units; otherwise 8 x 8 MCUs of three */
	VkBool32 subsampled;
	uint32_t slot_count;
	uint32_t data_unit_count;
	/*! get_jpeg_capacity(width, height, quality) */
	uint64_t capacity;
	/*! tables, scratch, staging and events (csrc/jpeg_encoder.hip) */
	void* state;
} jpeg_encoder_t;

/* ---- the calls -----------------------------------------------------------------------------------------------------

   All return 0 on success and 1 after printing one line.

   create_jpeg_encoder(): quality 0 means 90, other values are clamped to 1 ... 100; chroma is subsampled 4:2:0 if and
   only if the quality, after the 0 -> 90 substitution and before the clamp, is <= 90.  slot_count is 1 ...
   VKR_MAX_FRAMES_IN_FLIGHT + 1.  It fails, with *encoder zeroed, for device == NULL, a zero extent, an extent above
   65535 (the frame header has 16 bits) and a slot count outside that range.

   begin_jpeg_encode(): device_pixels is row-major, 8 bits per channel, channel_count 3 (packed RGB8, the out_rgb8 of
   render_shading_pass_encoded()) or 4 (RGBA8, render_targets.encoded; alpha is ignored), rows row_stride_bytes apart
   (0: width * channel_count).  Nothing outside the first height * row_stride_bytes bytes is read.  Everything is enqueued on `stream`, a
   hipStream_t (NULL: device->stream), and the call returns without waiting for the device.  Ordering the pixels against
   their producer on that stream is the caller's business.  The slot's previous encode is waited for on the device, not
   on the host.

   How the file reaches the host without a host wait for its size: the last kernel of the chain reads the size word,
   which the kernel before it left in device memory, and copies the 16-byte size record and that many bytes, sixteen per
   lane, into the slot's pinned staging memory, which is mapped into the device's address space.  Then the slot's
   event is recorded.  So only the bytes of the file cross the bus, in one kernel of a fixed, small grid; the price is
   that these are stores of a kernel to host memory instead of a DMA transfer (DESIGN.md 4.12 has the times).

   end_jpeg_encode() waits for the slot's event and hands out the file image in the staging memory, valid until the
   slot's next begin_jpeg_encode().  encode_jpeg() is begin then end on slot 0 and device->stream.

   encode_jpeg_on_device() leaves the file in the caller's device memory: at most `capacity` bytes are written to
   device_out, none at or beyond device_out + capacity, and *device_size_word (8 bytes, device memory) gets the size
   of the complete file, whether it fitted or not.  A file that did not fit is cut off at `capacity`.  It works in the
   scratch memory of slot 0 and is ordered on the device behind that slot's previous encode, as that slot's next is
   behind it.

   get_jpeg_capacity(): the size no file of that extent and quality exceeds, from the code tables: the header, then per
   data unit the longest DC code with its extra bits (11 + 11 bits) and 63 times the longest AC code with its extra
   bits (16 + 10), rounded up to bytes plus one byte of fill, all doubled because every byte may need a stuffed zero
   behind it, then EOI.  0 for an extent that create_jpeg_encoder() rejects.

   ---- the rule ------------------------------------------------------------------------------------------------------

   The rule below, the order of operations included, is the interface.  All arithmetic is binary32, every operation
   rounded on its own, nothing contracted or reordered; integer where it says so.

   TABLES.  The base quantisation tables are Tables K.1 (luminance) and K.2 (chrominance) of ITU-T T.81, the four Huffman
   specifications Tables K.3 - K.6; code words follow from the (counts, symbols) lists by the canonical construction of
   Annex C.  With q the effective quality and integer division, s = q < 50 ? 5000 / q : 200 - 2 q, and a table entry is
   clamp((base * s + 50) / 100, 1, 255).  The descaling factor of the coefficient in row r, column c of a data unit is
   1.0f / (((float) entry * a[r]) * a[c]), a[k] = A[k] * 2.828427125f, A = {1, 1.387039845, 1.306562965, 1.175875602,
   1, 0.785694958, 0.541196100, 0.275899379}.

   HEADER, 607 bytes: SOI; APP0 "JFIF", version 1.1, no units, density 1 x 1, no thumbnail; one DQT with table 0
   (luminance) and table 1 (chrominance), entries in zig-zag order; SOF0 with 8 bits, height, width, three components:
   1 sampled 2x2 if subsampled else 1x1 with table 0, 2 and 3 sampled 1x1 with table 1; one DHT with DC 0, AC 0, DC 1,
   AC 1; SOS for the three components, component 1 with tables 0/0, the others with 1/1, spectral selection 0 ... 63.

   PIXELS.  An MCU covers 16 x 16 pixels if subsampled, else 8 x 8; MCUs go row by row.  A coordinate beyond the image
   takes the last column or row.  With r, g, b the channel values as floats:
     Y = ((0.299f r + 0.587f g) + 0.114f b) - 128
     U = (-0.16874f r - 0.33126f g) + 0.5f b
     V = (0.5f r - 0.41869f g) - 0.08131f b
   Subsampled, a chroma sample is (((a00 + a01) + a10) + a11) * 0.25f of the U or V of its 2 x 2 pixels (a01 to the
   right of a00, a10 below it).  Data units per MCU: Y top-left, top-right, bottom-left, bottom-right, U, V if
   subsampled, else Y, U, V.

   DCT.  The forward transform of Arai, Agui and Nakajima on the eight values d0 ... d7 of a row, for all rows, then of a
   column, for all columns:
     t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
     e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2
     D0 = e0 + e1, D4 = e0 - e1, z1 = (e2 + e3) * 0.707106781f, D2 = e3 + z1, D6 = e3 - z1
     o0 = t4 + t5, o1 = t5 + t6, o2 = t6 + t7
     z5 = (o0 - o2) * 0.382683433f, z2 = o0 * 0.541196100f + z5, z4 = o2 * 1.306562965f + z5, z3 = o1 * 0.707106781f
     z11 = t7 + z3, z13 = t7 - z3
     D5 = z13 + z2, D3 = z13 - z2, D1 = z11 + z4, D7 = z11 - z4

   QUANTISATION.  v = coefficient * factor; the integer is v < 0 ? v - 0.5f : v + 0.5f, truncated towards zero, and
   stands at the coefficient's zig-zag position.

   ENTROPY CODING follows T.81 F.1.2.  The DC difference is taken to the previous data unit of the same component, the
   first one to 0.  A value n != 0 of category c (the bit count of |n|) is coded as its Huffman code and the low c bits
   of n if n > 0, of n - 1 otherwise; a DC difference of 0 as the code of category 0 alone.  In front of a nonzero
   coefficient with z zeros before it stand z / 16 codes ZRL (0xF0), then the code of (z % 16) * 16 + c.  EOB (0x00)
   closes the data unit unless coefficient 63 is nonzero.  (A symbol without a code - an AC category above 10, which 8-bit
   pixels do not reach - contributes its extra bits alone, as in the writer.)  Bits are packed most significant first.
   A last partial byte is filled with ones; a stream that ends on a byte boundary gets no byte.  Every 0xFF byte of the
   segment, a filled last byte included, is followed by 0x00.  Then comes EOI. */
VKR_API int create_jpeg_encoder(jpeg_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, int32_t quality, uint32_t slot_count);
VKR_API void destroy_jpeg_encoder(jpeg_encoder_t* encoder);
VKR_API int begin_jpeg_encode(jpeg_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, void* stream);
VKR_API int end_jpeg_encode(jpeg_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_jpeg(jpeg_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_jpeg_on_device(jpeg_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes,
                                  void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream);
VKR_API uint64_t get_jpeg_capacity(uint32_t width, uint32_t height, int32_t quality);
/*! VKR_JPEG_STUFFING_CHUNK, for tests that place 0xFF bytes on the borders between lanes */
VKR_API uint32_t get_jpeg_stuffing_chunk_size(void);
/*! The 607 bytes of the header for an extent and quality; 1 for an extent that create_jpeg_encoder() rejects */
VKR_API int get_jpeg_header(uint8_t header[VKR_JPEG_HEADER_SIZE], uint32_t width, uint32_t height, int32_t quality);
/*! Writes the file.  Returns 0 on success. */
VKR_API int write_jpeg(const char* path, const uint8_t* bytes, uint64_t size);

#endif
