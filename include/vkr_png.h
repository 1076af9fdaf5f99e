/* Frames as PNG files, encoded on the device: the default screenshot format of the reference (stbi_write_png at
   src/main.c:1738) and the lossless file of the LDR frame.  The inflated IDAT stream - filter bytes and filtered rows - is
   the one of the reference's writer and of write_png_rgb8(), byte for byte; the compressed bytes are this encoder's own:
   the writer's deflate is one serial hash-chain walk, this one is stated so that it can be computed in parallel and uses
   dynamic Huffman codes, which the writer does not.  The kernels and the host side are csrc/png_encoder.hip, the numpy
   restatement of every byte vulkan_renderer_amd/png.py.  There is no host build: device == NULL is an error. */
#ifndef VKR_PNG_H
#define VKR_PNG_H
#include "vkr_device.h"

/*! Signature and IHDR: the bytes in front of the first IDAT (get_png_header()) */
#define VKR_PNG_HEADER_SIZE 33
/*! Bytes of a row of the filtered stream that are parsed on their own: no token crosses the end of a unit */
#define VKR_PNG_UNIT 4096
/*! A segment - one deflate block, one IDAT chunk - has as many whole rows as fit into this many bytes, at least one */
#define VKR_PNG_SEGMENT_BYTES 65536

/*! An encoder for frames of one extent.  It owns all device scratch and the pinned staging memory of its slots: encoding
	a frame allocates nothing.  Per slot it holds, in device memory, 3 bytes per byte of the filtered stream (the stream
	and two bytes of token per position), get_png_capacity() + 16 bytes of file, 24 bytes per unit and 3 KB per segment
	of counts, code tables and block headers, and get_png_capacity() + 16 bytes of pinned host memory. */
typedef struct png_encoder_s {
	uint32_t width, height;
	uint32_t slot_count;
	/*! bytes per row of the filtered stream, 3 * width + 1, and rows of a segment */
	uint32_t row_length, rows_per_segment;
	uint32_t segment_count;
	/*! get_png_capacity(width, height) */
	uint64_t capacity;
	/*! scratch, staging and events (csrc/png_encoder.hip) */
	void* state;
} png_encoder_t;

/* ---- the calls -----------------------------------------------------------------------------------------------------

   All return 0 on success and 1 after printing one line.

   create_png_encoder(): slot_count is 1 ... VKR_MAX_FRAMES_IN_FLIGHT + 1.  It fails, with *encoder zeroed, for
   device == NULL, a zero extent, an extent above 65535 and a slot count outside that range.

   begin_png_encode(): device_pixels is row-major, 8 bits per channel, channel_count 3 (packed RGB8, the out_rgb8 of
   render_shading_pass_encoded()) or 4 (RGBA8, render_targets.encoded; alpha is ignored), rows row_stride_bytes apart
   (0: width * channel_count).  Nothing outside the first height * row_stride_bytes bytes is read.  Everything is enqueued
   on `stream`, a hipStream_t (NULL: device->stream), and the call returns without waiting for the device.  Ordering the
   pixels against their producer on that stream is the caller's business.  The slot's previous encode is waited for on
   the device, not on the host.

   How the file reaches the host without a host wait for its size: the last kernel of the chain reads the size word,
   which the kernel before it left in device memory, and copies the 16-byte size record and that many bytes, sixteen per
   lane, into the slot's pinned staging memory, which is mapped into the device's address space.  Then the slot's event
   is recorded.  So only the bytes of the file cross the bus (DESIGN.md 4.14 has the times).

   end_png_encode() waits for the slot's event and hands out the file image in the staging memory, valid until the
   slot's next begin_png_encode().  encode_png() is begin then end on slot 0 and device->stream.

   encode_png_on_device() leaves the file in the caller's device memory: at most `capacity` bytes are written to
   device_out, none at or beyond device_out + capacity, and *device_size_word (8 bytes, device memory) gets the size of
   the complete file, whether it fitted or not.  A file that did not fit is cut off at `capacity`.  It works in the
   scratch memory of slot 0 and is ordered on the device behind that slot's previous encode, as that slot's next is
   behind it.

   get_png_capacity(): the size no file of that extent exceeds (CAPACITY below); 0 for an extent that
   create_png_encoder() rejects.

   ---- the rule ------------------------------------------------------------------------------------------------------

   The rule below is the interface: restatement and device agree in every byte.  All of it is integer arithmetic.

   FILE.  The signature; IHDR with width, height, 8 bits, colour type 2 and 0, 0, 0; one IDAT chunk per segment; IEND.
   Input alpha is dropped: the file always has three channels, as the reference's.

   FILTERED STREAM F.  `height` rows of L = 3 * width + 1 bytes: the filter byte, then the residuals (value - prediction)
   mod 256 of that filter.  With a the byte three to the left, b the byte above and c the byte above a, each 0 outside
   the image, the predictions are 0: 0, 1: a, 2: b, 3: (a + b) >> 1, 4: Paeth (p = a + b - c; a if |p - a| <= |p - b| and
   |p - a| <= |p - c|, else b if |p - b| <= |p - c|, else c).  A row takes the filter with the smallest sum of |residual
   as a signed char|; among equal sums the lowest filter number.  This is what stbi_write_png does with its filter
   heuristic, whose first-row variants are these filters with a zero row above.

   SEGMENTS.  R = clamp(65536 / L, 1, height) rows each (integer division), the last one what is left.  A segment is one
   deflate block.

   TOKENS.  A row of F is cut into units of 4096 bytes, the last one shorter.  With i, j positions in F as a whole: the
   candidate distances are 1, 3 and L, the latter only if L <= 32768.  The length of distance d at i is the number of
   consecutive j >= i inside i's unit with j - d >= 0 and F[j] = F[j - d], at most 258: a match may refer to any earlier
   byte, also of an earlier unit or segment, but covers bytes of its own unit only.  From the unit's start on, the
   parse takes at i the candidate with the greatest length if that is >= 3 - among equal lengths the one named first in
   "1, 3, L" - and goes on at i + length; otherwise the literal F[i], and goes on at i + 1.

   CODES, per segment.  Counts are taken over the 286 literal and length symbols, the end of block counted once, and
   over the 30 distance symbols.  Code lengths of an alphabet from its counts and a limit:
     1. while fewer than two symbols have a count, the lowest-numbered symbol without one gets the count 1 (in practice
        the distance alphabet only; the bits of the block are computed with the counts as they were);
     2. the symbols with a count, sorted by (count, symbol), are the leaves.  Until one node is left, the two lightest
        nodes are joined, taken one after the other from the front of the leaves and the front of the joined nodes in
        the order of their making - a leaf where both weigh the same -, into a node of their summed weight, which goes to
        the back of the joined nodes.  A symbol's length is its leaf's depth;
     3. if a length exceeds the limit, every count c > 0 becomes (c + 1) >> 1 and step 2 is repeated.
   The limit is 15 for both alphabets.  Codes are the canonical ones of RFC 1951 3.2.2.  A dynamic block header sends
   HLIT = 29, HDIST = 29, HCLEN = 15, the 19 lengths of the code-length code in the order of the RFC and then all 316
   lengths, literal and length symbols first, each as its own symbol 0 ... 15: no repeat codes.  The code-length code
   comes from the counts of the values 0 ... 15 among those 316 lengths by the same steps with the limit 7.
   The block is dynamic if its bits - header, tokens, end of block - are fewer than those of the fixed code of RFC 1951
   3.2.6 for the same tokens, otherwise fixed.  No stored block holds data.

   FRAMING.  The first IDAT begins with the zlib header 78 5E.  A block begins at a byte border with BFINAL - 1 in the
   last segment - and BTYPE.  Behind every block but the last come the bits 000, zeros up to the byte border and
   00 00 FF FF: an empty stored block.  The last block is filled up with zero bits and followed by the Adler-32 of F,
   most significant byte first.  Every IDAT has its own CRC-32.

   CAPACITY.  In the fixed code no token takes more than 9 bits per byte that it covers: a literal 8 or 9 bits; a match
   of 3 ... 10 bytes 7 + 5 + 13 = 25 <= 27 bits, of 11 ... 114 bytes at most 7 + 4 + 5 + 13 = 29 <= 99 bits, of more at
   most 8 + 5 + 5 + 13 = 31.  A chosen block never exceeds the fixed one.  So a segment of n bytes of F has at most
   3 + 9 n + 7 bits of block and 3 of the stored block's header: (9 n + 20) / 8 bytes with the border, then 4 bytes of
   stored block or Adler-32, in 12 bytes of chunk.  get_png_capacity() = 33 + 2 + 12 + the sum over the segments of
   (9 n + 20) / 8 + 16, in 64 bits. */
VKR_API int create_png_encoder(png_encoder_t* encoder, const device_t* device, uint32_t width, uint32_t height, uint32_t slot_count);
VKR_API void destroy_png_encoder(png_encoder_t* encoder);
VKR_API int begin_png_encode(png_encoder_t* encoder, uint32_t slot, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, void* stream);
VKR_API int end_png_encode(png_encoder_t* encoder, uint32_t slot, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_png(png_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes, const uint8_t** bytes, uint64_t* size);
VKR_API int encode_png_on_device(png_encoder_t* encoder, const void* device_pixels, uint32_t channel_count, uint64_t row_stride_bytes,
                                 void* device_out, uint64_t capacity, uint64_t* device_size_word, void* stream);
VKR_API uint64_t get_png_capacity(uint32_t width, uint32_t height);
/*! The 33 bytes in front of the first IDAT; 1 for an extent that create_png_encoder() rejects */
VKR_API int get_png_header(uint8_t header[VKR_PNG_HEADER_SIZE], uint32_t width, uint32_t height);
/*! Writes the file.  Returns 0 on success. */
VKR_API int write_png_file(const char* path, const uint8_t* bytes, uint64_t size);

/*! TEST PROBE.  Everything behind the filter for a filtered stream of the caller's: `host_stream` holds `rows` rows of
	row_length bytes (host memory; row_length 1 ... 262144, rows 1 ... 65535) and is taken as F with L = row_length, so
	that streams which the filter heuristic never produces reach tokens, codes, framing and checksums.  IHDR gets
	row_length as width and rows as height: the file is a PNG container around a zlib stream of the bytes, not an image.
	At most out_capacity bytes go to `out` (host memory), *out_size gets the size of the file; get_png_stream_capacity()
	bounds it.  Returns 0 on success. */
VKR_API int probe_png_stream(const device_t* device, const uint8_t* host_stream, uint32_t row_length, uint32_t rows, uint8_t* out, uint64_t out_capacity, uint64_t* out_size);
/*! CAPACITY for a stream of the probe; 0 for one it rejects */
VKR_API uint64_t get_png_stream_capacity(uint32_t row_length, uint32_t rows);

#endif
